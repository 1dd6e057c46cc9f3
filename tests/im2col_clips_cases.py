"""The per-clip form of the patch-embedding operand load (MAEST_IM2COL_CLIP_TOKENS on maest_patch_im2col(_strided): csrc/embed.hip
patch_im2col_clips_kernel; ops.patch_im2col with a 3-D table) and ops.token_assemble_clips; run by test_emu_im2col_clips.py under the
emulator and by test_im2col_clips_gpu.py on the device, in both builds.

The condition is EQUALITY, never a tolerance: include/maest_hip.h defines the form as the shared form's arithmetic per element, so the
flagged call must equal, with torch.equal on the bits, the shared form called clip by clip with that clip's table (the whole batch goes
in, so that a mixup partner is there; the rows of clip b are compared).  A blank entry is all-zero bits whatever x holds."""
import functools

import numpy as np
import pytest
import torch

from maest_amd import _lib, ops
from tests import guard
from tests.kernel_cases import f16_build, rnd

FDIM, T = 96, 256                       # the mel of the model test's clips: a 9 x 25 grid at stride (10, 10)
SHAPES = [(1, 1), (3, 7), (2, 225)]     # (B, P): the minimum; a ragged last workgroup (336 threads); the model test's grid
STRIDES = [(10, 10), (8, 12)]           # (frequency, time): the published one, and one whose grid (11 x 21) has another shape
X_DTYPES = [torch.float32, torch.float16]
OUT_DTYPES = [torch.float32, torch.bfloat16]      # (torch.bfloat16: the 16-bit container of the build that runs)
BIG = (2, 4_200_000)                    # B * P * 256 = 2.15e9 > 2^31 output elements (the device only)


def grid_of(stride):
    return (FDIM - 16) // stride[0] + 1, (T - 16) // stride[1] + 1


@functools.lru_cache(maxsize=None)
def table(B, P, stride):
    """int32 [B, P, 2], shared, never modified: every clip another list of distinct (f, t) positions -- clip 0 ascending and holding the
    last valid position, the last clip of B > 1 in descending order, the others unordered."""
    Fp, Tp = grid_of(stride)
    rng = np.random.Generator(np.random.PCG64(100 * B + P + stride[0]))
    rows = []
    for b in range(B):
        if P <= Fp * Tp:
            pos = rng.permutation(Fp * Tp)[:P]
            if b == 0:
                pos[0] = Fp * Tp - 1 if Fp * Tp - 1 not in pos else pos[0]
                pos = np.sort(pos)
            elif b == B - 1:
                pos = np.sort(pos)[::-1].copy()
        else:
            pos = rng.integers(0, Fp * Tp, P)       # (BIG: more rows than positions)
        rows.append(np.stack([pos // Tp, pos % Tp], -1))
    t = torch.from_numpy(np.stack(rows).astype(np.int32))
    assert int(t[..., 0].max()) < Fp and int(t[..., 1].max()) < Tp and t.min() >= 0
    if P <= Fp * Tp:
        assert tuple(t[0, -1].tolist()) == (Fp - 1, Tp - 1), "clip 0 must end at the last valid (f, t)"
    if B > 1 and P > 1:
        assert not torch.equal(t[0], t[1])
    return t


@functools.lru_cache(maxsize=None)
def operand(B, dtype):
    return rnd((B, FDIM, T), 7 + B).to(dtype)


def options(B, mix, masked):
    """perm / lam and the stripe lists of a case (CPU tensors), or Nones."""
    rng = np.random.Generator(np.random.PCG64(50 + B))
    kw = dict(perm=None, lam=None, t_stripes=None, f_stripes=None)
    if mix:
        kw["perm"] = torch.from_numpy(np.roll(np.arange(B), 1).astype(np.int32))
        kw["lam"] = torch.from_numpy(rng.random(B).astype(np.float32))
    if masked:
        kw["t_stripes"] = torch.from_numpy(np.stack([rng.integers(0, T - 8, (B, 3)), rng.integers(0, 30, (B, 3))], -1).astype(np.int32))
        kw["f_stripes"] = torch.from_numpy(np.stack([rng.integers(0, FDIM - 5, (B, 2)), rng.integers(0, 6, (B, 2))], -1).astype(np.int32))
    return kw


def _to(dev, kw):
    return {k: v if v is None or not torch.is_tensor(v) else v.to(dev) for k, v in kw.items()}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _say(what, B, P, **kw):
    print(f"im2col per clip, {what}, {'f16' if f16_build() else 'bf16'} build, B = {B}, P = {P}, {kw}")


def shared_by_clip(x, tok, out_dtype, stride, kw):
    """The shared form called clip by clip with that clip's table -> [B * P, 256]."""
    B, P = tok.shape[:2]
    return torch.cat([ops.patch_im2col(x, tok[b].contiguous(), out_dtype, stride=stride, **kw)[b * P:(b + 1) * P] for b in range(B)])


def case_equal(dev, B, P, x_dtype, out_dtype, stride, mix=False, masked=False):
    _say("equality with the shared form clip by clip", B, P, x=x_dtype, out=out_dtype, stride=stride, mix=mix, masked=masked)
    x, tok, kw = operand(B, x_dtype).to(dev), table(B, P, stride).to(dev), _to(dev, options(B, mix, masked))
    got = ops.patch_im2col(x, tok, out_dtype, stride=stride, **kw)
    assert got.shape == (B * P, 256) and got.dtype == out_dtype
    assert torch.equal(bits(got), bits(shared_by_clip(x, tok, out_dtype, stride, kw))), "the per-clip form differs from the shared form"
    if not mix and not masked and x_dtype == torch.float32 and out_dtype == torch.float32:      # and what both are: the patch itself
        t0 = tok.cpu()
        for b, j in ((0, 0), (B - 1, P - 1)):
            f, t = (int(v) for v in t0[b, j])
            want = operand(B, x_dtype)[b, f * stride[0]:f * stride[0] + 16, t * stride[1]:t * stride[1] + 16].reshape(256)
            assert torch.equal(got[b * P + j].cpu(), want), f"row ({b}, {j}) is not the patch at ({f}, {t})"


def case_broadcast(dev, B, P, out_dtype, stride):
    """A table without blank bits under the flag equals the unflagged call on a broadcast table."""
    _say("a broadcast table against the unflagged call", B, P, out=out_dtype, stride=stride)
    x, tok = operand(B, torch.float32).to(dev), table(B, P, stride)[0].contiguous().to(dev)
    kw = _to(dev, options(B, B > 1, True))
    flagged = ops.patch_im2col(x, tok.unsqueeze(0).expand(B, P, 2).contiguous(), out_dtype, stride=stride, **kw)
    assert torch.equal(bits(flagged), bits(ops.patch_im2col(x, tok, out_dtype, stride=stride, **kw)))


def case_blank(dev, out_dtype, x_dtype, mix):
    """B = 3, P = 7: every token of clip 1 is blank and x[1] is all NaN -> all-zero bits, with mixup too (clip 1's partner is finite, and
    clip 2, whose partner is clip 1, is NaN as the shared form makes it); two blank tokens of clip 0 are zero rows among rows that equal
    the shared form's."""
    B, P, stride = 3, 7, (10, 10)
    _say("blank tokens over NaN samples", B, P, out=out_dtype, x=x_dtype, mix=mix)
    x = operand(B, x_dtype).clone()
    x[1] = float("nan")
    x = x.to(dev)
    tok = table(B, P, stride).clone()
    blank = torch.zeros((B, P), dtype=torch.bool)
    blank[1] = True
    blank[0, 2] = blank[0, 6] = True
    marked = tok.clone()
    marked[..., 0] |= blank.to(torch.int32) * _lib.TOK_BLANK
    kw = _to(dev, options(B, mix, True))
    got = bits(ops.patch_im2col(x, marked.to(dev), out_dtype, stride=stride, **kw)).cpu().reshape(B, P, 256)
    ref = bits(shared_by_clip(x, tok.to(dev), out_dtype, stride, kw)).cpu().reshape(B, P, 256)
    assert not bool(got[blank].any()), "a blank row holds a set bit"
    assert bool((ref[1] != 0).any()), "(the unmarked rows of the NaN clip are not zero: the case can tell)"
    assert torch.equal(got[~blank], ref[~blank]), "a row that is not blank differs from the shared form"


def case_argument_errors(dev):
    """The refusals of the flagged entry, and the unflagged entry as it was: MAEST_ERR_INVALID (status 1) and its message."""
    B, P, stride = 2, 3, (10, 10)
    x, tok = operand(B, torch.float32).to(dev), table(B, P, stride).to(dev)
    out = torch.zeros((B * P, 256), dtype=torch.float32, device=dev)
    out16 = torch.zeros((B * P, 256), dtype=torch.bfloat16, device=dev)
    C = _lib.IM2COL_CLIP_TOKENS
    st = ops._s(x)

    def call(code, o=out, entry="maest_patch_im2col_strided", t=tok):
        args = [ops._p(x), _lib.F32, B, FDIM, T] + ([10, 10] if entry.endswith("strided") else [])
        _lib.call(entry, *args, None, None, ops._p(t), P, None, 0, None, 0, ops._p(o), code, st)

    def refused(match, *a, **kw):
        with pytest.raises(_lib.MaestHipError, match=match) as e:
            call(*a, **kw)
        assert "status 1" in str(e.value)

    for entry in ("maest_patch_im2col_strided", "maest_patch_im2col"):
        for extra in (0x200, 0x400, 0x8000, 1 << 16, 1 << 30):
            refused("unknown flag bits", _lib.F32 | C | extra, entry=entry)
            refused("bad dtype", _lib.F32 | extra, entry=entry)                  # without the flag: the entry as it was
        for base in (_lib.F32X3, _lib.F16, _lib.BF16_QS, 0xFF):
            refused("bad dtype", base | C, entry=entry)
            refused("bad dtype", base, entry=entry)
        call(_lib.F32 | C, entry=entry)
        call(_lib.BF16 | C, o=out16, entry=entry)
        assert torch.equal(out, ops.patch_im2col(x, tok, torch.float32)) and torch.equal(bits(out16), bits(ops.patch_im2col(x, tok, torch.bfloat16)))
    refused("null pointer", _lib.F32 | C, t=None)


def _assemble_args(dev, Fp, Tt):
    return [t.to(dev) for t in (rnd((768,), 40, .02), rnd((768,), 41, .02), rnd((2, 768), 42, .02), rnd((768, Fp), 43, .02), rnd((768, Tt), 44, .02))]


def case_token_assemble_clips(dev, B, P, toffset=1):
    """ops.token_assemble_clips against ops.token_assemble clip by clip with that clip's table (torch.equal: the arithmetic of the
    [B, 2 + P, 768] call per element); blank bits in the table change nothing: the token keeps its positional terms."""
    stride = (10, 10)
    Fp, Tp = grid_of(stride)
    _say("token assembly against the shared call clip by clip", B, P)
    tok = table(B, P, stride)
    marked = tok.clone()
    marked[:, ::2, 0] |= _lib.TOK_BLANK
    patches = rnd((B * P, 768), 45).to(dev)
    args = _assemble_args(dev, Fp, Tp + 2)
    got = ops.token_assemble_clips(patches, *args, toffset, marked.to(dev), B)
    assert got.shape == (B, 2 + P, 768) and got.dtype == torch.float32
    for b in range(B):
        want = ops.token_assemble(patches[b * P:(b + 1) * P].contiguous(), *args, toffset, tok[b].contiguous().to(dev), 1)
        assert torch.equal(bits(got[b]), bits(want[0])), f"clip {b} differs from token_assemble with its table"


def case_regions(dev, B, P, out_dtype):
    """Inside a guard (the caller's guard.covering): `out`, allocated by the wrapper and filled with the guard's pattern, is written in
    exactly [B * P, 256] -- every element, blank rows included, nothing in the bands --, and x, the table, perm / lam and the stripes are
    bitwise unchanged (the guard checks the arena of a const argument).  The same for ops.token_assemble_clips."""
    assert guard.guarded._active is not None
    stride = (10, 10)
    x = operand(B, torch.float32).to(dev)
    marked = table(B, P, stride).clone()
    marked[-1, -1, 0] |= _lib.TOK_BLANK
    tok = marked.to(dev)
    kw = _to(dev, options(B, B > 1, True))
    got = ops.patch_im2col(x, tok, out_dtype, stride=stride, **kw)
    assert got.shape == (B * P, 256) and got.is_contiguous()
    assert not bool(guard.untouched(got).any()), "elements of out were never written"
    assert not bool(bits(got[-1]).any()), "the blank row is not zero"
    assert torch.equal(x.cpu(), operand(B, torch.float32)) and torch.equal(tok.cpu(), marked)
    Fp, Tp = grid_of(stride)
    x0 = ops.token_assemble_clips(rnd((B * P, 768), 45).to(dev), *_assemble_args(dev, Fp, Tp), 0, tok, B)
    assert not bool(guard.untouched(x0).any())


def case_big(dev):
    """Output offsets past 2^31 elements: B * P = 8.4e6 rows of 256; 16-bit output, the two clips against the shared form."""
    B, P = BIG
    stride = (10, 10)
    _say("offsets past 2^31", B, P)
    assert B * P * 256 > 2 ** 31
    x, tok = operand(B, torch.float16).to(dev), table(B, P, stride).to(dev)
    got = ops.patch_im2col(x, tok, torch.bfloat16, stride=stride)
    for b in range(B):
        want = ops.patch_im2col(x, tok[b].contiguous(), torch.bfloat16, stride=stride)[b * P:(b + 1) * P]
        assert torch.equal(bits(got[b * P:(b + 1) * P]), bits(want)), f"clip {b} differs"
        del want
