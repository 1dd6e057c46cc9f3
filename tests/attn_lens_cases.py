"""Token counts per clip in the attention forward (MAEST_ATTN_LENS, ops.attn_fwd(n_tok=...)): the cases shared by test_emu_attn_lens.py
(the emulator) and test_attn_lens_gpu.py (the device), in both builds -- a sibling of attn_probs_cases.

The contract (include/maest_hip.h): clip b attends over its first n_b = n_tok[b] rows; rows >= n_b of qkv are never read; written rows
>= n_b leave as +0.0; rows the unflagged call leaves unwritten stay unwritten; n_tok is only read.  Masked keys contribute exact zeros and
the key tiles are walked in the order of an unflagged call at N = n_b, so every form is held to BIT EQUALITY with that call on the clip
alone -- and, because nobody gated the unflagged kernels at the shortest of these lengths before, every clip is also held to the fp64
softmax of its stored operands at the tolerance the existing cases apply to the same form:

    fp32                     kernel_cases.tol(torch.float32) = (2e-5, 2e-5), rtol and atol        (kernel_cases.case_attention)
    16-bit forms, BF16_QS    2e-2 rtol and atol in the bf16 build, an eighth of it in the half build   (kernel_cases.case_attention, fwd_tol)
    x3 forms (and A3 rows)   1e-4 of the clip's output scale                                       (kernel_cases.case_x3: "split-bf16 attention forward")

Forms: every kernel instantiation the flag can reach, by the switches that select them (attention.hip attn_fwd_launch)."""
import numpy as np
import torch

from maest_amd import _lib, ops
from tests import guard as G
from tests.kernel_cases import _attn_ref, close, f16_build, f32, lp, rnd, t16, tol

E = 768
SCALE = 0.125
LOG2E = 1.4426950408889634
# name -> (16-bit operands, x3, q_prescaled, out_split3, options of the flagged call, options of the unflagged call it is compared with)
FORMS = {
    "f32": (False, False, False, False, {}, {}),                                 # attn_fwd_kernel<float>
    "x3": (False, True, False, False, {}, {}),                                   # attn_fwd_x3s_kernel (q_rows = N), attn_fwd_kernel<float, true> (head rows)
    "x3r": (False, True, False, False, dict(attn_fwd=1), dict(attn_fwd=1)),      # attn_fwd_kernel<float, true> at every q_rows: the per-use split
    "a3": (False, True, False, True, {}, {}),                                    # the MAEST_SPLIT3_A output of the split-tile kernel
    "a3r": (False, True, False, True, dict(attn_fwd=1), dict(attn_fwd=1)),       # ... and of the per-use split kernel
    # the flagged call runs on the DEFAULT switches: it must take the LDS-DMA kernel at every N (the unflagged default above 320 tokens is the
    # persistent kernel, another arithmetic): compared with the unflagged call forced onto the LDS-DMA kernel
    "16": (True, False, False, False, {}, dict(attn_fwd=2)),
    "16r": (True, False, False, False, dict(attn_fwd=1), dict(attn_fwd=1)),      # attn_fwd_kernel<16-bit>: register-staged tiles
    "qs": (True, False, True, False, {}, dict(attn_fwd=2)),                      # MAEST_BF16_QS on the LDS-DMA kernel
    "16w8": (True, False, False, False, dict(attn_fwd_waves=8), dict(attn_fwd=2, attn_fwd_waves=8)),     # 256-query workgroups (the device)
}
FORMS_EMU = ("f32", "x3", "x3r", "a3", "16", "16r", "qs")
FORMS_16 = ("16", "16r", "qs", "16w8")

EMU_SHAPES = [(5, 75, (1, 32, 33, 64, 75)), (2, 40, (3, 40))]
GPU_SHAPES = [(12, 161, (1, 3, 31, 32, 33, 64, 65, 96, 127, 128, 129, 161)), (5, 330, (3, 128, 129, 257, 330))]


def operands(form, B, N, counts=None, seed=70):
    """-> the qkv tensor the kernels read ([B * N, 2304]); counts: rows >= counts[b] of clip b filled with NaN."""
    sixteen, _, qs, _, _, _ = FORMS[form]
    x = rnd((B * N, 3 * E), seed)
    if counts is not None:
        x = x.reshape(B, N, 3 * E).clone()
        for b, n in enumerate(counts):
            x[b, n:] = float("nan")
        x = x.reshape(B * N, 3 * E)
    if not sixteen:
        return x.contiguous()
    qkv = lp(x)
    if qs:      # what the row-scaled qkv projection writes: q' = scale * log2(e) * q, rounded once
        qp = lp(f32(qkv[:, :E]) * float(np.float32(SCALE) * np.float32(LOG2E)))
        qkv = torch.cat([qp, qkv[:, E:]], 1).contiguous()
    return qkv


def values(form, qkv):
    """The fp64 values the reference attends over: the operands as stored, q' of MAEST_BF16_QS taken back to q."""
    x = f32(qkv).double()
    if FORMS[form][2]:
        x = torch.cat([x[:, :E] / (SCALE * LOG2E), x[:, E:]], 1)
    return x


def run(dev, form, qkv, B, N, q_rows, n_tok=None):
    """One call; n_tok: a list of counts (flagged, on the flagged call's switches) or None (unflagged, on the comparison's).
    -> (out on the CPU, the n_tok tensor the kernel was handed, read back)."""
    _, x3, qs, a3, opt_f, opt_u = FORMS[form]
    nt = None if n_tok is None else torch.tensor(list(n_tok), dtype=torch.int32).to(dev)
    with ops.options(**(opt_u if n_tok is None else opt_f)):
        out = ops.attn_fwd(qkv.to(dev), B, N, SCALE, q_rows=q_rows, x3=x3, q_prescaled=qs, out_split3=a3 and q_rows == N, n_tok=nt)
    return out.cpu(), (None if nt is None else nt.cpu())


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(what, got, want):
    d = bits(got) != bits(want)
    assert not bool(d.any()), f"{what}: {int(d.sum())}/{d.numel()} elements differ; first at {tuple(int(i) for i in d.nonzero()[0])}"


def written_rows(N, q_rows):
    """Rows of every clip the unflagged call writes: all of them, or the 32-row tiles that hold the first q_rows."""
    return N if q_rows >= N else min(N, -(-q_rows // 32) * 32)


def gate64(form, what, got, qkv_clip, n, rows):
    """Clip rows [0, rows) of `got` against the fp64 softmax attention over the clip's n stored rows, at the form's existing tolerance."""
    sixteen, x3, _, a3, _, _ = FORMS[form]
    ref = _attn_ref(values(form, qkv_clip), 1, n, SCALE)[0][:rows]
    if a3 and got.shape[1] == 3 * E:      # MAEST_SPLIT3_A rows: hi | hi | lo
        same_bits(f"{what}: the two hi thirds", got[:, :E], got[:, E:2 * E])
        got = f32(got[:, :E]).double() + f32(got[:, 2 * E:]).double()
    if x3:
        e = float((got.double() - ref).abs().max() / ref.abs().max())
        print(f"  {what}: {e:.2e} of the output scale (gate 1e-4)")
        assert e < 1e-4, f"{what}: {e:.2e} of the output scale"
    elif sixteen:
        t = t16(2e-2, 2e-2 / 8)
        close(got, ref.float(), t, t, what)
    else:
        close(got, ref.float(), *tol(torch.float32), what)


def case_lens(dev, form, B, N, counts, q_rows=None, full_B=None):
    """Checks 1 - 5 of one form at one shape (module docstring; q_rows < N wants an active guard: the pre-fill pattern of the unwritten rows).
    full_B (the emulator, whose time goes with the active work-items): the full-count comparison runs on the first full_B clips only."""
    q_rows = N if q_rows is None else q_rows
    counts = list(counts)
    assert len(counts) == B and all(1 <= n <= N for n in counts)
    W = written_rows(N, q_rows)
    print(f"token counts, {'f16' if f16_build() else 'bf16'} build, form {form}, B = {B}, N = {N}, q_rows = {q_rows}, counts {counts}")
    qkv = operands(form, B, N)
    out, nt = run(dev, form, qkv, B, N, q_rows, counts)
    ld = out.shape[1]
    o3 = out.reshape(B, N, ld)
    # 4. written rows: zeros behind the clip's tokens, the pre-fill pattern where the unflagged call writes nothing, n_tok as it was
    assert nt.tolist() == counts, f"n_tok was modified: {nt.tolist()}"
    for b, n in enumerate(counts):
        z = bits(o3[b, n:W])
        assert not bool((z != 0).any()), f"clip {b} (n = {n}): {int((z != 0).sum())} non-zero words in the written rows [{n}, {W})"
    if W < N:
        assert G.guarded._active is not None, "q_rows < N: run this case under guard.guarded() (the pre-fill pattern)"
        assert bool(G.untouched(o3[:, W:]).all()), f"rows >= {W} were written"
    # 2. every clip against the unflagged call on the clip alone (bit for bit), and against the fp64 softmax over its own keys
    for b, n in enumerate(counts):
        rows = min(n, W)
        clip = qkv[b * N:b * N + n].contiguous()
        # (head rows of the x3 form run on the per-use split kernel; alone, a clip of n <= q_rows tokens is a complete pass, which the
        # dispatch hands to the split-tile kernel -- another order inside a chunk step: keep the clip alone on the flagged call's kernel)
        alone_form = "x3r" if form == "x3" and q_rows < N and n <= q_rows else form
        alone, _ = run(dev, alone_form, clip, 1, n, min(q_rows, n))
        same_bits(f"clip {b} (n = {n}) against the unflagged call on the clip alone", o3[b, :rows], alone[:rows, :ld])
        gate64(form, f"clip {b} (n = {n}) against the fp64 softmax over its {n} keys", o3[b, :rows], clip, n, rows)
    # 3. padding is never read: NaN behind every clip's tokens, the same bits
    out_nan, _ = run(dev, form, operands(form, B, N, counts), B, N, q_rows, counts)
    same_bits("NaN in the padded rows of qkv", out_nan.reshape(B, N, ld)[:, :W], o3[:, :W])
    # 5. two calls
    out_2, _ = run(dev, form, qkv, B, N, q_rows, counts)
    same_bits("two calls", out_2.reshape(B, N, ld)[:, :W], o3[:, :W])
    # 1. full counts change nothing
    Bf = B if full_B is None else full_B
    qf = qkv[:Bf * N].contiguous()
    full, _ = run(dev, form, qf, Bf, N, q_rows, [N] * Bf)
    plain, _ = run(dev, form, qf, Bf, N, q_rows)
    same_bits("n_tok = N against the unflagged call", full.reshape(Bf, N, ld)[:, :W], plain.reshape(Bf, N, ld)[:, :W])


def case_argument_errors(dev):
    """Every refusal returns MAEST_ERR_INVALID (status 1) with its message in maest_last_error(); the accepted codes run."""
    import pytest
    B, N = 2, 8
    qkv = rnd((B * N, 3 * E), 3).to(dev)
    qkv16 = lp(rnd((B * N, 3 * E), 3)).to(dev)
    out = torch.zeros(B * N * 3 * E, dtype=torch.float32, device=dev)
    nt = torch.tensor([3, 8], dtype=torch.int32).to(dev)
    L, P, PM = _lib.ATTN_LENS, _lib.ATTN_PROBS, _lib.ATTN_PROBS_MEAN
    st = ops._s(qkv)

    def refused(match, entry="maest_attn_fwd_rows", q=qkv, o=out, l=nt, code=_lib.F32 | L, q_rows=N):
        with pytest.raises(_lib.MaestHipError, match=match) as e:
            if entry == "maest_attn_fwd_rows":
                _lib.call(entry, ops._p(q), ops._p(o), ops._p(l), B, N, code, SCALE, q_rows, st)
            else:
                _lib.call(entry, ops._p(q), ops._p(o), ops._p(o), ops._p(o), ops._p(o), ops._p(o), B, N, code, SCALE, q_rows, st)
        assert "status 1" in str(e.value)

    refused("MAEST_ATTN_LENS reads the token counts", l=None)
    refused("MAEST_ATTN_LENS reads the token counts", l=None, q=qkv16, code=_lib.BF16 | L)
    refused("MAEST_ATTN_LENS with MAEST_ATTN_PROBS", code=_lib.F32 | L | P)
    refused("MAEST_ATTN_LENS with MAEST_ATTN_PROBS", code=_lib.F32 | L | P | PM, l=None)
    refused("bad dtype", code=_lib.F16 | L)
    refused("bad dtype", code=_lib.SPLIT3_A | L)
    refused("q_rows", q_rows=N + 1)
    refused("alignment", o=out[1:])
    refused("bad dtype", entry="maest_attn_bwd_rows")      # the backward does not know the flag: a bit no dtype code has
    for code, q in ((_lib.F32, qkv), (_lib.F32X3, qkv), (_lib.F32X3_A3, qkv), (_lib.BF16, qkv16), (_lib.BF16_QS, qkv16)):
        _lib.call("maest_attn_fwd_rows", ops._p(q), ops._p(out), ops._p(nt), B, N, code | L, SCALE, N, st)
    assert nt.cpu().tolist() == [3, 8]
