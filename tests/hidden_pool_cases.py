"""The grid pools of the hidden states (MAEST_GATHER_POOLS on maest_gather_head_rows: ops.grid_pools, csrc/misc.hip gather_pools_kernel)
against two conditions, neither of them measured; run by test_emu_hidden_pool.py under the emulator and by test_hidden_pool_gpu.py on the
device, in both builds (the operands are fp32 in both).

EQUALITY (include/maest_hip.h).  Every output element is defined operation by operation -- a sum that starts at 0.0f, fp32 adds in
ascending row order, one IEEE division --, so the kernel must equal `reference`, an explicit ascending fp32 loop (never a library sum,
which may add pairwise), with torch.equal.  The inputs make the order visible: magnitudes spread over +-8 binary orders, and `operand`
asserts, on the CPU and for these very inputs, that a descending and a pairwise sum each differ from the ascending one in at least one
element of every pool that has enough terms for the order to exist (descending: 3 terms -- two terms commute --, pairwise: 4).  That is a
condition on the inputs, not on the kernel.

THE BOUND.  Every pool lies within

    (gamma_n + u) * mean|x|,      gamma_n = n u / (1 - n u),  u = 2^-24,  n the number of terms,  mean|x| the fp64 mean of their magnitudes,

of the fp64 mean: n adds (the first of them, 0.0f + x, exact) and one division.  It refuses what equality with a wrong reference could not:
a pool over the wrong rows, a wrong divisor.

`pipeline` is the same definition evaluated independently -- every add and the division made in fp64 on two fp32 values and rounded to fp32,
which is the correctly rounded fp32 operation (53 >= 2 * 24 + 2 bits: the double rounding is innocuous for +, /) -- with one of the defects the
conditions must refuse; test_emu_hidden_pool.py shows, without any kernel, that the sound pipeline passes both and each defect fails one."""
import functools

import numpy as np
import torch

from maest_amd import _lib, ops
from tests import guard
from tests.kernel_cases import f16_build

H, E = 2, 768
U = 2.0 ** -24
SHAPES = [(1, 1, 1), (2, 9, 1), (2, 1, 7), (3, 4, 13), (2, 9, 25)]      # (clips, Fk, Tk): the minimum, one column, one row, odd sizes, the model test's N = 227
SHAPES_GPU = [(2, 9, 62), (1, 9, 187)]                                   # N = 560 and 1685: the 10 s and the 30 s token counts (the device only)
POOL_NAMES = ("mean", "freq", "time")


def gamma(n):
    return n * U / (1.0 - n * U)


def _terms(x, Fk, Tk):
    """The rows each pool sums, in the order of the definition: {pool: fp32 [clips, outputs, terms, 768]}."""
    clips = x.shape[0]
    g = x[:, H:].reshape(clips, Fk, Tk, E)
    return {"mean": x[:, H:].reshape(clips, 1, Fk * Tk, E), "freq": g, "time": g.transpose(1, 2)}


def _ascending(t):
    s = torch.zeros(t.shape[:2] + (E,), dtype=torch.float32)
    for i in range(t.shape[2]):
        s = s + t[:, :, i]
    return s


def _descending(t):
    s = torch.zeros(t.shape[:2] + (E,), dtype=torch.float32)
    for i in range(t.shape[2] - 1, -1, -1):
        s = s + t[:, :, i]
    return s


def _pairwise(t):
    n = t.shape[2]
    if n == 1:
        return 0.0 + t[:, :, 0]
    return _pairwise(t[:, :, :n // 2]) + _pairwise(t[:, :, n // 2:])


@functools.lru_cache(maxsize=None)
def operand(clips, Fk, Tk):
    """fp32 [clips, 2 + Fk * Tk, 768], magnitudes spread over about +-8 binary orders; shared, never modified.  Asserts the condition on
    the inputs of the module docstring."""
    rng = np.random.Generator(np.random.PCG64(1000 * clips + 100 * Fk + Tk))
    shape = (clips, H + Fk * Tk, E)
    x = torch.from_numpy((rng.standard_normal(shape) * np.exp2(rng.uniform(-8.0, 8.0, shape))).astype(np.float32))
    for name, t in _terms(x, Fk, Tk).items():
        n, asc = t.shape[2], _ascending(t)
        if n >= 3:
            assert not torch.equal(_descending(t), asc), f"{(clips, Fk, Tk)}: a descending sum has the bits of the ascending one in pool {name}"
        if n >= 4:
            assert not torch.equal(_pairwise(t), asc), f"{(clips, Fk, Tk)}: a pairwise sum has the bits of the ascending one in pool {name}"
    return x


def reference(x, Fk, Tk):
    """The definition as an explicit loop -> {"head", "mean", "freq", "time"}, fp32."""
    out = {"head": x[:, :H].clone()}
    for name, t in _terms(x, Fk, Tk).items():
        out[name] = _ascending(t) / float(t.shape[2])
    out["mean"] = out["mean"][:, 0]
    return out


@functools.lru_cache(maxsize=None)
def reference_of(clips, Fk, Tk):
    """(reference, {pool: (fp64 mean, limit)}) of a case's operand: computed once, shared, never modified."""
    x = operand(clips, Fk, Tk)
    lims = {}
    for name, t in _terms(x, Fk, Tk).items():
        n, d = t.shape[2], t.double()
        m, lim = d.mean(2), (gamma(n) + U) * d.abs().mean(2)
        lims[name] = (m[:, 0], lim[:, 0]) if name == "mean" else (m, lim)
    return reference(x, Fk, Tk), lims


def equal(what, got, ref):
    """EQUALITY of the module docstring on the four parts."""
    for name in ("head",) + POOL_NAMES:
        g, r = got[name].detach().cpu(), ref[name]
        assert g.dtype == torch.float32 and g.shape == r.shape, (what, name, g.dtype, tuple(g.shape), tuple(r.shape))
        bad = g.contiguous().view(torch.int32) != r.contiguous().view(torch.int32)
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the ascending fp32 loop in {name!r}; first at "
                                     f"{tuple(int(i) for i in bad.nonzero()[0])}")


def gate(what, got, lims):
    """THE BOUND of the module docstring on the three pools; prints and returns the worst share of the limit used."""
    worst = 0.0
    for name in POOL_NAMES:
        m, lim = lims[name]
        g = got[name].detach().cpu().double()
        assert g.shape == m.shape, (what, name, tuple(g.shape), tuple(m.shape))
        assert bool(torch.isfinite(g).all()), f"{what}: non-finite results in {name!r} (elements never written?)"
        err = (g - m).abs()
        ratio = float((err / lim.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        bad = err > lim
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} elements of {name!r} outside the bound, worst {ratio:.3g} x; first "
                                     f"at {tuple(int(i) for i in bad.nonzero()[0])}")
    print(f"  {what}: worst |pool - fp64 mean| / limit = {worst:.3g}")
    return worst


def _parts(r):
    return dict(zip(("head", "mean", "freq", "time"), r))


def run(dev, clips, Fk, Tk):
    return _parts(ops.grid_pools(operand(clips, Fk, Tk).to(dev), Tk, H))


def _say(what, clips, Fk, Tk):
    print(f"grid pools, {what}, {'f16' if f16_build() else 'bf16'} build, clips = {clips}, Fk = {Fk}, Tk = {Tk}, N = {H + Fk * Tk}")


def case_exact(dev, clips, Fk, Tk):
    """Equality with the loop, the bound, and rows 0 .. 2 against ops.embed_pool of the same tensor."""
    _say("equality, bound and the embed_pool identity", clips, Fk, Tk)
    got = run(dev, clips, Fk, Tk)
    ref, lims = reference_of(clips, Fk, Tk)
    assert got["freq"].shape == (clips, Fk, E) and got["time"].shape == (clips, Tk, E)
    equal("the kernel", got, ref)
    gate("the kernel", got, lims)
    emb = ops.embed_pool(operand(clips, Fk, Tk).to(dev)).cpu()
    rows = torch.cat([got["head"].cpu().reshape(clips, H * E), got["mean"].cpu()], dim=1)
    assert torch.equal(rows.view(torch.int32), emb.view(torch.int32)), "rows 0 .. 2 differ from maest_embed_pool's output"
    if (Fk, Tk) == (1, 1):      # the minimum: every pool is the one patch row (0.0f + x, / 1.0f)
        x = operand(clips, Fk, Tk)
        for name in POOL_NAMES:
            assert torch.equal(got[name].cpu().reshape(clips, E), 0.0 + x[:, H])


def case_repeat(dev, clips, Fk, Tk):
    a, b = run(dev, clips, Fk, Tk), run(dev, clips, Fk, Tk)
    for name in a:
        assert torch.equal(a[name].cpu().view(torch.int32), b[name].cpu().view(torch.int32)), f"two launches differ in {name!r}"


def case_regions(dev, clips, Fk, Tk):
    """Inside a guard (the caller's guard.covering): dst, allocated by the wrapper and filled with the guard's pattern, is written in
    exactly [clips, 3 + Fk + Tk, 768] -- every element, nothing in the bands --, and src is bitwise unchanged (the guard checks the arena
    of a const argument)."""
    assert guard.guarded._active is not None
    x = operand(clips, Fk, Tk).to(dev)
    parts = ops.grid_pools(x, Tk, H)
    whole = parts[0]._base
    assert whole.shape == (clips, H + 1 + Fk + Tk, E) and whole.is_contiguous()
    assert not bool(guard.untouched(whole).any()), "elements of dst were never written"
    equal("the kernel (guarded)", _parts(parts), reference_of(clips, Fk, Tk)[0])
    assert torch.equal(x.cpu().view(torch.int32), operand(clips, Fk, Tk).view(torch.int32))


def case_argument_errors(dev):
    """The refusals of the form: MAEST_ERR_INVALID (status 1) with its message in maest_last_error(); and the entry point without the
    flag as it was."""
    import pytest
    clips, Fk, Tk = 1, 2, 3
    n_tok = H + Fk * Tk
    x = operand(1, 9, 1)[:, :n_tok].contiguous().to(dev)
    x16 = x.bfloat16()
    dst = torch.zeros(clips * (H + 1 + 1 + Fk * Tk) * E + 4, dtype=torch.float32, device=dev)      # (room for every grid of the P = 6 rows)
    G, T = _lib.GATHER_POOLS, _lib.gather_pools_t
    st = ops._s(x)

    def call(src=x, n_tok_=n_tok, n_head=H, code=_lib.F32 | G | T(Tk), d=dst):
        _lib.call("maest_gather_head_rows", ops._p(src), clips, n_tok_, n_head, code, ops._p(d), st)

    def refused(match, **kw):
        with pytest.raises(_lib.MaestHipError, match=match) as e:
            call(**kw)
        assert "status 1" in str(e.value)

    refused("base code must be MAEST_F32", src=x16, code=_lib.BF16 | G | T(Tk))      # a 16-bit base code beside the flag
    refused("base code must be MAEST_F32", code=_lib.F32X3 | G | T(Tk))
    refused("Tk = 0", code=_lib.F32 | G)
    refused("no Fk x Tk grid", code=_lib.F32 | G | T(4))                             # P = 6
    refused("no Fk x Tk grid", code=_lib.F32 | G | T(7))                             # Tk > P
    refused("patch rows behind the head rows", n_tok_=H)                             # n_tok == n_head
    refused("unknown flag bits", code=_lib.F32 | G | 0x200 | T(Tk))
    refused("unknown flag bits", code=_lib.F32 | G | 0x8000 | T(Tk))
    refused("alignment", d=dst[1:])
    refused("null pointer", d=None)
    refused("bad dtype", code=_lib.F32 | T(Tk))                                      # the Tk bits without the flag: the entry point as it was
    refused("bad dtype", code=_lib.F32 | 0x200)
    call()
    call(code=_lib.F32 | G | T(1))
    call(code=_lib.F32 | G | T(6))
    # without the flag: the head rows, fp32 and 16-bit, as ever
    assert torch.equal(ops.gather_head_rows(x.reshape(n_tok, E), clips, n_tok, H).cpu(), x.cpu()[0, :H])
    assert torch.equal(ops.gather_head_rows(x16.reshape(n_tok, E), clips, n_tok, H).cpu(), x16.cpu()[0, :H])


# ---------------------------------------------------------------------------------------------- doctored pipelines (tests of the conditions)
DEFECTS = ("time and freq swapped", "cls / dist in the mean", "divided by n_tok", "descending order")


def _round32(d):
    return d.float().double()


def _sum64(t, descending=False):
    """The fp32 chain made in fp64: s <- fp32(s + x), every step (the module docstring) -> fp64 tensor of fp32 values."""
    s = torch.zeros(t.shape[:2] + (E,), dtype=torch.float64)
    order = range(t.shape[2] - 1, -1, -1) if descending else range(t.shape[2])
    for i in order:
        s = _round32(s + t[:, :, i].double())
    return s


def pipeline(x, Fk, Tk, defect=None):
    """The form's definition evaluated step by step in fp64 with a rounding to fp32 behind every operation -> the four parts, fp32; with one
    of the defects the conditions must refuse:
       "time and freq swapped"    the patch rows read as a Tk x Fk grid in time-major order              (the bound)
       "cls / dist in the mean"   the mean row sums all n_tok rows                                      (the bound)
       "divided by n_tok"         the mean row divides by n_tok instead of P                            (the bound)
       "descending order"         every sum runs from its last term to its first                        (equality)"""
    clips, n_tok = x.shape[0], x.shape[1]
    terms = _terms(x, Fk, Tk)
    if defect == "time and freq swapped":
        g = x[:, H:].reshape(clips, Tk, Fk, E)
        terms["freq"], terms["time"] = g.transpose(1, 2), g
    if defect == "cls / dist in the mean":
        terms["mean"] = x.reshape(clips, 1, n_tok, E)
    out = {"head": x[:, :H].clone()}
    for name, t in terms.items():
        n = n_tok if (defect == "divided by n_tok" and name == "mean") else (Fk * Tk if name == "mean" else t.shape[2])
        out[name] = (_sum64(t, descending=defect == "descending order") / float(n)).float()
    out["mean"] = out["mean"][:, 0]
    return out
