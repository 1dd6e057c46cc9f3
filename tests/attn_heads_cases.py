"""Per-head attention pooling (MAEST_ATTN_APPLY_HEADS on MAEST_ATTN_APPLY, with and without MAEST_ATTN_APPLY_GRAD: ops.attn_apply_heads,
ops.attn_relevance_heads) against two conditions, neither of them measured (a sibling of attn_apply_cases and attn_relevance_cases: their
operands, their weights, their dO, their fp64 references, the same two builds; run by test_emu_attn_heads.py under the emulator and by
test_attn_heads_gpu.py on the device).

THE IDENTITY (include/maest_hip.h).  Y [B, 12, R, N] of the flagged call and Z [B, R, N] of the same call without the flag satisfy

    fp32(1 / 12) * (((Y[:, 0] + Y[:, 1]) + Y[:, 2]) + ... + Y[:, 11]) == Z          bit for bit  (ops.heads_mean: eleven fp32 adds, one product)

because per head both kernels run the same arithmetic in the same order and IEEE adds and products are correctly rounded wherever they are
made.  There is no tolerance: a head in another slot than its own (other than 0 <-> 1: one commutative add), another order of the queries,
a contracted or split operation, a scale applied early -- each changes bits.

THE BOUND.  The fp64 reference keeps the heads apart,

    Y_ref[b, h, r, k] = sum_{q < q_rows} W[b, r, q] a_ref_h[q, k],      a_ref = p_ref  (plain),   max(p_ref g_ref, 0)  (GRAD)

with p_ref, E' (the relative error of the kernel's probability: scores, the lse2 route, v_exp, the N-term sum) taken from
attn_apply_cases.reference and, under GRAD, g_ref, dg from the operands as attn_relevance_cases.reference forms them.  The limit is the
per-head term of the siblings' gates -- without their division by twelve, which belongs to the mean -- with the rounding count of ONE head:
per element a chain of fmas over the queries of one half-wave (at most q_rows of them carry a non-zero weight; the rows staged for queries >=
q_rows add exact zeros) and the half-wave add, so fewer than q_rows + 1 roundings of non-negative terms where the mean form has q_rows + 14
(its eleven head adds, the product with fp32(1 / 12) and that constant's own rounding are not made here).  Under GRAD the product p g costs
one more u, as in the sibling: gamma_{q_rows + 2} where it has gamma_{q_rows + 15}.

    plain:  |Y - Y_ref| <= sum_q |W| p_ref (E' + gamma_{q_rows + 1}) + 2^-100 sum_q |W|
    GRAD:   |Y - Y_ref| <= sum_q |W| p_ref (|g| (E' + gamma_{q_rows + 2}) + (1 + E') dg) + 2^-100 sum_q |W| max |g|        for every element

(the floors: probabilities below 2^-126 are flushed by v_exp_f32, as in the siblings; max |g| per clip).  Nothing here is looser than the
siblings' constants: E', dg, u_prod and the floors are theirs, the gamma index is smaller.

test_attn_heads_gates_pass_the_sound_pipeline / _reject_defects (test_emu_attn_heads.py) show, without any kernel, what the two conditions
pass and what they refuse: two heads in each other's slots, one head scaled by 1 / 12, a head sum taken in descending order."""
import functools

import torch

from maest_amd import _lib, ops
from tests import attn_apply_cases as AC
from tests import attn_probs_cases as PC
from tests import attn_relevance_cases as RC
from tests import guard
from tests.kernel_cases import f16_build, lp, rnd

H, HD, E = PC.H, PC.HD, PC.E
U, LN2, FLOOR, SCALE = PC.U, PC.LN2, PC.FLOOR, PC.SCALE
CODES = PC.CODES
SHAPES = AC.SHAPES            # (B, N, q_rows, R): the smallest shapes at which the kernel can go wrong (attn_apply_cases)
SHAPE_GPU = AC.SHAPE_GPU      # three key blocks, the eight-row kernel (the device only)
weights = AC.weights
_bits_equal = AC._bits_equal
BASE = {"f32": _lib.F32, "x3": _lib.F32X3, "16": _lib.BF16, "qs": _lib.BF16_QS}


def reference(xs, ds, w, B, N, q_rows, c2, u_prod, shared):
    """fp64 -> (Y_ref [B, 12, R, N], its limit [B, 12, R, N]): the module docstring.  ds: dO as stored (GRAD), None: the plain form.
    shared: attn_apply_cases.reference(...) of the same case (its p_ref and E' are read, nothing is recomputed or modified)."""
    p_ref, e_apply = shared[4], shared[6]
    wd = w[:, :, :q_rows].double()
    wa = wd.abs()
    if ds is None:
        a_ref = p_ref
        term = p_ref * (e_apply + PC.gamma(q_rows + 1))
        floor = FLOOR * wa.sum(-1).reshape(B, 1, -1, 1)
    else:
        _, _, v = PC._heads(xs, B, N)
        do = RC._dheads(ds, B, N)[:, :, :q_rows]
        g = do @ v.transpose(-2, -1)                                               # [B, 12, q_rows, N]
        dg = (do.abs() @ v.abs().transpose(-2, -1)) * (PC.gamma(66) + u_prod)
        a_ref = (p_ref * g).clamp_min(0)
        term = p_ref * (g.abs() * (e_apply + PC.gamma(q_rows + 2)) + (1 + e_apply) * dg)
        floor = FLOOR * wa.sum(-1).reshape(B, 1, -1, 1) * g.abs().amax((1, 2, 3)).reshape(B, 1, 1, 1)
    y_ref = torch.einsum("brq,bhqk->bhrk", wd, a_ref)
    lim = torch.einsum("brq,bhqk->bhrk", wa, term) + floor
    return y_ref, lim


@functools.lru_cache(maxsize=None)
def _reference_of(B, N, q_rows, R, code, grad, seed, spike, times, f16):
    _, xs = PC._operands(B, N, code, seed, spike, times, f16)
    ds = RC._dout(B, N, code, 52, f16)[1] if grad else None
    shared = AC._reference_of(B, N, q_rows, R, code, seed, spike, times, f16)
    return reference(xs, ds, weights(B, R, N, q_rows), B, N, q_rows, PC.c2_of(code), PC.U_PROD[code], shared)


def reference_of(B, N, q_rows, R, code, grad, seed=30, spike=False, times=1.0):
    """The per-head reference of the siblings' operands, dO and weights (computed once per case and build, shared, never modified)."""
    return _reference_of(B, N, q_rows, R, code, grad, seed, spike, times, f16_build() and code in ("16", "qs"))


def gate(what, y, ref):
    """The bound of the module docstring on y [B, 12, R, N]; prints and returns the worst share of the limit used."""
    y_ref, lim = ref
    y = y.detach().cpu().double()
    assert y.shape == y_ref.shape, (what, tuple(y.shape), tuple(y_ref.shape))
    assert bool(torch.isfinite(y).all()), f"{what}: {int((~torch.isfinite(y)).sum())} non-finite results (elements never written?)"
    err = (y - y_ref).abs()
    ratio = float((err / lim.clamp_min(1e-300)).max())
    print(f"  {what}: worst |Y - Y_ref| / limit = {ratio:.3g} over the twelve heads (relative limit "
          f"{float((lim / y_ref.clamp_min(1e-300)).min()):.1e} and up)")
    bad = err > lim
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the bound, worst {ratio:.3g} x; first at "
                                 f"(clip, head, row, key) = {tuple(int(i) for i in bad.nonzero()[0])}")
    return ratio


def identity(what, y, mean):
    """The identity of the module docstring: heads_mean(y) has the bits of the mean form's result."""
    assert y.dtype == torch.float32 and mean.dtype == torch.float32
    _bits_equal(what, ops.heads_mean(y).cpu(), mean.cpu())


def run(dev, B, N, q_rows, R, code, grad, w=None, variant=None, **kw):
    """The per-head call of a case -> fp32 [B, 12, R, N] on `dev`."""
    qkv, _ = PC.operands(B, N, code, **kw)
    w = weights(B, R, N, q_rows) if w is None else w
    if not grad:
        assert variant is None
        return ops.attn_apply_heads(qkv.to(dev), w.to(dev), B, N, SCALE, q_rows=q_rows, x3=code == "x3", q_prescaled=code == "qs")
    d, _ = RC.dout(B, N, q_rows, code, variant=variant)
    return ops.attn_relevance_heads(qkv.to(dev), d.to(dev), w.to(dev), B, N, SCALE, q_rows=q_rows, x3=code == "x3", q_prescaled=code == "qs")


@functools.lru_cache(maxsize=None)
def _run_once(dev, B, N, q_rows, R, code, grad, f16, kw):
    return run(dev, B, N, q_rows, R, code, grad, **dict(kw)).cpu()


def run_shared(dev, B, N, q_rows, R, code, grad, **kw):
    """run(...) on the plain weights, made once per case and build and shared by the identity and the bound (never modified; the repeat
    and the tail cases make their own calls)."""
    return _run_once(str(dev), B, N, q_rows, R, code, grad, f16_build(), tuple(sorted(kw.items())))


def run_mean(dev, B, N, q_rows, R, code, grad, **kw):
    """The same call without the flag (the siblings' run) -> fp32 [B, R, N]."""
    return (RC.run if grad else AC.run)(dev, B, N, q_rows, R, code, **kw)


def _say(what, B, N, q_rows, R, code, grad, kw=None):
    print(f"attention heads, {what}, {'GRAD' if grad else 'plain'}, {'f16' if f16_build() else 'bf16'} build, code {code}, B = {B}, N = {N}, "
          f"q_rows = {q_rows}, R = {R}, {kw or 'plain operands'}")


def case_identity(dev, B, N, q_rows, R, code, grad, **kw):
    """heads_mean of the per-head result is the mean form's result, bit for bit."""
    _say("identity", B, N, q_rows, R, code, grad, kw)
    y = run_shared(dev, B, N, q_rows, R, code, grad, **kw)
    assert y.dtype == torch.float32 and y.shape == (B, H, R, N)
    identity("heads_mean(Y of the per-head form) against the mean form", y, run_mean(dev, B, N, q_rows, R, code, grad, **kw))


def case_bound(dev, B, N, q_rows, R, code, grad, **kw):
    """Every head against its fp64 reference.  Returns the share of the limit used."""
    _say("bound", B, N, q_rows, R, code, grad, kw)
    y = run_shared(dev, B, N, q_rows, R, code, grad, **kw)
    assert y.dtype == torch.float32 and y.shape == (B, H, R, N)
    return gate("Y", y, reference_of(B, N, q_rows, R, code, grad, **kw))


def case_repeat(dev, B, N, q_rows, R, code, grad):
    a, b = run(dev, B, N, q_rows, R, code, grad).cpu(), run(dev, B, N, q_rows, R, code, grad).cpu()
    _bits_equal("two calls", a, b)


def case_tails(dev, B, N, q_rows, R, code, grad):
    """Columns >= q_rows of W and, under GRAD, rows >= q_rows of dO hold NaN: Y is finite and bit-identical to the result without them."""
    assert q_rows < N
    y = run(dev, B, N, q_rows, R, code, grad).cpu()
    yn = run(dev, B, N, q_rows, R, code, grad, w=weights(B, R, N, q_rows, nan_tail=True), variant="nan" if grad else None).cpu()
    assert bool(torch.isfinite(yn).all()), "NaN in the columns of W / the rows of dO >= q_rows reached Y"
    _bits_equal("Y with NaN past q_rows", yn, y)


def run_raw(dev, B, N, q_rows, R, code, grad):
    """The flagged call with its workspace in hand -> (Y, workspace), both allocated filled with the guard's pattern, through the names the
    guard replaces when one is active; W and dO carry NaN past q_rows."""
    qkv, _ = PC.operands(B, N, code)
    qkv, w = qkv.to(dev), weights(B, R, N, q_rows, nan_tail=q_rows < N).to(dev)
    d = RC.dout(B, N, q_rows, code, variant="nan" if q_rows < N else None)[0].to(dev) if grad else None
    ops._chk(qkv, d, w)
    y = guard.fill_pattern_(ops.torch.empty((B, H, R, N), dtype=torch.float32, device=dev))
    work = guard.fill_pattern_(ops.torch.empty((B, H, N), dtype=torch.float32, device=dev))
    flags = _lib.ATTN_APPLY | _lib.ATTN_APPLY_HEADS | (_lib.ATTN_APPLY_GRAD if grad else 0) | _lib.attn_apply_rows(R)
    ops.call("maest_attn_bwd_rows", ops._p(qkv), ops._p(d), ops._p(w), None, ops._p(work), ops._p(y), B, N, BASE[code] | flags, SCALE, q_rows,
             ops._s(qkv))
    return y, work


def case_regions(dev, B, N, q_rows, R, code, grad):
    """Y has exactly [B, 12, R, N] elements, all written (under the guard: a store for a key >= N or into a thirteenth head lands in a
    band); the workspace holds a finite lse2 in rows < q_rows and is untouched past them."""
    y, work = run_raw(dev, B, N, q_rows, R, code, grad)
    assert y.shape == (B, H, R, N) and not bool(guard.untouched(y).any()), "elements of Y were never written"
    gate("Y (raw call)", y.cpu(), reference_of(B, N, q_rows, R, code, grad))
    assert bool(torch.isfinite(work[:, :, :q_rows]).all()), "lse2 of a row < q_rows is missing"
    if q_rows < N:
        assert bool(guard.untouched(work[:, :, q_rows:]).all()), "the workspace was written at rows >= q_rows"


def case_argument_errors(dev):
    """The refusals of the flag: MAEST_ERR_INVALID (status 1) with its message in maest_last_error(); the accepted codes run, plain and
    GRAD, every row count, through both entries (the siblings' case_argument_errors cover the forms without the flag as they were)."""
    import pytest
    B, N, R = 1, 8, 2
    qkv = rnd((B * N, 3 * E), 3).to(dev)
    qkv16 = lp(rnd((B * N, 3 * E), 3)).to(dev)
    do = torch.zeros(B * N * E + 4, dtype=torch.float32, device=dev)
    do16 = lp(torch.zeros(B * N * E + 8)).to(dev)
    w = torch.ones(B * R * N + 4, dtype=torch.float32, device=dev)
    y = torch.zeros(B * H * 8 * N + 4, dtype=torch.float32, device=dev)
    work = torch.zeros(B * H * N + 4, dtype=torch.float32, device=dev)
    A, G, HF, rows = _lib.ATTN_APPLY, _lib.ATTN_APPLY_GRAD, _lib.ATTN_APPLY_HEADS, _lib.attn_apply_rows
    st = ops._s(qkv)

    def call(q=qkv, o=None, w_=w, l=None, d=work, y_=y, code=_lib.F32 | A | HF | rows(R), q_rows=N, entry="maest_attn_bwd_rows"):
        args = [ops._p(q), ops._p(o), ops._p(w_), ops._p(l), ops._p(d), ops._p(y_), B, N, code, SCALE]
        _lib.call(entry, *args, *([q_rows] if entry.endswith("_rows") else []), st)

    def refused(match, **kw):
        with pytest.raises(_lib.MaestHipError, match=match) as e:
            call(**kw)
        assert "status 1" in str(e.value)

    refused("MAEST_ATTN_APPLY_HEADS without MAEST_ATTN_APPLY", code=_lib.F32 | HF, l=work, o=do)             # the flag alone
    refused("MAEST_ATTN_APPLY_HEADS without MAEST_ATTN_APPLY", code=_lib.F32 | HF | rows(R))
    refused("MAEST_ATTN_APPLY_HEADS without MAEST_ATTN_APPLY", code=_lib.F32 | HF | G | rows(R), o=do)
    refused("MAEST_ATTN_APPLY_HEADS with MAEST_ATTN_PROBS", code=_lib.F32 | HF | _lib.ATTN_PROBS)
    refused("MAEST_ATTN_APPLY_HEADS with MAEST_ATTN_PROBS", code=_lib.F32 | A | HF | _lib.ATTN_PROBS | rows(R))
    refused("MAEST_ATTN_APPLY_HEADS with MAEST_ATTN_PROBS", code=_lib.F32 | A | HF | G | _lib.ATTN_PROBS_MEAN | rows(R), o=do)
    refused("MAEST_F32X3_A3", code=_lib.F32X3_A3 | A | HF | rows(R))
    refused("MAEST_F32X3_A3", code=_lib.F32X3_A3 | A | HF | G | rows(R), o=do)
    refused("pass NULL", o=do)                                            # `out` without MAEST_ATTN_APPLY_GRAD
    refused("pass NULL", l=work)
    refused("null pointer", code=_lib.F32 | A | HF | G | rows(R))         # ... and with it `out` is an operand
    refused("bad dtype", code=_lib.SPLIT3_A | A | HF | rows(R))
    refused("bad dtype", code=_lib.F32 | A | HF | 0x2000 | rows(R))       # the next bit up is nobody's
    refused("alignment", y_=y[1:])
    refused("q_rows", q_rows=N + 1)
    refused("outside 1..8", code=_lib.F32 | A | HF | rows(9))
    for code, q, o in ((_lib.F32, qkv, do), (_lib.F32X3, qkv, do), (_lib.BF16, qkv16, do16), (_lib.BF16_QS, qkv16, do16)):
        for r in (1, 4, 8):                                               # (the two-, four- and eight-row kernels)
            call(q=q, code=code | A | HF | rows(r))
            call(q=q, o=o, code=code | A | HF | G | rows(r))
    call(entry="maest_attn_bwd")


# ---------------------------------------------------------------------------------------------- doctored pipelines (tests of the gates)
DEFECTS = ("heads swapped", "one head / 12", "descending head sum")


def pipeline64(xs, ds, w, B, N, q_rows, c2, defect=None):
    """The per-head form in fp64 on the stored operands -> (Y [B, 12, R, N] rounded to fp32, the mean a mean-form kernel would write beside
    it, fp32 [B, R, N]), with one of the defects the conditions must refuse:
       "heads swapped"         heads 3 and 7 written to each other's slots                       (the bound)
       "one head / 12"         head 5 scaled by 1 / 12, as if the mean's factor had been kept    (the bound)
       "descending head sum"   the mean form adds the heads from 11 down to 0                    (the identity)"""
    q, k, v = PC._heads(xs, B, N)
    q = q[:, :, :q_rows]
    t = c2 * (q @ k.transpose(-2, -1))
    m = t.amax(-1, keepdim=True)
    a = torch.exp2(t - (m + torch.log2(torch.exp2(t - m).sum(-1, keepdim=True))))
    if ds is not None:
        a = (a * (RC._dheads(ds, B, N)[:, :, :q_rows] @ v.transpose(-2, -1))).clamp_min(0)
    y = torch.einsum("brq,bhqk->bhrk", w[:, :, :q_rows].double(), a).float()
    order = range(H - 1, -1, -1) if defect == "descending head sum" else range(H)
    tot = None
    for h in order:
        tot = y[:, h] if tot is None else tot + y[:, h]
    mean = tot * ops._TWELFTH
    if defect == "heads swapped":
        y = y[:, [0, 1, 2, 7, 4, 5, 6, 3, 8, 9, 10, 11]].contiguous()
    elif defect == "one head / 12":
        y = y.clone()
        y[:, 5] /= 12
    return y, mean
