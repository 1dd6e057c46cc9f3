"""Gradient-weighted attention pooling (MAEST_ATTN_APPLY | MAEST_ATTN_APPLY_GRAD, ops.attn_relevance: the step of gradient-weighted rollout)
against an error bound that is DERIVED, not measured (a sibling of attn_apply_cases: the same qkv operands, the same weights, the same two
builds; run by test_emu_attn_relevance.py under the emulator and by test_attn_relevance_gpu.py on the device).

The reference is fp64 on the operands as stored:

    Y_ref[b, r, k] = (1 / 12) sum_h sum_{q < q_rows} W[b, r, q] max(p_ref_h[q, k] g_ref_h[q, k], 0),     g_ref_h[q, k] = dO_h[q] . V_h[k]

with p_ref the fp64 softmax of attn_probs_cases.reference.  The kernel's factors:

    g   the dP product of the backward, 64 products summed in fp32 in the mode's arithmetic: off by at most
            dg(q, k) = (|dO| . |V|)[q, k] (gamma_66 + u_prod)              (u_prod: attn_probs_cases -- 0, or the split product's 2^-16 + 2^-23)
    p   = 2^(c2 s - lse2[q]): relative error E'(q, k) of attn_apply_cases (scores, the lse2 route, v_exp, the N-term sum)
    p g one rounding: u
    max(., 0): |max(a, 0) - max(b, 0)| <= |a - b|, so the rectifier passes the error of the product on and adds none
    the sum over q and h: the plain form's chain, fewer than q_rows + 14 roundings of non-negative terms: gamma_{q_rows + 14}

so per term |a - a_ref| <= p_ref (|g| (E' + u) + (1 + E') dg) (to first order in u; the factor (1 + E') carries the cross term), the
accumulation adds gamma_{q_rows + 14} of the terms' sum -- which the first term's |g| p_ref bounds --, and with u + gamma_{q_rows + 14} <=
gamma_{q_rows + 15}:

    gate:   |Y - Y_ref| <= sum_h sum_q |W| p_ref (|g| (E' + gamma_{q_rows + 15}) + (1 + E') dg) / 12 + 2^-100 sum_q |W| max |g|

for every element (the floor: probabilities below 2^-126 are flushed by v_exp_f32, as in the plain form; max |g| per clip).  A zero dO makes
the limit zero and the result must be zero exactly (case_zero).  There is no row-sum condition: the rectifier keeps none.

test_attn_relevance_gate_passes_the_sound_pipeline / _rejects_defects (test_emu_attn_relevance.py) show what the gate passes and refuses."""
import functools

import torch

from maest_amd import _lib, ops
from tests import attn_apply_cases as AC
from tests import attn_probs_cases as PC
from tests import guard
from tests.kernel_cases import f16_build, f32, lp, rnd

H, HD, E = PC.H, PC.HD, PC.E
U, LN2, FLOOR, SCALE = PC.U, PC.LN2, PC.FLOOR, PC.SCALE
CODES = PC.CODES
SHAPES = AC.SHAPES            # (B, N, q_rows, R): the smallest shapes at which the kernel can go wrong (attn_apply_cases)
SHAPE_GPU = AC.SHAPE_GPU      # three key blocks, the eight-row kernel (the device only)
weights = AC.weights


@functools.lru_cache(maxsize=None)
def _dout(B, N, code, seed, f16):
    """-> (dO as the kernel reads it: [B * N, 768] of the operand type, its values as stored in fp64)."""
    x = rnd((B * N, E), seed)
    d = x.contiguous() if code in ("f32", "x3") else lp(x)
    return d, f32(d).double()


def dout(B, N, q_rows, code, seed=52, variant=None):
    """The dO operand of a case (shared, never modified: the variants are clones).  variant "zero": all zero; "nan": NaN in rows >= q_rows."""
    d, ds = _dout(B, N, code, seed, f16_build() and code in ("16", "qs"))
    if variant == "zero":
        d = torch.zeros_like(d)
    elif variant == "nan":
        d = d.clone().reshape(B, N, E)
        d[:, q_rows:] = float("nan")
        d = d.reshape(B * N, E)
    else:
        assert variant is None
    return d, ds


def _dheads(ds, B, N):
    """[B * N, 768] -> [B, 12, N, 64]"""
    return ds.reshape(B, N, H, HD).permute(0, 2, 1, 3)


def reference(xs, ds, w, B, N, q_rows, c2, u_prod):
    """fp64 -> (Y_ref [B, R, N], its limit [B, R, N]): the module docstring."""
    _, _, _, _, p_ref, _, e_apply = AC.reference(xs, w, B, N, q_rows, c2, u_prod)
    _, _, v = PC._heads(xs, B, N)
    do = _dheads(ds, B, N)[:, :, :q_rows]
    g = do @ v.transpose(-2, -1)                                               # [B, 12, q_rows, N]
    dg = (do.abs() @ v.abs().transpose(-2, -1)) * (PC.gamma(66) + u_prod)
    wd = w[:, :, :q_rows].double()
    wa = wd.abs()
    y_ref = torch.einsum("brq,bhqk->brk", wd, (p_ref * g).clamp_min(0)) / 12
    term = p_ref * (g.abs() * (e_apply + PC.gamma(q_rows + 15)) + (1 + e_apply) * dg)
    lim = torch.einsum("brq,bhqk->brk", wa, term) / 12 + FLOOR * wa.sum(-1, keepdim=True) * g.abs().amax((1, 2, 3)).reshape(B, 1, 1)
    return y_ref, lim


@functools.lru_cache(maxsize=None)
def _reference_of(B, N, q_rows, R, code, seed, spike, times, f16):
    _, xs = PC._operands(B, N, code, seed, spike, times, f16)
    _, ds = _dout(B, N, code, 52, f16)
    return reference(xs, ds, weights(B, R, N, q_rows), B, N, q_rows, PC.c2_of(code), PC.U_PROD[code])


def reference_of(B, N, q_rows, R, code, seed=30, spike=False, times=1.0):
    """The reference of operands(...), dout(...) and weights(...) (computed once per case and build, shared by the tests, never modified)."""
    return _reference_of(B, N, q_rows, R, code, seed, spike, times, f16_build() and code in ("16", "qs"))


def gate(what, y, ref):
    """The condition of the module docstring on y [B, R, N]; prints and returns the worst share of the limit used."""
    y_ref, lim = ref
    y = y.detach().cpu().double()
    assert y.shape == y_ref.shape, (what, tuple(y.shape), tuple(y_ref.shape))
    assert bool(torch.isfinite(y).all()), f"{what}: {int((~torch.isfinite(y)).sum())} non-finite results (elements never written?)"
    err = (y - y_ref).abs()
    ratio = float((err / lim.clamp_min(1e-300)).max())
    print(f"  {what}: worst |Y - Y_ref| / limit = {ratio:.3g} (relative limit {float((lim / y_ref.clamp_min(1e-300)).min()):.1e} and up; "
          f"{float((y_ref == 0).double().mean()):.2f} of the reference is exactly zero)")
    bad = err > lim
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the bound, worst {ratio:.3g} x; first at "
                                 f"{tuple(int(i) for i in bad.nonzero()[0])}")
    return ratio


def run(dev, B, N, q_rows, R, code, w=None, variant=None, **kw):
    qkv, _ = PC.operands(B, N, code, **kw)
    d, _ = dout(B, N, q_rows, code, variant=variant)
    w = weights(B, R, N, q_rows) if w is None else w
    return ops.attn_relevance(qkv.to(dev), d.to(dev), w.to(dev), B, N, SCALE, q_rows=q_rows, x3=code == "x3", q_prescaled=code == "qs")


_bits_equal = AC._bits_equal


def case_relevance(dev, B, N, q_rows, R, code, **kw):
    """The gate.  Returns the share of the limit used."""
    print(f"attention relevance, {'f16' if f16_build() else 'bf16'} build, code {code}, B = {B}, N = {N}, q_rows = {q_rows}, R = {R}, {kw or 'plain'}")
    y = run(dev, B, N, q_rows, R, code, **kw).cpu()
    assert y.dtype == torch.float32 and y.shape == (B, R, N)
    return gate("Y", y, reference_of(B, N, q_rows, R, code, **kw))


def case_zero(dev, B, N, q_rows, R, code):
    """dO = 0: Y = 0, bit for bit."""
    y = run(dev, B, N, q_rows, R, code, variant="zero").cpu()
    _bits_equal("Y of a zero dO", y, torch.zeros_like(y))


def case_nan_rows(dev, B, N, q_rows, R, code):
    """Rows >= q_rows of dO and columns >= q_rows of W hold NaN: Y is finite and bit-identical to the result with finite values there."""
    assert q_rows < N
    y = run(dev, B, N, q_rows, R, code).cpu()
    yn = run(dev, B, N, q_rows, R, code, w=weights(B, R, N, q_rows, nan_tail=True), variant="nan").cpu()
    assert bool(torch.isfinite(yn).all()), "NaN in the rows of dO / the columns of W >= q_rows reached Y"
    _bits_equal("Y with NaN in dO rows and W columns >= q_rows", yn, y)


def case_repeat(dev, B, N, q_rows, R, code):
    a, b = run(dev, B, N, q_rows, R, code).cpu(), run(dev, B, N, q_rows, R, code).cpu()
    _bits_equal("two calls", a, b)


def run_raw(dev, B, N, q_rows, R, code):
    """The flagged call with its workspace in hand -> (Y, workspace), both allocated filled with the guard's pattern, through the names the
    guard replaces when one is active; dO and W carry NaN past q_rows."""
    qkv, _ = PC.operands(B, N, code)
    d, _ = dout(B, N, q_rows, code, variant="nan" if q_rows < N else None)
    qkv, d, w = qkv.to(dev), d.to(dev), weights(B, R, N, q_rows, nan_tail=q_rows < N).to(dev)
    ops._chk(qkv, d, w)
    y = guard.fill_pattern_(ops.torch.empty((B, R, N), dtype=torch.float32, device=dev))
    work = guard.fill_pattern_(ops.torch.empty((B, H, N), dtype=torch.float32, device=dev))
    base = {"f32": _lib.F32, "x3": _lib.F32X3, "16": _lib.BF16, "qs": _lib.BF16_QS}[code]
    ops.call("maest_attn_bwd_rows", ops._p(qkv), ops._p(d), ops._p(w), None, ops._p(work), ops._p(y), B, N,
             base | _lib.ATTN_APPLY | _lib.ATTN_APPLY_GRAD | _lib.attn_apply_rows(R), SCALE, q_rows, ops._s(qkv))
    return y, work


def case_regions(dev, B, N, q_rows, R, code):
    """Y has exactly [B, R, N] elements, all written; the workspace holds a finite lse2 in rows < q_rows and is untouched past them.  (Under
    the guard: dO and W are const, nothing outside the operands is read or written.)"""
    y, work = run_raw(dev, B, N, q_rows, R, code)
    assert y.shape == (B, R, N) and not bool(guard.untouched(y).any()), "elements of Y were never written"
    gate("Y (raw call)", y.cpu(), reference_of(B, N, q_rows, R, code))
    assert bool(torch.isfinite(work[:, :, :q_rows]).all()), "lse2 of a row < q_rows is missing"
    if q_rows < N:
        assert bool(guard.untouched(work[:, :, q_rows:]).all()), "the workspace was written at rows >= q_rows"


def case_argument_errors(dev):
    """The refusals of the flag: MAEST_ERR_INVALID (status 1) with its message in maest_last_error(); the accepted codes run through both
    entries; without the flag nothing changes (attn_apply_cases.case_argument_errors covers the plain form as it was)."""
    import pytest
    B, N, R = 1, 8, 2
    qkv = rnd((B * N, 3 * E), 3).to(dev)
    qkv16 = lp(rnd((B * N, 3 * E), 3)).to(dev)
    do = torch.zeros(B * N * E + 4, dtype=torch.float32, device=dev)
    do16 = lp(torch.zeros(B * N * E + 8)).to(dev)
    w = torch.ones(B * R * N + 4, dtype=torch.float32, device=dev)
    y = torch.zeros(B * 8 * N + 4, dtype=torch.float32, device=dev)
    work = torch.zeros(B * H * N + 4, dtype=torch.float32, device=dev)
    A, G, rows = _lib.ATTN_APPLY, _lib.ATTN_APPLY_GRAD, _lib.attn_apply_rows
    st = ops._s(qkv)

    def call(q=qkv, o=do, w_=w, l=None, d=work, y_=y, code=_lib.F32 | A | G | rows(R), q_rows=N, entry="maest_attn_bwd_rows"):
        args = [ops._p(q), ops._p(o), ops._p(w_), ops._p(l), ops._p(d), ops._p(y_), B, N, code, SCALE]
        _lib.call(entry, *args, *([q_rows] if entry.endswith("_rows") else []), st)

    def refused(match, **kw):
        with pytest.raises(_lib.MaestHipError, match=match) as e:
            call(**kw)
        assert "status 1" in str(e.value)

    refused("bad dtype", code=_lib.F32 | G, l=work)                       # the flag without MAEST_ATTN_APPLY: the backward's dtype check
    refused("bad dtype", code=_lib.F32 | G | rows(R), l=work)
    refused("bad dtype", code=_lib.F32 | A | G | _lib.ATTN_PROBS | rows(R))
    refused("bad dtype", code=_lib.F32 | A | G | _lib.ATTN_PROBS_MEAN | rows(R))
    refused("bad dtype", code=_lib.SPLIT3_A | A | G | rows(R))
    refused("MAEST_F32X3_A3", code=_lib.F32X3_A3 | A | G | rows(R))
    refused("null pointer", o=None)                                       # with the flag, `out` is an operand
    refused("pass NULL", l=work)
    refused("pass NULL", code=_lib.F32 | A | rows(R))                     # ... and without it `out` is still refused
    refused("alignment", o=do[1:])
    refused("alignment", w_=w[1:])
    refused("q_rows", q_rows=0)
    refused("q_rows", q_rows=N + 1)
    refused("outside 1..8", code=_lib.F32 | A | G | rows(9))
    for code, q, o in ((_lib.F32, qkv, do), (_lib.F32X3, qkv, do), (_lib.BF16, qkv16, do16), (_lib.BF16_QS, qkv16, do16)):
        for r in (1, 2, 5, 8):
            call(q=q, o=o, code=code | A | G | rows(r))
    call(entry="maest_attn_bwd")


def case_neighbours_unchanged(dev, B=1, N=70):
    """A plain maest_attn_bwd call and a plain MAEST_ATTN_APPLY call before and after a flagged one give bit-identical results."""
    qkv, _ = PC.operands(B, N, "f32")
    qkv = qkv.to(dev)
    out, lse = ops.attn_fwd(qkv, B, N, SCALE, save_lse=True)
    do = rnd((B * N, E), 9).to(dev)
    before = ops.attn_bwd(qkv, out, do, lse, B, N, SCALE).cpu()
    plain_before = AC.run(dev, B, N, N, 2, "f32").cpu()
    run(dev, B, N, N, 2, "f32")
    after = ops.attn_bwd(qkv, out, do, lse, B, N, SCALE).cpu()
    plain_after = AC.run(dev, B, N, N, 2, "f32").cpu()
    _bits_equal("maest_attn_bwd around a flagged call", after, before)
    _bits_equal("MAEST_ATTN_APPLY around a flagged call", plain_after, plain_before)
    AC.gate("the plain form beside the flagged one", plain_after, AC.reference_of(B, N, N, 2, "f32"))


# ---------------------------------------------------------------------------------------------- doctored pipelines (tests of the gate)
DEFECTS = ("signed", "abs", "rectify after the mean", "g from K", "no 1/12", "all queries", "bf16 p")


def pipeline64(xs, ds, w, B, N, q_rows, c2, defect=None):
    """The kernel's launches in fp64 on the stored operands, with one of the defects the gate must refuse:
       "signed"                  the signed product p g (no rectifier)
       "abs"                     |p g| instead of max(p g, 0)
       "rectify after the mean"  the rectifier applied to the head mean of p g
       "g from K"                dP formed from the k columns instead of the v columns
       "no 1/12"                 the head sum left unscaled
       "all queries"             queries >= q_rows included (W and dO hold finite values there)
       "bf16 p"                  probabilities rounded to bf16 before the product"""
    q, k, v = PC._heads(xs, B, N)
    nq = N if defect == "all queries" else q_rows
    q = q[:, :, :nq]
    do = _dheads(ds, B, N)[:, :, :nq]
    t = c2 * (q @ k.transpose(-2, -1))
    m = t.amax(-1, keepdim=True)
    lse2 = m + torch.log2(torch.exp2(t - m).sum(-1, keepdim=True))
    p = torch.exp2(t - lse2)
    if defect == "bf16 p":
        p = p.float().bfloat16().double()
    g = do @ (k if defect == "g from K" else v).transpose(-2, -1)
    a = p * g
    wd = w[:, :, :nq].double()
    if defect == "rectify after the mean":
        return torch.einsum("brq,bqk->brk", wd, a.mean(1).clamp_min(0))
    a = a if defect == "signed" else a.abs() if defect == "abs" else a.clamp_min(0)
    y = torch.einsum("brq,bhqk->brk", wd, a)
    return y if defect == "no 1/12" else y / 12
