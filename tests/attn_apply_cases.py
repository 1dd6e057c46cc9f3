"""Weighted attention pooling (MAEST_ATTN_APPLY, ops.attn_apply: the step of attention rollout) against an error bound that is DERIVED, not
measured (a sibling of attn_probs_cases: the same operands, the same fp64 reference, the same two builds; run by test_emu_attn_apply.py under
the emulator and by test_attn_apply_gpu.py on the device).

The reference is fp64:  Y_ref[b, r, k] = (1 / 12) sum_h sum_{q < q_rows} W[b, r, q] p_ref_h[q, k],  p_ref the fp64 softmax of the operands as
stored (attn_probs_cases.reference).  The kernel never normalises by a division; its probability is

    p = 2^(c2 s - lse2[q]),    lse2 = fp32(m + log2 l)          (m, l: the online maximum and fp32 sum of attn_probs_kernel's first pass)

so its exponent carries, next to the error delta(q, k) of attn_probs_cases (products, fp32 sums, the scale fma, the max subtraction) and the
error of l (ln 2 max_j delta(q, j) + N u, relative: the sum's exponents and its N terms), the roundings of the lse2 route.  The bound allows
an fp32 route its three roundings:

    log2:     4 u |log2 l| <= 4 u log2 N        (a log2f of at most 4 ulp; 1 <= l <= N because the maximum's own term is 2^0)
    the add:  u |lse2|
    t - lse2: u |t - lse2|                      (one fma)

The kernel forms m + log2 l in fp64 and rounds it to fp32 once (attn_apply_stats_kernel: once per row, so the cost is nothing), which uses
the second term alone -- its log2 and its add are off by parts in 2^52; the first term is kept as the bound of the route as specified and is
deliberately wider than this kernel needs (4 log2 N against 2 |lse2| + 2 |t - lse2|: a fifth of the route's allowance at the test shapes).
With a factor 2 on the last two (they are taken at the reference's values, the kernel's differ by the terms above) the probability's relative
error is at most

    E'(q, k) = E(q, k) + ln 2 * u * (4 log2 N + 2 |lse2[q]| + 2 |t[q, k] - lse2[q]|)          E: attn_probs_cases (its 1 u of the division
                                                                                              stays in: an upper bound either way)

The product keeps P and W in fp32: per element a chain of at most q_rows / 2 fmas, the half-wave add, eleven head adds, the multiplication by
fp32(1 / 12) and that constant's own rounding -- fewer than q_rows + 14 roundings of non-negative terms: gamma_{q_rows + 14}.  Probabilities
below 2^-126 are flushed by v_exp_f32: an absolute 2^-100 per unit of weight covers them.

    gate:   |Y - Y_ref| <= sum_h sum_q |W| p_ref (E' + gamma_{q_rows + 14}) / 12 + 2^-100 sum_q |W|            for every element

The row sums: sum_k Y_ref[b, r, k] = sum_{q < q_rows} W[b, r, q] exactly.  A row of the kernel's P sums to l' / l, l' the sum of the second
launch's exponentials: the errors of the scores cancel as far as both launches form the same scores; they are NOT assumed bit-equal (the
operands change places between the launches), so every score may differ by 2 a (gamma_66 + u_prod); the lse2 roundings above do not cancel;
the N-term sum and the exponentials cost (N + 8) u on either side:

    D(q) = ln 2 * (u max_k (4 log2 N + 2 |lse2| + 2 |t - lse2|) + 2 max_k a (gamma_66 + u_prod)) + 2 (N + 8) u
    gate:   |sum_k Y - sum_q W| <= sum_h sum_q |W| (D_h(q) + gamma_{q_rows + 14}) / 12 + N 2^-100 sum_q |W|     for every (clip, weight row)

test_attn_apply_gate_passes_the_sound_pipeline / _rejects_defects (test_emu_attn_apply.py) show what the gate passes and what it refuses."""
import functools
import math

import numpy as np
import torch

from maest_amd import _lib, ops
from tests import attn_probs_cases as PC
from tests import guard
from tests.kernel_cases import f16_build, lp, rnd

H, HD, E = PC.H, PC.HD, PC.E
U, LN2, FLOOR, SCALE = PC.U, PC.LN2, PC.FLOOR, PC.SCALE
CODES = PC.CODES

# (B, N, q_rows, R): the smallest shapes at which the kernel can go wrong
SHAPES = [(2, 64, 64, 2),       # one full query tile, one key block
          (2, 70, 70, 2),       # ragged last query tile, ragged key block
          (2, 161, 161, 3),     # two key blocks, three query tiles; R = 3 in the four-row kernel
          (2, 161, 2, 2),       # the top block of a head-token rollout
          (2, 161, 40, 1)]      # a partial query tile, one weight row
SHAPE_GPU = (1, 353, 353, 8)    # three key blocks, the eight-row kernel (the device only)


@functools.lru_cache(maxsize=None)
def _weights(B, R, N, seed):
    """fp32 [B, R, N], non-negative, about one exact zero in eight."""
    w = rnd((B, R, N), seed).abs()
    w[rnd((B, R, N), seed + 1) > 1.15] = 0.0
    return w.contiguous()


def weights(B, R, N, q_rows, seed=41, nan_tail=False):
    """The weight rows of a case (shared, never modified: callers get a clone when they ask for the NaN tail)."""
    w = _weights(B, R, N, seed)
    if nan_tail:
        w = w.clone()
        w[:, :, q_rows:] = float("nan")
    return w


def reference(xs, w, B, N, q_rows, c2, u_prod):
    """fp64 -> (Y_ref [B, R, N], its limit [B, R, N], sum_q W [B, R], the row-sum limit [B, R], p_ref, E, E'): the module docstring."""
    p_ref, e_maps = PC.reference(xs, B, N, q_rows, c2, u_prod)
    q, k, _ = PC._heads(xs, B, N)
    q = q[:, :, :q_rows]
    t = c2 * (q @ k.transpose(-2, -1))
    a = c2 * (q.abs() @ k.abs().transpose(-2, -1))
    lse2 = torch.logsumexp(t * LN2, -1, keepdim=True) / LN2
    route = U * (4 * math.log2(N) + 2 * lse2.abs() + 2 * (t - lse2).abs())
    e_apply = e_maps + LN2 * route
    g = PC.gamma(q_rows + 14)
    wa = w[:, :, :q_rows].double().abs()
    wsum = w[:, :, :q_rows].double().sum(-1)
    y_ref = torch.einsum("brq,bhqk->brk", w[:, :, :q_rows].double(), p_ref) / 12
    lim = torch.einsum("brq,bhqk->brk", wa, p_ref * (e_apply + g)) / 12 + FLOOR * wa.sum(-1, keepdim=True)
    d = LN2 * (route.amax(-1) + 2 * a.amax(-1) * (PC.gamma(66) + u_prod)) + 2 * (N + 8) * U      # [B, 12, q_rows]
    rowlim = torch.einsum("brq,bhq->br", wa, d + g) / 12 + N * FLOOR * wa.sum(-1)
    return y_ref, lim, wsum, rowlim, p_ref, e_maps, e_apply


@functools.lru_cache(maxsize=None)
def _reference_of(B, N, q_rows, R, code, seed, spike, times, f16):
    _, xs = PC._operands(B, N, code, seed, spike, times, f16)
    return reference(xs, weights(B, R, N, q_rows), B, N, q_rows, PC.c2_of(code), PC.U_PROD[code])


def reference_of(B, N, q_rows, R, code, seed=30, spike=False, times=1.0):
    """The reference of operands(...) and weights(...) (computed once per case and build, shared by the tests, never modified)."""
    return _reference_of(B, N, q_rows, R, code, seed, spike, times, f16_build() and code in ("16", "qs"))


def gate(what, y, ref):
    """The two conditions of the module docstring on y [B, R, N]; prints and returns the worst shares of the two limits used."""
    y_ref, lim, wsum, rowlim = ref[:4]
    y = y.detach().cpu().double()
    assert y.shape == y_ref.shape, (what, tuple(y.shape), tuple(y_ref.shape))
    assert bool(torch.isfinite(y).all()), f"{what}: {int((~torch.isfinite(y)).sum())} non-finite results (elements never written?)"
    err = (y - y_ref).abs()
    ratio = float((err / lim).max())
    dsum = (y.sum(-1) - wsum).abs()
    rratio = float((dsum / rowlim).max())
    print(f"  {what}: worst |Y - Y_ref| / limit = {ratio:.3g} (relative limit {float((lim / y_ref.clamp_min(1e-300)).min()):.1e} and up), "
          f"worst |sum_k Y - sum_q W| / limit = {rratio:.3g} (limit {float(rowlim.min()):.1e} .. {float(rowlim.max()):.1e})")
    bad = err > lim
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the bound, worst {ratio:.3g} x; first at "
                                 f"{tuple(int(i) for i in bad.nonzero()[0])}")
    assert rratio <= 1, f"{what}: a row sums to the sum of its weights {float(dsum.max()):+.3e} off, {rratio:.3g} x its limit"
    return ratio, rratio


def run(dev, B, N, q_rows, R, code, w=None, **kw):
    qkv, _ = PC.operands(B, N, code, **kw)
    w = weights(B, R, N, q_rows) if w is None else w
    return ops.attn_apply(qkv.to(dev), w.to(dev), B, N, SCALE, q_rows=q_rows, x3=code == "x3", q_prescaled=code == "qs")


def _bits_equal(what, got, want):
    same = got.view(torch.int32) == want.view(torch.int32)
    assert bool(same.all()), (f"{what}: {int((~same).sum())}/{same.numel()} elements differ; first at "
                              f"{tuple(int(i) for i in (~same).nonzero()[0])}")


def case_apply(dev, B, N, q_rows, R, code, **kw):
    """The gate.  Returns (share of the element limit, share of the row-sum limit)."""
    print(f"attention apply, {'f16' if f16_build() else 'bf16'} build, code {code}, B = {B}, N = {N}, q_rows = {q_rows}, R = {R}, {kw or 'plain'}")
    y = run(dev, B, N, q_rows, R, code, **kw).cpu()
    assert y.dtype == torch.float32 and y.shape == (B, R, N)
    return gate("Y", y, reference_of(B, N, q_rows, R, code, **kw))


def case_nan_columns(dev, B, N, q_rows, R, code):
    """Columns >= q_rows of W hold NaN: Y is finite and bit-identical to the result with finite columns there."""
    assert q_rows < N
    y = run(dev, B, N, q_rows, R, code).cpu()
    yn = run(dev, B, N, q_rows, R, code, w=weights(B, R, N, q_rows, nan_tail=True)).cpu()
    assert bool(torch.isfinite(yn).all()), "NaN weights in columns >= q_rows reached Y"
    _bits_equal("Y with NaN in the weight columns >= q_rows", yn, y)


def case_repeat(dev, B, N, q_rows, R, code):
    a, b = run(dev, B, N, q_rows, R, code).cpu(), run(dev, B, N, q_rows, R, code).cpu()
    _bits_equal("two calls", a, b)


def case_onehot(dev, B, N, code, queries=(0, 1, 37)):
    """W one-hot at query q0 gives row q0 of the head-mean maps (ops.attn_probs): two kernels, each inside its own bound of the same
    reference -- E for the maps (and the 13 roundings of their mean), E' + gamma_{N + 14} for this one."""
    R = len(queries)
    w = torch.zeros(B, R, N)
    for r, q0 in enumerate(queries):
        w[:, r, q0] = 1.0
    y = run(dev, B, N, N, R, code, w=w).cpu().double()
    pm = PC.run(dev, B, N, N, code, head_mean=True).cpu().double()[:, list(queries)]
    _, xs = PC.operands(B, N, code)
    _, _, _, _, p_ref, e_maps, e_apply = reference(xs, w, B, N, N, PC.c2_of(code), PC.U_PROD[code])
    lim = (p_ref * (e_maps + e_apply + PC.gamma(13) + PC.gamma(N + 14))).sum(1)[:, list(queries)] / 12 + 2 * FLOOR
    ratio = float(((y - pm).abs() / lim).max())
    print(f"  one-hot weights against the head-mean maps, code {code}: worst |Y - maps row| / limit = {ratio:.3g}")
    assert ratio <= 1, f"one-hot rows differ from the head-mean maps by {ratio:.3g} x the two kernels' bounds"


def run_raw(dev, B, N, q_rows, R, code):
    """The flagged call with its workspace in hand (ops.attn_apply keeps it to itself) -> (Y, workspace), both allocated filled with the
    guard's pattern, through the names the guard replaces when one is active."""
    qkv, _ = PC.operands(B, N, code)
    qkv, w = qkv.to(dev), weights(B, R, N, q_rows, nan_tail=q_rows < N).to(dev)
    ops._chk(qkv, w)
    y = guard.fill_pattern_(ops.torch.empty((B, R, N), dtype=torch.float32, device=dev))
    work = guard.fill_pattern_(ops.torch.empty((B, H, N), dtype=torch.float32, device=dev))
    base = {"f32": _lib.F32, "x3": _lib.F32X3, "16": _lib.BF16, "qs": _lib.BF16_QS}[code]
    ops.call("maest_attn_bwd_rows", ops._p(qkv), None, ops._p(w), None, ops._p(work), ops._p(y), B, N,
             base | _lib.ATTN_APPLY | _lib.attn_apply_rows(R), SCALE, q_rows, ops._s(qkv))
    return y, work


def case_regions(dev, B, N, q_rows, R, code):
    """Y has exactly [B, R, N] elements, all written; the workspace holds a finite lse2 in rows < q_rows and is untouched past them."""
    y, work = run_raw(dev, B, N, q_rows, R, code)
    assert y.shape == (B, R, N) and not bool(guard.untouched(y).any()), "elements of Y were never written"
    gate("Y (raw call)", y.cpu(), reference_of(B, N, q_rows, R, code))
    assert bool(torch.isfinite(work[:, :, :q_rows]).all()), "lse2 of a row < q_rows is missing"
    if q_rows < N:
        assert bool(guard.untouched(work[:, :, q_rows:]).all()), "the workspace was written at rows >= q_rows"


def case_argument_errors(dev):
    """Every refusal of the flagged form returns MAEST_ERR_INVALID (status 1) with its message in maest_last_error(); the accepted codes run;
    calls without the flag behave as before."""
    import pytest
    B, N, R = 1, 8, 2
    qkv = rnd((B * N, 3 * E), 3).to(dev)
    qkv16 = lp(rnd((B * N, 3 * E), 3)).to(dev)
    w = torch.ones(B * R * N + 4, dtype=torch.float32, device=dev)
    y = torch.zeros(B * 8 * N + 4, dtype=torch.float32, device=dev)
    work = torch.zeros(B * H * N + 4, dtype=torch.float32, device=dev)
    out = torch.zeros(B * N, E, dtype=torch.float32, device=dev)
    A, rows = _lib.ATTN_APPLY, _lib.attn_apply_rows
    st = ops._s(qkv)

    def call(q=qkv, o=None, w_=w, l=None, d=work, y_=y, code=_lib.F32 | A | rows(R), q_rows=N, entry="maest_attn_bwd_rows"):
        args = [ops._p(q), ops._p(o), ops._p(w_), ops._p(l), ops._p(d), ops._p(y_), B, N, code, SCALE]
        _lib.call(entry, *args, *([q_rows] if entry.endswith("_rows") else []), st)

    def refused(match, **kw):
        with pytest.raises(_lib.MaestHipError, match=match) as e:
            call(**kw)
        assert "status 1" in str(e.value)

    refused("MAEST_F32X3_A3", code=_lib.F32X3_A3 | A | rows(R))
    refused("pass NULL", l=work)
    refused("pass NULL", o=out)
    refused("q_rows", q_rows=0)
    refused("q_rows", q_rows=N + 1)
    refused("alignment", y_=y[1:])
    refused("alignment", w_=w[1:])
    refused("alignment", d=work[1:])
    refused("alignment", q=qkv.reshape(-1)[1:])
    refused("bad dtype", code=_lib.SPLIT3_A | A | rows(R))
    refused("bad dtype", code=_lib.F16 | A | rows(R))
    refused("bad dtype", code=_lib.F32 | A | _lib.ATTN_PROBS | rows(R))
    refused("outside 1..8", code=_lib.F32 | A | rows(9))
    refused("outside 1..8", code=_lib.F32 | A | rows(256))
    refused("null pointer", y_=None)
    refused("null pointer", w_=None)
    refused("null pointer", d=None)
    # without the flag the entry is the backward it was: the rows field alone is a bad dtype, and a backward without lse a null pointer
    refused("bad dtype", code=_lib.F32 | rows(2), l=work, o=out)
    refused("null pointer", code=_lib.F32)
    refused("null pointer", code=_lib.F32, entry="maest_attn_bwd")
    # ... and the accepted codes run, every row count, through both entries
    for code, q in ((_lib.F32, qkv), (_lib.F32X3, qkv), (_lib.BF16, qkv16), (_lib.BF16_QS, qkv16)):
        for r in (1, 2, 5, 8):
            call(q=q, code=code | A | rows(r))
    call(entry="maest_attn_bwd")


def case_backward_unchanged(dev, B=1, N=70):
    """A plain maest_attn_bwd call (no flag) before and after a flagged one gives bit-identical gradients."""
    qkv, _ = PC.operands(B, N, "f32")
    qkv = qkv.to(dev)
    out, lse = ops.attn_fwd(qkv, B, N, SCALE, save_lse=True)
    dout = rnd((B * N, E), 9).to(dev)
    before = ops.attn_bwd(qkv, out, dout, lse, B, N, SCALE).cpu()
    run(dev, B, N, N, 2, "f32")
    after = ops.attn_bwd(qkv, out, dout, lse, B, N, SCALE).cpu()
    _bits_equal("maest_attn_bwd around a flagged call", after, before)


# ---------------------------------------------------------------------------------------------- doctored pipelines (tests of the gate)
DEFECTS = ("no 1/12", "all queries", "padding", "ln lse", "bf16 p", "bf16 c2")


def pipeline64(xs, w, B, N, q_rows, c2, defect=None):
    """The kernel's two launches in fp64 on the stored operands, with one of the defects the gate must refuse:
       "no 1/12"      the head sum left unscaled
       "all queries"  queries >= q_rows included (W holds finite weights there)
       "padding"      the padding keys of the ragged last tile left unmasked in the statistics (zero keys: score 0)
       "ln lse"       the row statistic taken in the natural-log domain and used as a log2 exponent
       "bf16 p"       probabilities rounded to bf16 before the product
       "bf16 c2"      the exponent factor rounded to bf16"""
    q, k, _ = PC._heads(xs, B, N)
    nq = N if defect == "all queries" else q_rows
    q = q[:, :, :nq]
    if defect == "bf16 c2":
        c2 = float(torch.tensor(c2).bfloat16())
    t = c2 * (q @ k.transpose(-2, -1))
    ts = torch.cat([t, torch.zeros(t.shape[:-1] + (-N % 64,), dtype=t.dtype)], -1) if defect == "padding" else t
    m = ts.amax(-1, keepdim=True)
    l = torch.exp2(ts - m).sum(-1, keepdim=True)
    lse2 = m * LN2 + torch.log(l) if defect == "ln lse" else m + torch.log2(l)
    p = torch.exp2(t - lse2)
    if defect == "bf16 p":
        p = p.float().bfloat16().double()
    y = torch.einsum("brq,bhqk->brk", w[:, :, :nq].double(), p)
    return y if defect == "no 1/12" else y / 12
