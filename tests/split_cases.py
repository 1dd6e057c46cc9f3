"""The split-bf16 ("bf16x3") kernels against what their roundings allow (a sibling of attention_cases / epilogue_cases: the same helpers, run under
the emulator at tiny shapes and on the device at the shapes of tests/test_split_gpu.py).

In bf16x3 the tensors are fp32 and every matrix product is three bf16 MFMAs on hi / lo operand splits.  kernel_cases.case_split_precision
accepts 1e-4 of the output's maximum, about 20 x what the split achieves: a `lo` part truncated instead of rounded (1.7 x the error), a `hi`
part truncated (2.9 x), a tile that silently degrades to plain bf16 all pass it.  Here every split kernel is measured against an fp64
REFERENCE on the unsplit fp32 operands next to an fp64 MODEL of the same pipeline that rounds where the kernel rounds and nowhere else:

    E_rms = rms(x - ref) / rms(ref),  E_max = max |x - ref| / max |ref|           per output tensor
    gate:   E_rms(kernel) <= 1.25 E_rms(model)   and   E_max(kernel) <= 2 E_max(model)        (attention_cases.RMS_MARGIN, MAX_MARGIN)

The margins cover what the model leaves out -- fp32 accumulation order and v_exp_f32, measured on the host at < 1 % of the model's error
(the three-term product evaluated in fp32 sits within 0.1 % of its fp64 evaluation) -- and the sampling noise of a maximum.  The smallest
defect of tests/test_split_gate_cpu.py (`lo` truncated) sits at 1.67 x rms.

The model's rounding points, each with the source line that performs it (bf() = round to nearest even to bf16):
  every product      hi = bf(x), lo = bf(x - hi) of both operands,     common.h split_bf16x8 (`hb = pack_bf2(x0, x1)`, `l[..] = pack_bf2(r0, r1)`),
                     sum of lo_a hi_b + hi_a lo_b + hi_a hi_b          common.h mma_chunk2<T, true> (three MFMAs, "small terms first")
  NT GEMM            a, b split per fragment pair                      gemm256.hip gemm_nt256w_kernel, `if constexpr (X3)` branch of compute()
                     (bias, GELU, MUL, RESIDUAL: fp32 / libm on the fp32 accumulator: no rounding of the model's)
  NT GEMM over 3 K   the same three terms as ONE bf16 GEMM: rows [hi | hi | lo] x [hi | lo | hi] (include/maest_hip.h MAEST_SPLIT3_A / _B)
  TN GEMM            a, b split per slice                              gemm256.hip gemm_tn256_kernel, `if constexpr (X3)` (mma_chunk2 on fa / fb);
                     colsum is an fp32 sum of the unsplit a            the same kernel, `else cs += u2f(w)`
  attention forward  q split once, k and v split once per tile         attention.hip attn_fwd_x3s_kernel (x3_split4 in the Q prologue and in
                                                                       x3_tile_store); attn_fwd_kernel<float, true>: mma_rows<T, X3> /
                                                                       mma_transposed<T, X3> split the same values at the point of use
                     S = the three terms of q k^T
                     P = 2^(c2 S - m), m the tile-by-tile running     attn_fwd_x3s_kernel / attn_fwd_kernel `m_new = fmaxf(m_run, mx * c2)`
                     maximum; P split per tile                         attn_fwd_x3s_kernel `split_bf2(s[kb][8 * st + 2 * j], ...)`;
                                                                       attn_fwd_kernel: mma_transposed<T, X3>(o, v_lds, .., s[kb])
                     l = the row sum of the UNSPLIT P                  both kernels `ps += pv`
                     out fp32 (no rounding), or [hi | hi | lo] rows    attention.hip store_dT_split3 (out_split3: asserted bit-equal to the split
                                                                       of the fp32 result, so the model stops at fp32)
  attention backward S = three terms of q k^T, dP = three terms        attention.hip attn_bwd_dkdv_kernel<float, true> `mma_rows<T, X3>(s, q_lds, ..)`,
                     of dO v^T (q, k, v, dO split)                     `mma_rows<T, X3>(dp, do_lds, ..)`; attn_bwd_dq_kernel<float, true> the same
                     P = 2^(c2 S - lse log2 e), dS = P (dP - delta)    fp32; delta = rowsum(dO * O) is an fp32 sum (attn_delta_kernel): no rounding
                     dV = three terms of P^T dO (P, dO split)          attn_bwd_dkdv_kernel `mma_transposed<T, X3>(dv, do_lds, .., s)`
                     dK = scale x three terms of dS^T q (dS, q split)  attn_bwd_dkdv_kernel `mma_transposed<T, X3>(dk, q_lds, .., dp)`
                     dQ = scale x three terms of dS k (dS, k split)    attn_bwd_dq_kernel `mma_transposed<T, X3>(dq, k_lds, .., dp)`
lse is held to attention_cases.LSE_ABS, or -- where the model's own lse is further than half of that from the reference (the spike rows, whose one
dominating score carries the split error of a 384-unit dot product) -- to twice the model's distance, as attention_cases does for the
persistent form.

No silent fallback: every case also runs the same call on plain fp32 operands (the result must differ: the dispatch calls the exact kernel
"a superset" and would take it without a word) and on plain bf16 operands (which must sit at least 10 x outside the gate).  Shapes the
dispatch documents as exact fp32 (gemm256.hip gemm_nt256_try, tn256_plan) are gated with kernel_cases.gemm_ref64 + close32 instead
(case_nt_fallback, case_tn_fallback).

Measured kernel / model ratios (worst tensor of the case: E_rms ratio, E_max ratio); the gate is 1.25 / 2.0:
  emulator   NT (549, 256, 64), none + bias / residual                                  1.001  1.025
             TN (144, 256, 256), gemm_variant = 4                                        1.001  1.003
             attention forward (1, 64) / (2, 70), both forms                             1.003  0.988 / 1.003  1.014
             attention backward (2, 70), both feeds                                      1.003  1.018
  MI355X     NT (549, 256, 32 / 64 / 96 / 160)                                           1.000  1.001 / 1.000  1.006 / 1.000  0.998 / 1.000  1.004
             NT (562, 768, 3072) / (843, 768, 768) / (1120, 2304, 768)                   1.009  0.984 / 1.002  1.001 / 1.002  1.002
             NT (22172, 768, 64), the two-launch tail                                    1.000  1.000
             NT (843, 768, 768) + mul, gemm_epilogue 0 / 1, gemm_tail 2 (each)           1.002  1.001
             NT (843, 768, 768) gelu + aux_out, against the propagated bound             0.625  0.827
             NT row-dot (562, 768, 768)                                                  1.002  1.001
             NT over 3 K (843, 2304, 3 x 768) / (843, 768, 3 x 768) residual             1.004  0.983 / 1.004  1.018
             NT over 3 K (843, 3072, 3 x 768) gelu, fp32 and split rows                  0.718  0.957
             NT over 3 K (843, 768, 3 x 3072) residual / (150, 768, 3 x 768)             1.015  1.009 / 1.004  1.015
             TN (128 / 144 / 304, 768, 768)                                              1.000  1.001 / 1.000  0.999 / 1.001  1.002
             TN (1120, 2304, 768) / (4496, 768, 3072)                                    1.003  1.003 / 1.014  1.030
             TN (304, 768, 768) lda + 64 / tn_reduce = 1 / deterministic = 1             1.001  1.017 / 1.000  1.002 / 1.000  1.002
             attention forward (1, 64) / (1, 128) / (2, 129) / (3, 281)                  1.002  0.991 / 1.002  1.007 / 1.001  1.027 / 1.001  1.006
             attention forward (2, 320) / (2, 321) / (1, 875) / (1, 1685)                1.001  1.014 / 1.001  1.087 / 1.002  1.083 / 1.003  1.018
             attention forward, spike (1, 290) / (2, 560)                                1.001  0.997 / 1.002  0.997
             attention forward, q_rows = 2 (3, 281) / (2, 321)                           1.000  1.003 / 0.999  1.028
             attention backward (1, 64) / (2, 129) / (3, 281) / (2, 321) / (1, 875)      1.003  1.007 / 1.003  1.026 / 1.002  1.013 / 1.002  1.018 / 1.003  1.036
             attention backward, spike (1, 290)                                          1.015  1.066
The guarded cases repeat (549, 256, 96), (843, 768, 768), TN lda + 64 and the (2, 321) pair with the same figures.  The GELU epilogue of the
split kernel is also held to the model passed through gelu / gelu' themselves (gelu_through): 1.001 / 1.022 under the emulator at (549, 256, 64).
"""
import math

import numpy as np
import torch

from maest_amd import _lib, ops
from tests import kernel_cases as KC
from tests.attention_cases import E, H, LN2, LOG2E, LSE_ABS, MAX_MARGIN, RMS_MARGIN, _f32mul, _heads, _rows, errors, reference
from tests.kernel_cases import close32, gemm_ref64, lp, rnd

SCALE = 0.125


# ------------------------------------------------------------------------------------------------ the split and its product
def bf(t):
    """fp64 -> bf16 (through fp32, as the kernels convert), round to nearest even, as fp64."""
    return t.float().bfloat16().double()


def bf_trunc(t):
    """fp64 -> bf16 by dropping the low 16 bits of the fp32 value (a defect: never what a kernel may do)."""
    return (t.float().view(torch.int32) & -65536).view(torch.float32).double()


def split(x, rd_hi=bf, rd_lo=bf):
    """x (fp64 values of fp32 numbers) -> hi = bf(x), lo = bf(x - hi); x - hi is exact in fp32 (common.h split_bf16x8)."""
    hi = rd_hi(x)
    return hi, rd_lo(x - hi)


def terms3(ah, al, bh, bl):
    """sum_k lo_a hi_b + hi_a lo_b + hi_a hi_b of the pieces a [.., M, K], b [.., N, K] (hi_b + lo_b is exact in fp64: two matrix products)."""
    return ah @ (bh + bl).transpose(-2, -1) + al @ bh.transpose(-2, -1)


def prod3(a, b, sa=split, sb=split):
    """The split product of a [.., M, K] and b [.., N, K] (fp64 values of the fp32 operands) -> [.., M, N]."""
    return terms3(*sa(a), *sb(b))


def gate(what, got, model, ref, ratios=None):
    """Require E_rms(got) <= RMS_MARGIN E_rms(model) and E_max(got) <= MAX_MARGIN E_max(model); print and record the two ratios."""
    got = got.detach().cpu().double()
    KC.note(what, got, lambda: ref)
    (gr, gm), (mr, mm) = errors(got, ref), errors(model, ref)
    assert mr > 0 and mm > 0, f"{what}: the model shows no rounding error: nothing to compare with"
    print(f"  {what}: E_rms {gr:.3e} = {gr / mr:.3f} x model ({mr:.3e}), E_max {gm:.3e} = {gm / mm:.3f} x model ({mm:.3e})")
    if ratios is not None:
        ratios[what] = (gr / mr, gm / mm)
    assert gr <= RMS_MARGIN * mr, f"{what}: rms error {gr:.3e} is {gr / mr:.2f} x what the roundings allow ({mr:.3e})"
    assert gm <= MAX_MARGIN * mm, f"{what}: max error {gm:.3e} is {gm / mm:.2f} x what the roundings allow ({mm:.3e})"


def controls(what, got, plain32, plain16, model, ref):
    """No silent fallback: the same call on plain fp32 operands gives another result, and on plain bf16 operands one at least 10 x outside
    the gate (the `e16 > 10 * e` idea of kernel_cases.case_split_precision)."""
    assert got.dtype == torch.float32 and plain32.dtype == torch.float32
    assert not torch.equal(got.detach().cpu(), plain32.detach().cpu()), \
        f"{what}: bit-equal to the call on plain fp32 operands: the exact fp32 kernel served it, not the split one"
    (er, em), (mr, mm) = errors(KC.f32(plain16.detach()).cpu().double(), ref), errors(model, ref)
    assert er >= 10 * RMS_MARGIN * mr and em >= 10 * MAX_MARGIN * mm, \
        f"{what}: plain bf16 operands ({er:.2e} rms, {em:.2e} max) are not 10 x outside the gate ({RMS_MARGIN * mr:.2e}, {MAX_MARGIN * mm:.2e})"


def summary(case, ratios):
    """Print (one line, for the table of this module's docstring) and return the worst ratios of a case."""
    worst = (max(r for r, _ in ratios.values()), max(m for _, m in ratios.values()))
    print(f"SPLIT-RATIO | {'emulator' if _lib.host_emulation() else 'device'} | {case} | {worst[0]:.3f} | {worst[1]:.3f}")
    return worst


# ------------------------------------------------------------------------------------------------ dispatch, restated
def nt_takes_split(M, N, K):
    """gemm256.hip gemm_nt256_try for fp32 operands under the options in force."""
    return M >= max(512, ops.get_option("gemm_min_m")) and N >= 256 and N % 256 == 0 and K % 32 == 0


def tn_takes_split(M, N, K):
    """gemm256.hip tn256_plan for fp32 operands under the options in force."""
    return (M % 256 == 0 and N % 256 == 0 and K % 16 == 0 and K >= 128 and (M * N >= 8 * 65536 or ops.get_option("gemm_variant") == 4))


# ------------------------------------------------------------------------------------------------ NT GEMM
_nt_cache = {}


def lp16(t):
    """fp32 [rows, K] -> the plain bf16 operand of the control call, K padded with zero columns to the 64 the bf16 kernels ask for (the same product)."""
    pad = -t.shape[1] % 64
    return lp(torch.cat([t, torch.zeros(t.shape[0], pad)], 1) if pad else t).contiguous()


def nt_data(M, N, K, wscale=1.0):
    """Operands, the fp64 accumulator a b^T and its model, made once per shape (the last shape is kept)."""
    key = (M, N, K, wscale)
    if key not in _nt_cache:
        _nt_cache.clear()
        a, b = rnd((M, K), 50), rnd((N, K), 51, wscale)
        a64, b64 = a.double(), b.double()
        _nt_cache[key] = dict(a=a, b=b, bias=rnd((N,), 52), res=rnd((M, N), 53), pre=rnd((M, N), 54), racc=a64 @ b64.t(), macc=prod3(a64, b64))
    return _nt_cache[key]


def _nt_forms(d):
    """name -> (gemm_nt keywords, the epilogue in fp64)"""
    bias, res, pre = d["bias"].double(), d["res"].double(), d["pre"].double()
    return {"none + bias": (dict(), lambda x: x + bias),
            "residual": (dict(epi=ops.EPI_RESIDUAL, aux_in=d["res"]), lambda x: x + bias + res),
            "mul": (dict(epi=ops.EPI_MUL, aux_in=d["pre"]), lambda x: (x + bias) * pre)}


def case_nt(dev, M, N, K, epis=("none + bias", "residual"), what=None):
    """gemm_nt256w_kernel<float, .., true> at [M, N, K] under the options in force, each epilogue of `epis` through gate() and controls()."""
    assert nt_takes_split(M, N, K), f"({M}, {N}, {K}) does not reach the split kernel under the options in force"
    d = nt_data(M, N, K)
    a, b, bias = d["a"].to(dev), d["b"].to(dev), d["bias"].to(dev)
    a16, b16 = lp16(d["a"]).to(dev), lp16(d["b"]).to(dev)
    what = what or f"NT ({M}, {N}, {K})"
    ratios = {}
    forms = _nt_forms(d)
    for name in epis:
        kw, post = forms[name]
        kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
        ref, model = post(d["racc"]), post(d["macc"])
        c = ops.gemm_nt(a, b, bias, out_dtype=torch.float32, x3=True, **kw)
        gate(f"{what}, {name}", c, model, ref, ratios)
        c32 = ops.gemm_nt(a, b, bias, out_dtype=torch.float32, **kw)
        c16 = ops.gemm_nt(a16, b16, bias, out_dtype=torch.float32, **kw)
        controls(f"{what}, {name}", c, c32, c16, model, ref)
    return summary(what, ratios)


def gelu_models(racc, macc, bias):
    """GELU and GELU' of the reference accumulator, and the model error propagated through them by their largest slopes (max |gelu'| = 1.13,
    max |gelu''| = 0.80: kernel_cases.gate_gelu)."""
    from tests import epilogue_cases as EC
    g, dg = EC.gelu_ref(racc + bias)
    return g, dg, g + 1.13 * (macc - racc), dg + 0.80 * (macc - racc)


def gelu_through(macc, bias):
    """GELU and GELU' of the MODEL accumulator: the tighter companion of gelu_models (the slopes at the arguments themselves, not their maxima;
    the epilogue's own fp32 / libm arithmetic, epilogue_cases.deltas at E_fit = 0, is 2 % of the split's error)."""
    from tests import epilogue_cases as EC
    return EC.gelu_ref(macc + bias)


def case_nt_gelu(dev, M, N, K):
    """The GELU epilogue with its fp32 side output (aux_out = gelu'), weights scaled by 1 / sqrt(K) so that the arguments fall where the
    function bends."""
    assert nt_takes_split(M, N, K)
    d = nt_data(M, N, K, wscale=K ** -0.5)
    a, b, bias = d["a"].to(dev), d["b"].to(dev), d["bias"].to(dev)
    g, dg, mg, mdg = gelu_models(d["racc"], d["macc"], d["bias"].double())
    what, ratios = f"NT ({M}, {N}, {K}), gelu + aux_out", {}
    aux = torch.empty((M, N), dtype=torch.float32, device=dev)
    c = ops.gemm_nt(a, b, bias, out_dtype=torch.float32, epi=ops.EPI_GELU, aux_out=aux, x3=True)
    gate(f"{what}: gelu", c, mg, g, ratios)
    gate(f"{what}: gelu'", aux, mdg, dg, ratios)
    tg, tdg = gelu_through(d["macc"], d["bias"].double())
    gate(f"{what}: gelu against the model through gelu itself", c, tg, g, ratios)
    gate(f"{what}: gelu' against the model through gelu' itself", aux, tdg, dg, ratios)
    aux32 = torch.empty((M, N), dtype=torch.float32, device=dev)
    c32 = ops.gemm_nt(a, b, bias, out_dtype=torch.float32, epi=ops.EPI_GELU, aux_out=aux32)
    c16 = ops.gemm_nt(lp16(d["a"]).to(dev), lp16(d["b"]).to(dev), bias, out_dtype=torch.float32, epi=ops.EPI_GELU)
    controls(what, c, c32, c16, mg, g)
    return summary(what, ratios)


def case_nt_rowdot(dev, M, N, K, rows_per_item):
    """maest_gemm_nt_rowdot on split products: C through gate(), the row-dot side output against the products of the stored C itself (the
    values the kernel multiplied: kernel_cases.case_gemm_rowdot)."""
    assert nt_takes_split(M, N, K) and N % 256 == 0
    d = nt_data(M, N, K)
    a, b, bias, other = d["a"].to(dev), d["b"].to(dev), d["bias"].to(dev), d["pre"].to(dev)
    ref, model = d["racc"] + d["bias"].double(), d["macc"] + d["bias"].double()
    what, ratios = f"NT row-dot ({M}, {N}, {K})", {}
    c, rd = ops.gemm_nt_rowdot(a, b, other, rows_per_item, out_dtype=torch.float32, bias=bias, x3=True)
    gate(f"{what}: C", c, model, ref, ratios)
    c32, _ = ops.gemm_nt_rowdot(a, b, other, rows_per_item, out_dtype=torch.float32, bias=bias)
    c16, _ = ops.gemm_nt_rowdot(lp16(d["a"]).to(dev), lp16(d["b"]).to(dev), other, rows_per_item, out_dtype=torch.float32, bias=bias)
    controls(what, c, c32, c16, model, ref)
    assert rd.shape == (M // rows_per_item, N // 64, rows_per_item)
    want = (c.cpu().double() * d["pre"].double()).reshape(M // rows_per_item, rows_per_item, N // 64, 64)
    mag = want.abs().sum(-1).permute(0, 2, 1)
    close32(rd.cpu(), want.sum(-1).permute(0, 2, 1), 2 * 65 * 2.0 ** -24 * mag, f"{what}: per-(row, group) dot products")
    return summary(what, ratios)


def case_nt_fallback(dev, M, N, K):
    """A shape the dispatch documents as exact fp32 (gemm_nt256_try returns -1): x3 = True must give the fp32 kernel's accuracy."""
    assert not nt_takes_split(M, N, K), f"({M}, {N}, {K}) reaches the split kernel: not a fall-back shape"
    a, b, bias = rnd((M, K), 50), rnd((N, K), 51), rnd((N,), 52)
    c = ops.gemm_nt(a.to(dev), b.to(dev), bias.to(dev), out_dtype=torch.float32, x3=True)
    ref, dacc = gemm_ref64(a, b, bias)
    return close32(c.cpu(), ref, dacc, f"NT ({M}, {N}, {K}): exact fp32 fall-back of the split call")


# ------------------------------------------------------------------------------------------------ one bf16 GEMM over 3 K
def split3_rows(x):
    """fp32 [M, K] -> the bf16 [M, 3 K] rows [hi | hi | lo] the LayerNorm / attention / GELU kernels write (MAEST_SPLIT3_A)."""
    h = x.bfloat16()
    return torch.cat([h, h, (x - h.float()).bfloat16()], 1).contiguous()


def case_nt_over_3k(dev, M, N, K, epi="none", split_out=False):
    """MAEST_SPLIT3_A rows x cast_weights_multi(.., ops.SPLIT3) rows through the bf16 kernels, K = 3 x the logical depth.  epi: "none",
    "residual" or "gelu" (weights scaled by 1 / sqrt(K)); split_out: the GELU result once more as MAEST_SPLIT3_A rows."""
    d = nt_data(M, N, K, wscale=K ** -0.5 if epi == "gelu" else 1.0)
    bias = d["bias"].to(dev)
    a3 = split3_rows(d["a"]).to(dev)
    b3 = ops.cast_weights_multi([d["b"].to(dev)], ops.SPLIT3)[0][0]
    bh = d["b"].bfloat16()
    assert torch.equal(b3.cpu(), torch.cat([bh, (d["b"] - bh.float()).bfloat16(), bh], 1)), "split3 weight rows"
    what, ratios = f"NT over 3 K ({M}, {N}, 3 x {K}), {epi}", {}
    b64 = d["bias"].double()
    if epi == "gelu":
        ref, _, model, _ = gelu_models(d["racc"], d["macc"], b64)
        kw = dict(epi=ops.EPI_GELU)
    elif epi == "residual":
        ref, model = d["racc"] + b64 + d["res"].double(), d["macc"] + b64 + d["res"].double()
        kw = dict(epi=ops.EPI_RESIDUAL, aux_in=d["res"].to(dev))
    else:
        ref, model = d["racc"] + b64, d["macc"] + b64
        kw = {}
    c = ops.gemm_nt(a3, b3, bias, out_dtype=torch.float32, split3=True, **kw)
    gate(what, c, model, ref, ratios)
    c32 = ops.gemm_nt(d["a"].to(dev), d["b"].to(dev), bias, out_dtype=torch.float32, **kw)
    c16 = ops.gemm_nt(lp16(d["a"]).to(dev), lp16(d["b"]).to(dev), bias, out_dtype=torch.float32, **kw)
    controls(what, c, c32, c16, model, ref)
    if split_out:
        g3 = ops.gemm_nt(a3, b3, bias, out_dtype=ops.SPLIT3, epi=ops.EPI_GELU, split3=True).cpu()
        assert g3.shape == (M, 3 * N) and torch.equal(g3[:, :N].view(torch.int16), g3[:, N:2 * N].view(torch.int16)), f"{what}: the two hi thirds differ"
        if ops.gemm_split3_out_fast(M, N, 3 * K):      # both outputs left the same main loop and epilogue arithmetic: the split of the very fp32 values
            assert torch.equal(g3.view(torch.int16), split3_rows(c.cpu()).view(torch.int16)), f"{what}: the split rows are not the split of the fp32 output"
        mh, ml = split(model)                          # hi + lo of a row: the model's value split the same way
        gate(f"{what}: hi + lo of the split rows", g3[:, :N].double() + g3[:, 2 * N:].double(), mh + ml, ref, ratios)
    return summary(what, ratios)


# ------------------------------------------------------------------------------------------------ TN GEMM
_tn_cache = {}


def tn_data(K, M, N, lda_pad=0):
    key = (K, M, N, lda_pad)
    if key not in _tn_cache:
        _tn_cache.clear()
        a_full, b = rnd((K, M + lda_pad), 60), rnd((K, N), 61)
        a64, b64 = a_full[:, :M].double(), b.double()
        _tn_cache[key] = dict(a_full=a_full, b=b, ref=a64.t() @ b64, model=prod3(a64.t().contiguous(), b64.t().contiguous()),
                              cs=a64.sum(0), cs_delta=2 * (K + 1) * 2.0 ** -24 * a64.abs().sum(0))
    return _tn_cache[key]


def case_tn(dev, K, M, N, splits=(1, 3, 0), lda_pad=0, workspace=False, what=None):
    """gemm_tn256_kernel<float, true> at [K, M, N] under the options in force: out and colsum for every split_k of `splits`.
    workspace: the options in force combine the partials through the workspace (tn_reduce = 1, deterministic = 1): two calls bit-equal,
    and a second call into the same `out` accumulates."""
    assert tn_takes_split(M, N, K), f"({K}, {M}, {N}) does not reach the split kernel under the options in force"
    d = tn_data(K, M, N, lda_pad)
    a = d["a_full"].to(dev)[:, :M]
    b = d["b"].to(dev)
    what = what or f"TN ({K}, {M}, {N})" + (f", lda + {lda_pad}" if lda_pad else "")
    ratios = {}
    zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    c32 = ops.gemm_tn(a, b, zeros(M, N), split_k=0, M=M, N=N)
    c16 = ops.gemm_tn(lp(d["a_full"]).to(dev)[:, :M], lp(d["b"]).to(dev), zeros(M, N), split_k=0, M=M, N=N)
    for sk in splits:
        out, cs = zeros(M, N), zeros(M)
        ops.gemm_tn(a, b, out, colsum=cs, split_k=sk, M=M, N=N, x3=True)
        gate(f"{what}, split_k = {sk}", out, d["model"], d["ref"], ratios)
        controls(f"{what}, split_k = {sk}", out, c32, c16, d["model"], d["ref"])
        close32(cs.cpu(), d["cs"], d["cs_delta"], f"{what}, split_k = {sk}: colsum (an fp32 sum of the unsplit operand)")
        if workspace and ops.gemm_tn_workspace_bytes(torch.float32, M, N, K, sk, x3=True) > 0:
            out2, cs2 = zeros(M, N), zeros(M)
            ops.gemm_tn(a, b, out2, colsum=cs2, split_k=sk, M=M, N=N, x3=True)
            assert torch.equal(out, out2), f"{what}, split_k = {sk}: two calls through the workspace differ"
            if ops.get_option("deterministic") != 0:
                assert torch.equal(cs, cs2), f"{what}, split_k = {sk}: colsum of two ordered calls differs"
            ops.gemm_tn(a, b, out2, split_k=sk, M=M, N=N, x3=True)            # the second call accumulates
            gate(f"{what}, split_k = {sk}: a second call into the same C", out2, 2 * d["model"], 2 * d["ref"], ratios)
    return summary(what, ratios)


def case_tn_fallback(dev, K, M, N, split_k=0):
    """A shape (or, under deterministic = 1, a single split) that tn256_plan / gemm_tn256_try leave to the exact fp32 kernel."""
    a, b = rnd((K, M), 60), rnd((K, N), 61)
    out = torch.zeros((M, N), dtype=torch.float32, device=dev)
    ops.gemm_tn(a.to(dev), b.to(dev), out, split_k=split_k, x3=True)
    ref, dacc = gemm_ref64(a.t().contiguous(), b.t().contiguous(), None)
    return close32(out.cpu(), ref, dacc, f"TN ({K}, {M}, {N}): exact fp32 fall-back of the split call")


# ------------------------------------------------------------------------------------------------ attention
def _head_chunk(N):
    return max(1, min(H, (H * 600 * 600) // (N * N)))


def reference_fwd(x, N, scale):
    """fp64 softmax attention of ONE clip, forward only, a few heads at a time (N = 1685: 23 MB per head and tensor).  -> out [N, 768], lse [12, N]"""
    q, k, v = _heads(x, N)
    outs, lses, hc = [], [], _head_chunk(N)
    for h0 in range(0, H, hc):
        s = (q[h0:h0 + hc] @ k[h0:h0 + hc].transpose(-2, -1)) * scale
        outs.append(s.softmax(-1) @ v[h0:h0 + hc])
        lses.append(torch.logsumexp(s, -1))
    return _rows(torch.cat(outs), N), torch.cat(lses)


def model_fwd(x, N, scale, split_qk=split, split_p=split, split_v=split, split_v_last=None):
    """The forward pipeline of ONE clip in fp64 with the roundings of attn_fwd_x3s_kernel / attn_fwd_kernel<float, true>: x [N, 2304] fp64 = the
    fp32 operand.  -> out [N, 768], lse [12, N].  split_p / split_v_last: the split of P / of the V rows of the last key tile (tests of the gate)."""
    q, k, v = _heads(x, N)
    c2 = _f32mul(scale, LOG2E)
    nt = (N + 63) // 64
    outs, lses, hc = [], [], _head_chunk(N)
    for h0 in range(0, H, hc):
        qq, kk, vv = q[h0:h0 + hc], k[h0:h0 + hc], v[h0:h0 + hc]
        n = qq.shape[0]
        s2 = prod3(qq, kk, split_qk, split_qk) * c2
        st = torch.cat([s2, torch.full((n, N, nt * 64 - N), -math.inf, dtype=torch.float64)], -1).reshape(n, N, nt, 64)
        mrun = torch.cummax(st.amax(-1), -1).values                  # [n, N, nt]
        mfin = mrun[..., -1]
        p = torch.exp2(st - mrun[..., None])                         # against the maximum known when the tile is processed
        w = torch.exp2(mrun - mfin[..., None])[..., None]            # the rescaling that follows: factors of the fp32 state
        l = (p * w).reshape(n, N, -1).sum(-1)                        # the unsplit probabilities
        ph, pl = split_p(p)
        vh, vl = split_v(vv)
        if split_v_last is not None:
            k0 = (nt - 1) * 64
            lh, ll = split_v_last(vv[:, k0:])
            vh, vl = torch.cat([vh[:, :k0], lh], 1), torch.cat([vl[:, :k0], ll], 1)
        phw, plw = (ph * w).reshape(n, N, -1)[..., :N], (pl * w).reshape(n, N, -1)[..., :N]
        outs.append((phw @ (vh + vl) + plw @ vh) / l[..., None])
        lses.append((mfin + torch.log2(l)) * LN2)
    return _rows(torch.cat(outs), N), torch.cat(lses)


def model_bwd(x, out, lse, dout, N, scale, sp=split):
    """The backward pipeline of ONE clip in fp64 with the roundings of attn_bwd_dkdv_kernel<float, true> / attn_bwd_dq_kernel<float, true>, on the
    out / lse it is handed (fp64 values of the fp32 tensors the kernels read).  -> dqkv [N, 2304]"""
    q, k, v = _heads(x, N)
    do, o = _heads(dout, N)[0], _heads(out, N)[0]
    c2 = _f32mul(scale, LOG2E)
    delta = (do * o).sum(-1)
    p = torch.exp2(prod3(q, k, sp, sp) * c2 - (lse * LOG2E)[..., None])
    ds = p * (prod3(do, v, sp, sp) - delta[..., None])
    tr = lambda t: t.transpose(-2, -1).contiguous()
    dv = prod3(tr(p), tr(do), sp, sp)
    dk = prod3(tr(ds), tr(q), sp, sp) * scale
    dq = prod3(ds, tr(k), sp, sp) * scale
    return torch.cat([_rows(dq, N), _rows(dk, N), _rows(dv, N)], 1)


_attn_cache = {}


def attn_data(B, N, spike=False, backward=False, seed=70):
    """qkv, dout, and per clip the fp64 reference (with autograd where `backward`) and the forward model, made once per shape."""
    key = (B, N, spike)
    d = _attn_cache.get(key)
    if d is None or (backward and d["ref_g"] is None):
        _attn_cache.clear()
        qkv = rnd((B * N, 2304), seed)
        if spike:      # a large jump of the running maximum at a late key tile (the online-softmax rescale): kernel_cases.case_attention
            qkv[min(N - 1, 70), 768:768 + 64] = qkv[3, 0:64] * 6.0
        dout = rnd((B * N, E), seed + 1)
        x, g = qkv.double(), dout.double()
        ro, rl, rg, mo, ml = [], [], [], [], []
        for c in range(B):
            xc = x[c * N:(c + 1) * N]
            if backward:
                o, l, gr = reference(xc, g[c * N:(c + 1) * N], N, SCALE)
                rg.append(gr)
            else:
                o, l = reference_fwd(xc, N, SCALE)
            m = model_fwd(xc, N, SCALE)
            ro.append(o), rl.append(l), mo.append(m[0]), ml.append(m[1])
        d = dict(qkv=qkv, dout=dout, ref_out=torch.cat(ro), ref_lse=torch.stack(rl), ref_g=torch.cat(rg) if backward else None,
                 model_out=torch.cat(mo), model_lse=torch.stack(ml))
        _attn_cache[key] = d
    return d


def _lse_limit(d, rows=None):
    sl = slice(None) if rows is None else slice(0, rows)
    me = float((d["model_lse"][..., sl] - d["ref_lse"][..., sl]).abs().max())
    return LSE_ABS if 2 * me <= LSE_ABS else 2 * me


FWD_FORMS = (("split tiles", {}), ("per-use split", {"attn_fwd": 1}))


def case_attn_fwd(dev, B, N, spike=False, forms=FWD_FORMS, head_rows=False):
    """attn_fwd_x3s_kernel (the default) and attn_fwd_kernel<float, true> (attn_fwd = 1) at [B, N]: out through gate() and controls(), lse, and
    out_split3 bit-equal to the split of the fp32 result.  head_rows: the head-row pass instead (q_rows = 2, attn_fwd_kernel<float, true>): the
    written 32-row tile of every clip."""
    d = attn_data(B, N, spike)
    qkv = d["qkv"].to(dev)
    what = f"attention forward ({B}, {N})" + (", spike" if spike else "") + (", q_rows = 2" if head_rows else "")
    nv = min(32, N) if head_rows else N
    kq = {"q_rows": 2} if head_rows else {}
    rows = lambda t: t.detach().cpu().double().reshape(B, N, -1)[:, :nv]
    ref, model = rows(d["ref_out"]), rows(d["model_out"])
    ratios = {}
    o32 = ops.attn_fwd(qkv, B, N, SCALE, **kq)
    o16 = KC.f32(ops.attn_fwd(lp(d["qkv"]).to(dev), B, N, SCALE, **kq))
    lim = _lse_limit(d, nv)
    for name, opt in (forms if not head_rows else (("head rows", {}),)):
        with ops.options(**opt):
            out, lse = ops.attn_fwd(qkv, B, N, SCALE, save_lse=True, x3=True, **kq)
            gate(f"{what}, {name}: out", rows(out), model, ref, ratios)
            controls(f"{what}, {name}", rows(out).float(), rows(o32).float(), rows(o16), model, ref)
            el = float((lse.cpu().double()[..., :nv] - d["ref_lse"][..., :nv]).abs().max())
            print(f"  {what}, {name}: lse within {el:.2e} of the reference (limit {lim:.2e})")
            assert el <= lim, f"{what}, {name}: lse {el:.3e} from the reference, limit {lim:.3e}"
            if not head_rows:
                o3 = ops.attn_fwd(qkv, B, N, SCALE, x3=True, out_split3=True).cpu()
                assert torch.equal(o3.view(torch.int16), split3_rows(out.cpu()).view(torch.int16)), f"{what}, {name}: out_split3 rows are not the split of the fp32 result"
    return summary(what, ratios)


def case_attn_bwd(dev, B, N, spike=False):
    """attn_bwd_dkdv_kernel<float, true> / attn_bwd_dq_kernel<float, true> at [B, N]: dQ, dK, dV gated separately, once on the reference's out / lse
    (rounded to fp32) and once on the split forward's own."""
    d = attn_data(B, N, spike, backward=True)
    qkv, dout = d["qkv"].to(dev), d["dout"].to(dev)
    what = f"attention backward ({B}, {N})" + (", spike" if spike else "")
    x, g = d["qkv"].double(), d["dout"].double()
    ratios = {}
    fed = {"the reference": (d["ref_out"].float().to(dev), d["ref_lse"].float().contiguous().to(dev)),
           "the split forward": ops.attn_fwd(qkv, B, N, SCALE, save_lse=True, x3=True)}
    for src, (o, l) in fed.items():
        o64, l64 = o.cpu().double(), l.cpu().double()
        model = torch.cat([model_bwd(x[c * N:(c + 1) * N], o64[c * N:(c + 1) * N], l64[c], g[c * N:(c + 1) * N], N, SCALE) for c in range(B)])
        dqkv = ops.attn_bwd(qkv, o, dout, l, B, N, SCALE, x3=True)
        if src == "the reference":      # (the plain calls once: the second feed runs the same kernels on the same shape)
            d32 = ops.attn_bwd(qkv, o, dout, l, B, N, SCALE)
            d16 = KC.f32(ops.attn_bwd(lp(d["qkv"]).to(dev), lp(o.cpu()).to(dev), lp(d["dout"]).to(dev), l, B, N, SCALE))
        for name, sl in (("dQ", slice(0, E)), ("dK", slice(E, 2 * E)), ("dV", slice(2 * E, 3 * E))):
            gate(f"{what} on the out / lse of {src}: {name}", dqkv[:, sl], model[:, sl], d["ref_g"][:, sl], ratios)
            if src == "the reference":
                controls(f"{what}: {name}", dqkv[:, sl], d32[:, sl], d16[:, sl], model[:, sl], d["ref_g"][:, sl])
    return summary(what, ratios)
