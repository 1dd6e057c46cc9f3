"""The GEMM epilogues on accumulators that are known exactly, shared by the emulator tests, the GPU tests and
tests/test_epilogue_gate_cpu.py (which feeds the same gates a torch restatement of the epilogue, and that restatement with defects).

Operands, in the manner of kernel_cases.case_half_conversions: a[:, 0] = x16[m], a[:, 1] = 1, b[:, 0] = 1, b[:, 1] = c16[n], zero elsewhere, so
that acc[m, n] = x16[m] + c16[n] -- x16 on the 1/16 grid over [-12, 12] (exact in bf16 and in half) followed by +-0, +-16, +-100 and +- the
largest finite value of the build's format, c16[n] = (n % 256) / 4096 (8-bit values): the sums fit 16 significand bits, every fp32 partial
sum is exact in any order, and the 385 x 256 arguments fill the 1/4096 grid over [-12, 12 + 1/16).  A second pass has c16 = 0 and the fp32
bias[n] = (n % 256) / 4096 + 2^-14: the epilogue's acc + bias, exact too, reaches arguments off the 16-bit grid.

GELU gate (case_gelu_grid), against x Phi(x) and Phi(x) + x phi(x) in fp64.  Every constant is derived from the bounds the source documents:
    E        = E_fit + 12 * 2^-24      E_fit: the erf fit's documented bound -- 1.71e-6 for gelu_pair2<false> (four terms), 1.5e-7 for gelu_pair<false>
                                       (Abramowitz-Stegun 7.1.26), 0 for libm; 12 ulp: the ~10 fp32 operations and the two 1-ulp transcendentals
                                       behind the fit, each with sensitivity <= 1 on a quantity <= 1
    delta_g  = |x| E / 2 + 2^-24 |g|   (g = x cdf, cdf = (1 + erf) / 2; the final multiply)
    delta_dg = E / 2 + 2^-21           (the relative error of pdf times |x| pdf <= 0.25, and the final fma)
fp32 outputs: kernel_cases.close32; 16-bit outputs: kernel_cases.close16; MAEST_SPLIT3_A rows [ hi | hi | lo ]: hi + lo within delta_g + 2^-16 |g|,
the two hi thirds equal.  No element is left out of any gate.
"""
import math

import torch

from maest_amd import _lib, ops
from tests.kernel_cases import _bits_equal, close16, close32, f16_build, f32, lp, rnd

FORMS_ALL = ({"gemm_min_m": 1 << 30}, {"gemm_min_m": 512}, {"gemm_min_m": 512, "gemm_variant": 3}, {"gemm_min_m": 512, "gemm_tail": 2})
E_FIT4, E_FIT5 = 1.71e-6, 1.5e-7          # common.h: gelu_pair2<false>, gelu_pair<false>
ULP = 2.0 ** -24                          # half an fp32 ulp of 1 = the relative error of one fp32 rounding
N_GRID = 385                              # rows on the 1/16 grid


def e_fit(kw, dtype, out):
    """The documented bound of the erf form that serves ops.options(**kw) for operands of `dtype` and the output `out` ("f32", "16", "pair",
    "split3"), as the dispatch of gemm.hip (maest_gemm_nt) and gemm256.hip (gemm_nt256_try) reads: fp32 operands keep libm (EXACT) in every
    kernel; 16-bit operands run gelu_pair<false> in the 128 x 128 kernel (gemm.hip: epi_stage / epi_scalar) and gelu_pair2<false> in the
    256-row-tile kernels (gemm256.hip, gemm256_epi.h: stage256 / stage256_pair / stageT; gemm_nt_ow.hip: stage_blk).  Split rows exist in the
    one-wave-per-SIMD kernel's epilogue only: every other form writes them from the 128 x 128 kernel's element-wise epilogue."""
    if dtype == torch.float32:
        return 0.0
    if kw.get("gemm_min_m", 0) > 512:
        return E_FIT5
    if out == "split3":
        return E_FIT4 if kw.get("gemm_variant", 0) == 0 and bool(_lib.kernel_forms() & _lib.FORM_GEMM_NT_OW) else E_FIT5
    return E_FIT4


def row_values(M, largest=True):
    """x16[m]: (m - 192) / 16 for m < 385, then +-0, +-16, +-100 and (`largest`) +- the largest finite value of the build's format; +0 beyond."""
    big = (65504.0 if f16_build() else (2.0 - 2.0 ** -7) * 2.0 ** 127) if largest else 256.0
    x = torch.zeros(M, dtype=torch.float64)
    x[:N_GRID] = (torch.arange(N_GRID, dtype=torch.float64) - 192) / 16
    tail = torch.tensor([0.0, -0.0, 16.0, -16.0, 100.0, -100.0, big, -big], dtype=torch.float64)
    x[N_GRID:N_GRID + len(tail)] = tail
    return x


def operands(M, N, K, dtype, second, largest=True):
    """-> a [M, K], b [N, K] in `dtype` (16-bit: the build's container), bias (fp32 [N]; None in the first pass) and the fp64 argument
    x[m, n] = acc + bias of the GELU."""
    assert M >= N_GRID + 8 and K >= 2
    x = row_values(M, largest)
    c = (torch.arange(N) % 256).double() / 4096
    a, b = torch.zeros(M, K), torch.zeros(N, K)
    a[:, 0], a[:, 1], b[:, 0] = x.float(), 1.0, 1.0
    bias = None
    if second:
        bias = (c + 2.0 ** -14).float()
        c = bias.double()
    else:
        b[:, 1] = c.float()
    assert torch.equal(f32(lp(a, dtype)), a) and torch.equal(f32(lp(b, dtype)), b), "the operand values must be exact in the operand format"
    return lp(a, dtype), lp(b, dtype), bias, x[:, None] + c[None, :]


def gelu_ref(x):
    """fp64: x Phi(x), Phi(x) + x phi(x)."""
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * cdf, cdf + x * pdf


def deltas(x, g, fit):
    E = fit + 12 * ULP
    return x.abs() * E / 2 + ULP * g.abs(), torch.full_like(x, E / 2 + 2.0 ** -21), E


def check_gelu(outs, x, fit, what):
    """The gates of section 2 on the outputs of ONE kernel form for the fp64 arguments `x`; outs: {"f32": gelu -> fp32, "16": gelu -> 16-bit,
    "pair": (value, aux) in the kernel's output type, "split3": [M, 3 N] rows} (any subset).  `fit`: E_fit, or {output: E_fit}.
    Returns {output: worst err / delta}."""
    g, dg = gelu_ref(x)
    tailm = x <= -9.0
    worst = {}

    def far_tail(val, aux, E):
        v = f32(val.detach()).cpu().double()
        assert not bool(torch.isnan(v).any()), f"{what}: NaN in the GELU value"
        lim = x.abs() * E / 2
        if val.dtype == torch.bfloat16:
            lim = f32(lp(lim.float())).double()
        assert bool((v.abs() <= lim)[tailm].all()), f"{what}: |gelu(x)| > |x| E / 2 at an argument <= -9"
        if aux is not None:
            d = f32(aux.detach()).cpu().double()
            assert not bool(torch.isnan(d).any()), f"{what}: NaN in the derivative"
            dlim = E / 2 + 2.0 ** -21 + 1e-16          # (|gelu'(-9)| = 1e-18)
            if aux.dtype == torch.bfloat16:
                dlim = float(f32(lp(torch.tensor(dlim, dtype=torch.float32))))
            assert bool((d.abs() <= dlim)[tailm].all()), f"{what}: |gelu'(x)| > delta_dg at an argument <= -9"

    for name, o in outs.items():
        dgl, ddl, E = deltas(x, g, fit[name] if isinstance(fit, dict) else fit)
        if name == "f32":
            worst[name] = close32(o, g, dgl, f"{what}: gelu -> fp32")
            far_tail(o, None, E)
        elif name == "16":
            worst[name] = close16(o, g, dgl, f"{what}: gelu -> 16-bit")
            far_tail(o, None, E)
        elif name == "pair":
            val, aux = o
            gate = close16 if val.dtype == torch.bfloat16 else close32
            worst["pair value"] = gate(val, g, dgl, f"{what}: gelu of the pair form")
            worst["pair aux"] = gate(aux, dg, ddl, f"{what}: gelu' of the pair form (aux_out)")
            far_tail(val, aux, E)
            plain = outs.get("16" if val.dtype == torch.bfloat16 else "f32")
            if plain is not None:
                assert torch.equal(val.cpu().view(torch.int16 if val.dtype == torch.bfloat16 else torch.int32),
                                   plain.cpu().view(torch.int16 if val.dtype == torch.bfloat16 else torch.int32)), \
                    f"{what}: the pair form's value differs from the plain gelu output of the same kernel form"
        elif name == "split3":
            o = o.cpu()
            N = x.shape[1]
            assert o.shape == (x.shape[0], 3 * N) and torch.equal(o[:, :N].view(torch.int16), o[:, N:2 * N].view(torch.int16)), \
                f"{what}: the two hi thirds of the split rows differ"
            hi, lo = f32(o[:, :N]).double(), f32(o[:, 2 * N:]).double()
            lim = dgl + 2.0 ** -16 * g.abs()
            err = (hi + lo - g).abs()
            bad = ~(err <= lim)
            ratio = err / lim.clamp_min(1e-300)
            assert not bool(bad.any()), (f"{what}: hi + lo of the split rows: {int(bad.sum())} elements outside delta_g + 2^-16 |g|; worst err / delta "
                                         f"{float(torch.nan_to_num(ratio, nan=float('inf')).max()):.3f}")
            worst[name] = float(ratio.max())
            # hi is lp(g32), lo is lp(g32 - hi) of ONE fp32 value within delta_g: hi under the bracket, lo inside what a 16-bit rounding of g32 leaves
            close16(o[:, :N], g, dgl, f"{what}: hi third of the split rows")
            far_tail(o[:, :N], None, E)
        else:
            raise KeyError(name)
    return worst


def run_gelu(dev, dtype, kw, a, b, bias):
    """The outputs of one kernel form (ops.options(**kw)) for check_gelu."""
    M, N = a.shape[0], b.shape[0]
    a, b, bias = a.to(dev), b.to(dev), None if bias is None else bias.to(dev)
    outs = {}
    with ops.options(**kw):
        outs["f32"] = ops.gemm_nt(a, b, bias, out_dtype=torch.float32, epi=ops.EPI_GELU)
        if dtype == torch.bfloat16:
            outs["16"] = ops.gemm_nt(a, b, bias, out_dtype=dtype, epi=ops.EPI_GELU)
            if not f16_build():
                # (MAEST_SPLIT3_A rows are bf16 thirds, include/maest_hip.h: in half the lo third of |g| < 0.125 is subnormal, and hi + lo
                # cannot keep 2^-16 |g|)
                outs["split3"] = ops.gemm_nt(a, b, bias, out_dtype=ops.SPLIT3, epi=ops.EPI_GELU)
        aux = torch.empty((M, N), dtype=dtype, device=dev)
        val = ops.gemm_nt(a, b, bias, out_dtype=dtype, epi=ops.EPI_GELU, aux_out=aux)
        outs["pair"] = (val, aux)
    return outs


def case_gelu_grid(dev, dtype, forms, M=512, N=256, K=64):
    """Section 2: every GELU output of every kernel form in `forms` on the exact-argument grid, both passes.  -> {(form, pass, output): worst err / delta}."""
    worst = {}
    for second in (False, True):
        a, b, bias, x = operands(M, N, K, dtype, second)
        for kw in forms:
            outs = run_gelu(dev, dtype, kw, a, b, bias)
            fit = {o: e_fit(kw, dtype, o) for o in ("f32", "16", "pair", "split3")}
            for o, r in check_gelu(outs, x, fit, f"{kw}, {'acc + bias' if second else 'acc'}").items():
                worst[(str(kw), "bias" if second else "acc", o)] = r
    return worst


def exact_inputs(M, N, K, dtype, with_bias):
    """Section 3's operands: the grid of section 2 without the largest finite value (its sum with c16 is not an fp32 number in half), the
    fp32 accumulator acc32, a random 16-bit (fp32 for fp32 operands) multiplier and an fp32 residual on the 2^-14 grid, |res| < 8, so that
    (acc + bias) + res is exact."""
    a, b, _, x = operands(M, N, K, dtype, False, largest=False)
    acc32 = x.float()
    assert torch.equal(acc32.double(), x)
    bias = ((torch.arange(N) % 256).double() / 4096 + 2.0 ** -14).float() if with_bias else None
    pre = lp(rnd((M, N), 501), dtype)
    k = (torch.arange(M)[:, None] * 7919 + torch.arange(N)[None, :] * 104729) % (1 << 17) - (1 << 16)
    res = (k.double() / 2.0 ** 14).float()
    return a, b, bias, acc32, pre, res


def check_mul(got, acc32, bias, pre, what):
    """mul: (acc + bias) * pre -- ONE fp32 multiply of the fp32 sum, ONE rounding to the output type -- bit for bit."""
    v = acc32 if bias is None else acc32 + bias[None, :]
    want = v * f32(pre)
    if got.dtype == torch.bfloat16:
        _bits_equal(got, want, what)
    else:
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), what


def check_residual(got, acc32, bias, res, what):
    """residual: (acc + bias) + res in fp32, in that order (exact on these operands), bit for bit."""
    v = acc32 if bias is None else acc32 + bias[None, :]
    want = v + res
    assert torch.equal(want.double(), v.double() + res.double()), "the residual grid must keep the sum exact"
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), what


def case_epilogue_exact(dev, dtype, forms, M=512, N=256, K=64):
    """Section 3: the mul and residual epilogues of every kernel form on exact accumulators, with bias and without, bit for bit."""
    for with_bias in (True, False):
        a, b, bias, acc32, pre, res = exact_inputs(M, N, K, dtype, with_bias)
        bd = None if bias is None else bias.to(dev)
        for kw in forms:
            with ops.options(**kw):
                c = ops.gemm_nt(a.to(dev), b.to(dev), bd, out_dtype=dtype, epi=ops.EPI_MUL, aux_in=pre.to(dev))
                check_mul(c, acc32, bias, pre, f"mul -> {'16-bit' if dtype == torch.bfloat16 else 'fp32'} {kw}, bias {with_bias}")
                c = ops.gemm_nt(a.to(dev), b.to(dev), bd, out_dtype=torch.float32, epi=ops.EPI_RESIDUAL, aux_in=res.to(dev))
                check_residual(c, acc32, bias, res, f"residual -> fp32 {kw}, bias {with_bias}")
