"""CPU, no kernel: the gates of tests/epilogue_cases.py accept a faithful epilogue and reject defective ones.  A torch fp32 restatement of the
GEMM epilogue -- the two erf fits of csrc/common.h (gelu_pair2<false>: four terms on v_exp / v_rcp; gelu_pair<false>: Abramowitz-Stegun 7.1.26)
and libm's erf, then the store: fp32, round-to-nearest-even 16-bit, the value + aux pair, the [ hi | hi | lo ] split rows -- is fed to
check_gelu / check_mul / check_residual on the operands of case_gelu_grid / case_epilogue_exact, in both builds' 16-bit formats.  The faithful
restatement must sit inside every gate (err / delta <= 1); each defect of the table in DESIGN.md section 7b must leave at least the gate named there."""
import math

import pytest
import torch

from maest_amd import _lib
from tests import epilogue_cases as EC
from tests.kernel_cases import _neighbour16, f16_build, f32, lp

M, N, K = 512, 256, 64
F = torch.float32


def t(v):
    return torch.tensor(v, dtype=F)


def fit4(x, a3=-1.47149548, sign=True):
    """gelu_pair2<false>, statement by statement in fp32 (torch has no fma: the products round once more than the kernel's)."""
    pdf = torch.exp2(x * x * t(-0.72134752044448170) + t(-1.32574806473615900))
    hs = torch.copysign(t(0.5), x) if sign else torch.full_like(x, 0.5)
    r = 1.0 / ((x * hs) * t(0.54123076) + 1.0)
    poly = ((r * t(2.10931316) + t(a3)) * r + t(1.49964288)) * r + t(0.36917199)
    poly = poly * r
    cdf = (1.0 - poly * pdf) * hs + 0.5
    return x * cdf, x * pdf + cdf


def fit5(x, pdf_c=0.39894228040143268, sign=True, three=False):
    """gelu_pair<false>; `three`: the 3-term 7.1.25 in its place."""
    u = x * t(0.70710678118654752)
    e = torch.exp(-u * u)
    au = u.abs()
    if three:
        r = 1.0 / (1.0 + t(0.47047) * au)
        poly = r * (t(0.3480242) + r * (t(-0.0958798) + r * t(0.7478556)))
    else:
        r = 1.0 / (1.0 + t(0.3275911) * au)
        poly = r * (t(0.254829592) + r * (t(-0.284496736) + r * (t(1.421413741) + r * (t(-1.453152027) + r * t(1.061405429)))))
    ea = 1.0 - poly * e
    erfu = torch.where(u < 0, -ea, ea) if sign else ea
    cdf = 0.5 * (1.0 + erfu)
    return x * cdf, cdf + x * e * t(pdf_c)


def libm(x):
    u = x * t(0.70710678118654752)
    cdf = 0.5 * (1.0 + torch.erf(u))
    return x * cdf, cdf + x * torch.exp(-u * u) * t(0.39894228040143268)


def tanh_gelu(x):
    c = t(math.sqrt(2.0 / math.pi))
    th = torch.tanh(c * (x + t(0.044715) * x * x * x))
    return 0.5 * x * (1.0 + th), 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * c * (1.0 + 3 * t(0.044715) * x * x)


def truncate(v):
    """fp32 -> the build's 16-bit container, rounded toward zero."""
    r = lp(v)
    over = f32(r).abs() > v.abs()
    towards_zero = torch.where(f32(r) > 0, _neighbour16(r, False).view(torch.int16), _neighbour16(r, True).view(torch.int16)).view(torch.bfloat16)
    return torch.where(over, towards_zero.view(torch.int16), r.view(torch.int16)).view(torch.bfloat16)


def epilogue(arg32, fit, store=lp, aux_from_rounded=False):
    """The four GELU outputs of check_gelu for the fp32 arguments acc + bias."""
    g, dg = fit(arg32)
    if aux_from_rounded:
        dg = fit(f32(lp(arg32)))[1]
    hi = store(g)
    outs = {"f32": g, "16": hi, "pair": (hi, store(dg))}
    if not f16_build():          # (the split rows are bf16 thirds: include/maest_hip.h)
        outs["split3"] = torch.cat([hi, hi, store(g - f32(hi))], 1)
    return outs


@pytest.fixture(scope="module", params=["bf16", "f16"])
def grid(request):
    """Both passes' fp64 arguments and their fp32 form (exact, except next to the largest finite value) in one build's format."""
    with _lib.flavour(request.param):
        xs = [EC.operands(M, N, K, torch.bfloat16, second)[3] for second in (False, True)]
    return request.param, xs


def _rejects(flavour, xs, fit, e, names, **kw):
    """check_gelu raises on each output in `names` alone, in at least one of the two passes; -> the outputs of `names` it did not reject."""
    kept = []
    with _lib.flavour(flavour):
        for name in names:
            caught = False
            for x in xs:
                outs = epilogue(x.float(), fit, **kw)
                if name not in outs:
                    caught = True
                    break
                try:
                    EC.check_gelu({name: outs[name]}, x, e, "defect")
                except AssertionError:
                    caught = True
                    break
            if not caught:
                kept.append(name)
    return kept


ALL = ("f32", "16", "pair", "split3")
BITS16 = ("16", "pair", "split3")


def test_epilogue_gate_accepts_the_faithful_restatement(grid):
    flavour, xs = grid
    with _lib.flavour(flavour):
        for fit, e, name in ((fit4, EC.E_FIT4, "4-term fit"), (fit5, EC.E_FIT5, "5-term fit"), (libm, 0.0, "libm")):
            for x in xs:
                worst = EC.check_gelu(epilogue(x.float(), fit), x, e, name)
                print(f"  {flavour} {name}: worst err / delta " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
                assert max(worst.values()) <= 1.0 + 1e-9, (name, worst)


def test_epilogue_gate_rejects_gelu_defects(grid):
    flavour, xs = grid
    # tanh-GELU (4.7e-4 from erf-GELU), judged by the wider of the two fit bounds: every form
    assert _rejects(flavour, xs, tanh_gelu, EC.E_FIT4, ALL) == []
    # the 3-term 7.1.25 (2.5e-5): the fp32 output; the 16-bit forms that also catch it are printed (DESIGN.md section 7b lists them)
    kept = _rejects(flavour, xs, lambda x: fit5(x, three=True), EC.E_FIT4, ALL)
    print(f"  {flavour}: 3-term erf passes {kept or 'no form'}")
    assert "f32" not in kept
    # one constant of the 4-term fit off in its 4th digit
    assert "f32" not in _rejects(flavour, xs, lambda x: fit4(x, a3=-1.47249548), EC.E_FIT4, ("f32",))
    # the sign factor dropped for x < 0: every form, either fit
    assert _rejects(flavour, xs, lambda x: fit4(x, sign=False), EC.E_FIT4, ALL) == []
    assert _rejects(flavour, xs, lambda x: fit5(x, sign=False), EC.E_FIT5, ALL) == []
    # pdf constant 0.4 for 0.39894 (an error of 1.06e-3 |x| exp(-x^2 / 2) <= 6.4e-4 in the derivative alone): the aux of the pair form -- in half
    # anywhere, in bf16 at the negative arguments where gelu' is small
    assert _rejects(flavour, xs, lambda x: fit5(x, pdf_c=0.4), EC.E_FIT5, ("pair",)) == []
    neg = [x[:192] for x in xs]
    assert _rejects(flavour, neg, lambda x: fit5(x, pdf_c=0.4), EC.E_FIT5, ("pair",)) == []
    # a truncating 16-bit store: every 16-bit form
    assert _rejects(flavour, xs, fit4, EC.E_FIT4, BITS16, store=truncate) == []
    assert _rejects(flavour, xs, fit5, EC.E_FIT5, BITS16, store=truncate) == []
    # the aux computed from the argument rounded to 16 bits
    assert _rejects(flavour, xs, fit4, EC.E_FIT4, ("pair",), aux_from_rounded=True) == []


@pytest.mark.parametrize("flavour", ["bf16", "f16"])
@pytest.mark.parametrize("with_bias", [True, False])
def test_epilogue_exact_gate_rejects_double_roundings(flavour, with_bias):
    with _lib.flavour(flavour):
        a, b, bias, acc32, pre, res = EC.exact_inputs(M, N, K, torch.bfloat16, with_bias)
        v = acc32 if bias is None else acc32 + bias[None, :]
        EC.check_mul(lp(v * f32(pre)), acc32, bias, pre, "faithful mul")
        EC.check_residual(v + res, acc32, bias, res, "faithful residual")
        # the accumulator (+ bias) rounded to 16 bits before the multiply
        with pytest.raises(AssertionError, match="differ"):
            EC.check_mul(lp(f32(lp(v)) * f32(pre)), acc32, bias, pre, "mul of the rounded sum")
        if with_bias:
            # the bias added after the 16-bit rounding of the accumulator
            with pytest.raises(AssertionError, match="differ"):
                EC.check_mul(lp((f32(lp(acc32)) + bias[None, :]) * f32(pre)), acc32, bias, pre, "bias after the rounding")
            with pytest.raises(AssertionError):
                EC.check_residual((f32(lp(acc32)) + bias[None, :]) + res, acc32, bias, res, "bias after the rounding (residual)")
        # a truncating store
        with pytest.raises(AssertionError, match="differ"):
            EC.check_mul(truncate(v * f32(pre)), acc32, bias, pre, "truncating store")
