"""The attention maps (MAEST_ATTN_PROBS, ops.attn_probs) against an error bound that is DERIVED, not measured (a sibling of
attention_cases: the same helpers, the same two builds; run by test_emu_attn_probs.py under the emulator and by test_attn_probs_gpu.py).

The reference is the fp64 softmax of the operands as stored (16-bit operands: the values the build's 16 bits hold; MAEST_BF16_QS: the q
columns hold q' and the exponent factor is 1).  With

    c2 = fp32(scale) * fp32(log2 e)  (1 under BF16_QS),   t = c2 sum_d q_d k_d,   a = c2 sum_d |q_d| |k_d|,   u = 2^-24,
    gamma_n = n u / (1 - n u),   u_prod = 0 (fp32 / 16-bit operands: exact products),  2^-16 + 2^-23 (F32X3: the dropped lo * lo term
                                                                                        and the rounding of the lo parts)

the kernel's exponent t - m is off by at most

    delta(q, k) = a (gamma_66 + u_prod) + 2 u (|t| + max_j |t_j|)        products, fp32 sums, the scale fma, the max subtraction

and its probability by the relative error

    E(q, k) = ln 2 (delta(q, k) + max_j delta(q, j)) + (N + 8) u          own exponent, the sum's exponents, v_exp, the N-term sum, the division

    gate:   |p - p_ref| <= E p_ref + 2^-100   for every element          (results below the floor: flushed denormals of v_exp_f32)
            |sum_k p - 1| <= 2 (N + 8) u      for every row

E is 5e-5 .. 9e-5 at N = 64 .. 290 (x3: 2e-4 .. 4e-4): three orders below case_attention's 2e-2.  test_attn_probs_gate_rejects_defects
(test_emu_attn_probs.py) shows what the gate refuses."""
import functools

import numpy as np
import torch

from maest_amd import _lib, ops
from tests.kernel_cases import f16_build, f32, lp, rnd

H, HD, E = 12, 64, 768
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
U = 2.0 ** -24
FLOOR = 2.0 ** -100
SCALE = 0.125
CODES = ("f32", "x3", "16", "qs")          # MAEST_F32, MAEST_F32X3, MAEST_BF16 (the build's 16-bit type), MAEST_BF16_QS
U_PROD = {"f32": 0.0, "x3": 2.0 ** -16 + 2.0 ** -23, "16": 0.0, "qs": 0.0}

# (B, N, q_rows): the smallest shapes at which the kernel can go wrong
SHAPES = [(2, 64, 64),       # one full key tile
          (2, 70, 70),       # ragged last key tile and ragged query block
          (2, 161, 161),     # two query blocks, three key tiles
          (2, 161, 2),       # the head rows
          (2, 161, 40)]      # a partial second wave
SHAPE_GPU = (1, 353, 353)    # three query blocks (the device only)


def gamma(n):
    return n * U / (1 - n * U)


def c2_of(code, scale=SCALE):
    """The exponent per unit of the stored score product (csrc/attn_common.h attn_scale): an fp32 product."""
    return 1.0 if code == "qs" else float(np.float32(scale) * np.float32(LOG2E))


@functools.lru_cache(maxsize=None)
def _operands(B, N, code, seed, spike, times, f16):
    """-> (the qkv tensor the kernel reads, its values as stored in fp64 [B * N, 2304]).  spike: query 3 of head 0 (of every clip's
    token 3) scaled by 6 and key 5 set equal to it -- the reference's largest probability is 1.000, its smallest are below 2^-126.
    times: every operand scaled (3: exponents over +-40)."""
    x = rnd((B * N, 3 * E), seed, times)
    if spike:
        x = x.reshape(B, N, 3 * E).clone()
        x[:, 3, 0:HD] *= 6.0
        x[:, 5, E:E + HD] = x[:, 3, 0:HD]
        x = x.reshape(B * N, 3 * E)
    if code in ("f32", "x3"):
        qkv = x.contiguous()
    else:
        qkv = lp(x)
        if code == "qs":      # what the row-scaled qkv projection writes: q' = scale * log2(e) * q, rounded once
            qp = lp(f32(qkv[:, :E]) * float(np.float32(SCALE) * np.float32(LOG2E)))
            qkv = torch.cat([qp, qkv[:, E:]], 1).contiguous()
    return qkv, f32(qkv).double()


def operands(B, N, code, seed=30, spike=False, times=1.0):
    return _operands(B, N, code, seed, spike, times, f16_build() and code in ("16", "qs"))


def _heads(xs, B, N):
    """[B * N, 2304] -> q, k, v as [B, 12, N, 64]"""
    t = xs.reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def reference(xs, B, N, q_rows, c2, u_prod):
    """fp64 -> (p_ref, E) as [B, 12, q_rows, N]: the softmax of the stored operands and the relative bound of the module docstring."""
    q, k, _ = _heads(xs, B, N)
    q = q[:, :, :q_rows]
    t = c2 * (q @ k.transpose(-2, -1))
    a = c2 * (q.abs() @ k.abs().transpose(-2, -1))
    p_ref = torch.softmax(t * LN2, -1)
    delta = a * (gamma(66) + u_prod) + 2 * U * (t.abs() + t.abs().amax(-1, keepdim=True))
    bound = LN2 * (delta + delta.amax(-1, keepdim=True)) + (N + 8) * U
    return p_ref, bound


@functools.lru_cache(maxsize=None)
def _reference_of(B, N, q_rows, code, seed, spike, times, f16):
    _, xs = _operands(B, N, code, seed, spike, times, f16)
    return reference(xs, B, N, q_rows, c2_of(code), U_PROD[code])


def reference_of(B, N, q_rows, code, seed=30, spike=False, times=1.0):
    """The reference of operands(...) (computed once per case and build, shared by the tests, never modified)."""
    return _reference_of(B, N, q_rows, code, seed, spike, times, f16_build() and code in ("16", "qs"))


def gate(what, p, p_ref, bound, N):
    """The two conditions of the module docstring on p (any float dtype) [.., q_rows, N]; prints the worst share of the bound used and
    the worst row-sum deviation, returns them."""
    p = p.detach().cpu().double()
    assert p.shape == p_ref.shape, (what, tuple(p.shape), tuple(p_ref.shape))
    assert bool(torch.isfinite(p).all()), f"{what}: {int((~torch.isfinite(p)).sum())} non-finite probabilities (elements never written?)"
    err = (p - p_ref).abs()
    lim = bound * p_ref + FLOOR
    ratio = float((err / lim).max())
    dsum = float((p.sum(-1) - 1).abs().max())
    print(f"  {what}: worst |p - p_ref| / (E p_ref + 2^-100) = {ratio:.3f} (E {float(bound.min()):.1e} .. {float(bound.max()):.1e}), "
          f"row sums within {dsum:.1e} of 1 (limit {2 * (N + 8) * U:.1e})")
    bad = err > lim
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} probabilities outside the bound, worst {ratio:.2f} x; first at "
                                 f"{tuple(int(i) for i in bad.nonzero()[0])}")
    assert dsum <= 2 * (N + 8) * U, f"{what}: a row sums to 1 {dsum:+.3e} (limit {2 * (N + 8) * U:.1e})"
    return ratio, dsum


def head_mean(p):
    """(((p0 + p1) + p2) + ... + p11) * fp32(1 / 12) in fp32, heads ascending: the definition of the mean form."""
    acc = p[:, 0].clone()
    for h in range(1, H):
        acc = acc + p[:, h]
    return acc * torch.tensor(1.0 / 12.0, dtype=torch.float32)


def run(dev, B, N, q_rows, code, head_mean=False, **kw):
    qkv, _ = operands(B, N, code, **kw)
    return ops.attn_probs(qkv.to(dev), B, N, SCALE, q_rows=q_rows, x3=code == "x3", q_prescaled=code == "qs", head_mean=head_mean)


def _bits_equal(what, got, want):
    same = got.view(torch.int32) == want.view(torch.int32)
    assert bool(same.all()), (f"{what}: {int((~same).sum())}/{same.numel()} elements differ; first at "
                              f"{tuple(int(i) for i in (~same).nonzero()[0])}")


def case_probs(dev, B, N, q_rows, code, mean=True, **kw):
    """The per-head form through gate(); mean: the mean form bit for bit against head_mean() of it.  Returns (ratio, row-sum deviation)."""
    print(f"attention maps, {'f16' if f16_build() else 'bf16'} build, code {code}, B = {B}, N = {N}, q_rows = {q_rows}, {kw or 'plain'}")
    p = run(dev, B, N, q_rows, code, **kw).cpu()
    assert p.dtype == torch.float32 and p.shape == (B, H, q_rows, N)
    r = gate("per head", p, *reference_of(B, N, q_rows, code, **kw), N)
    if mean:
        pm = run(dev, B, N, q_rows, code, head_mean=True, **kw).cpu()
        assert pm.dtype == torch.float32 and pm.shape == (B, q_rows, N)
        _bits_equal("mean form against the ascending-head fp32 sum of the per-head form", pm, head_mean(p))
    return r


def case_mean(dev, B, N, q_rows, code, **kw):
    """The mean form alone: bit-identical to the ascending-head fp32 sum of the per-head output times fp32(1 / 12)."""
    p = run(dev, B, N, q_rows, code, **kw).cpu()
    pm = run(dev, B, N, q_rows, code, head_mean=True, **kw).cpu()
    assert pm.dtype == torch.float32 and pm.shape == (B, q_rows, N)
    _bits_equal("mean form against the ascending-head fp32 sum of the per-head form", pm, head_mean(p))


def case_repeat(dev, B, N, q_rows, code):
    """Two calls give bit-identical results, in both forms."""
    for hm in (False, True):
        a, b = run(dev, B, N, q_rows, code, head_mean=hm).cpu(), run(dev, B, N, q_rows, code, head_mean=hm).cpu()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"two calls differ (head_mean = {hm})"


def case_forward_consistency(dev, B, N):
    """A cross-check only: P @ v (fp64 on the host) against maest_attn_fwd's fp32-mode out, at case_attention's fp32 tolerance."""
    from tests.kernel_cases import close, tol
    qkv, xs = operands(B, N, "f32")
    p = run(dev, B, N, N, "f32").cpu().double()
    _, _, v = _heads(xs, B, N)
    want = (p @ v).transpose(1, 2).reshape(B * N, E).float()
    out = ops.attn_fwd(qkv.to(dev), B, N, SCALE)
    close(out, want, *tol(torch.float32), "attn_fwd out against P @ v of the maps")


def case_argument_errors(dev):
    """Every refusal of the flagged form returns MAEST_ERR_INVALID (status 1) with its message in maest_last_error()."""
    import pytest
    B, N = 1, 8
    qkv = rnd((B * N, 3 * E), 3).to(dev)
    qkv16 = lp(rnd((B * N, 3 * E), 3)).to(dev)
    out = torch.zeros(B * H * N * N + 4, dtype=torch.float32, device=dev)
    lse = torch.zeros(B * H * N, dtype=torch.float32, device=dev)
    P, PM = _lib.ATTN_PROBS, _lib.ATTN_PROBS_MEAN
    st = ops._s(qkv)

    def refused(match, q=qkv, o=out, l=None, code=_lib.F32 | P, q_rows=N):
        with pytest.raises(_lib.MaestHipError, match=match) as e:
            _lib.call("maest_attn_fwd_rows", ops._p(q), ops._p(o), ops._p(l), B, N, code, SCALE, q_rows, st)
        assert "status 1" in str(e.value)

    refused("MAEST_F32X3_A3", code=_lib.F32X3_A3 | P)
    refused("MAEST_F32X3_A3", code=_lib.F32X3_A3 | P | PM)
    refused("lse", l=lse)
    refused("lse", l=lse, q=qkv16, code=_lib.BF16 | P | PM)
    refused("q_rows", q_rows=0)
    refused("q_rows", q_rows=N + 1)
    refused("alignment", o=out[1:])
    refused("alignment", q=qkv.reshape(-1)[1:])
    refused("bad dtype", code=_lib.SPLIT3_A | P)
    refused("bad dtype", code=_lib.F16 | P)
    refused("MAEST_ATTN_PROBS_MEAN without", code=_lib.F32 | PM)
    refused("null pointer", o=None)
    # ... and the accepted codes still run, with and without the mean bit
    for code, q in ((_lib.F32, qkv), (_lib.F32X3, qkv), (_lib.BF16, qkv16), (_lib.BF16_QS, qkv16)):
        for fl in (P, P | PM):
            _lib.call("maest_attn_fwd_rows", ops._p(q), ops._p(out), None, B, N, code | fl, SCALE, N, st)


# ---------------------------------------------------------------------------------------------- doctored pipelines (tests of the gate)
def pipeline64(xs, B, N, q_rows, c2, defect=None):
    """The kernel's two passes in fp64 on the stored operands, with one of the defects the gate must refuse:
       "scale"     the exponent factor off by 2^-10
       "padding"   the padding keys of the ragged last tile left unmasked (zero keys: score 0)
       "bf16 sum"  normalisation by a sum of bf16-rounded exponentials
       "bf16 c2"   the exponent factor rounded to bf16"""
    q, k, _ = _heads(xs, B, N)
    q = q[:, :, :q_rows]
    if defect == "scale":
        c2 = c2 * (1 + 2.0 ** -10)
    if defect == "bf16 c2":
        c2 = float(torch.tensor(c2).bfloat16())
    t = c2 * (q @ k.transpose(-2, -1))
    if defect == "padding":
        t = torch.cat([t, torch.zeros(t.shape[:-1] + (-N % 64,), dtype=t.dtype)], -1)
    e = torch.exp2(t - t.amax(-1, keepdim=True))
    l = (e.float().bfloat16().double() if defect == "bf16 sum" else e).sum(-1, keepdim=True)
    return (e / l)[..., :N]
