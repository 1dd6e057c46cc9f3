"""Kernel-level parity cases shared by the emulator tests (CPU, tiny shapes) and the GPU tests.

Every case runs ONE C-ABI entry point through maest_amd.ops and compares it with the oracle
(oracle/maest_oracle.py) or with the one-line torch definition of the op, in fp32 on the CPU.
Tolerances: fp32 ("parity") mode 2e-5 relative unless stated; bf16 mode is checked against the
same math evaluated on bf16-ROUNDED operands (so the only difference is accumulation order).

The same cases run under the half-precision build (`with _lib.flavour("f16")`, libmaest_hip_f16.so): there a tensor tagged
torch.bfloat16 is the 16-bit operand CONTAINER whose bits the kernels read as IEEE half.  Every 16-bit operand is made with lp()
and read back with f32(), which follow the calling thread's build; 16-bit tolerances come from t16(bf16 value, f16 value).
(A tensor tagged torch.float16 is something else: the loader's half mel input, MAEST_F16, in both builds.)

16-bit results of the GEMM epilogues, LayerNorm and the patch-embed backward are also held to the rounding bracket close16(): the stored value
must be the round-to-nearest-even rounding of an fp32 value within a derived delta of an fp64 reference.
The LayerNorm, head and loss kernels on rows where fp32 is hard, against bounds counted from their roundings: tests/norm_cases.py (section 7c).
"""
import math

import numpy as np
import torch
from functools import partial
import torch.nn.functional as F

from maest_amd import _lib, ops
from oracle import maest_oracle as O


def rnd(shape, seed, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def f16_build():
    """Whether the calling thread's C-ABI calls go to the half-precision build (_lib.flavour("f16"))."""
    return _lib._tls.flavour == "f16"


def lp(t, dtype=torch.bfloat16):
    """fp32 -> `dtype`; for the 16-bit operand type (torch.bfloat16) the container of the calling thread's build: bfloat16, or the
    IEEE half bits (round to nearest even, +-inf past 65504, subnormals kept) tagged torch.bfloat16."""
    if dtype != torch.bfloat16:
        return t.to(dtype)
    return t.half().view(torch.bfloat16) if f16_build() else t.bfloat16()


def f32(t):
    """The inverse of lp(): a tensor -> its fp32 values, a 16-bit container read as the calling thread's build reads it."""
    if t.dtype == torch.bfloat16 and f16_build():
        return t.view(torch.float16).float()
    return t.float()


def t16(bf, f16):
    """A tolerance of a 16-bit result: `bf` in the bf16 build, `f16` (at most a quarter of it) in the half build."""
    assert f16 * 4 <= bf, (bf, f16)
    return f16 if f16_build() else bf


_errs = None     # record(): what -> worst error / reference maximum of the close() / note() calls inside the block


class record:
    """``with record() as errs:`` -- collect, per `what`, the worst |got - ref| / max |ref| that close() and note() see."""

    def __enter__(self):
        global _errs
        self.prev, _errs = _errs, {}
        return _errs

    def __exit__(self, *a):
        global _errs
        _errs = self.prev


def note(what, got, ref):
    """Record (no assertion) the error of `got` against ref(), a reference on UNROUNDED operands -- where the two builds differ by their
    operand rounding although the case's own reference (on rounded operands) leaves them both at fp32 noise."""
    if _errs is not None:
        a, b = f32(got.detach()).cpu().double(), ref().detach().cpu().double()
        e = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)
        _errs[what] = max(_errs.get(what, 0.0), e)


CONTROL_FLOOR = 1e-4     # bf16-build errors below this (relative to the output's maximum) are fp32 accumulation noise: not compared


def controlled(case, *args, **kw):
    """Run `case` in the half build, then on the same inputs in the bf16 build, and require every error the bf16 build shows above
    fp32 noise to be at least 4x smaller in the half build: a case cannot pass because the flavour switch was ignored, or because one
    constant, conversion or mnemonic of the half build still works in bf16.  Returns {what: (err f16, err bf16)}."""
    with record() as e16, _lib.flavour("f16"):
        case(*args, **kw)
    with record() as ebf:
        case(*args, **kw)
    both = {w: (e16[w], ebf[w]) for w in e16 if ebf.get(w, 0.0) > CONTROL_FLOOR}
    assert both, f"{case.__name__}: no result above fp32 noise to compare the two builds on"
    worst = max(both, key=lambda w: both[w][0] / both[w][1])
    print(f"{case.__name__}: worst f16 error {max(e16.values()):.2e}; closest to the control: {worst!r} f16 {both[worst][0]:.2e} "
          f"vs bf16 {both[worst][1]:.2e} (ratio {both[worst][1] / max(both[worst][0], 1e-30):.1f})")
    bad = {w: v for w, v in both.items() if not v[0] * 4 < v[1]}
    assert not bad, f"{case.__name__}: half build not 4x closer than bf16 (err f16, err bf16): {bad}"
    return both


def close(a, b, rtol, atol, what):
    a = f32(a.detach()).cpu()
    b = f32(b.detach()).cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    if _errs is not None:
        _errs[what] = max(_errs.get(what, 0.0), float(err.max()) / (float(b.abs().max()) + 1e-30))
    lim = atol + rtol * b.abs()
    bad = err > lim
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; max err {err.max().item():.3e} "
        f"(ref max {b.abs().max().item():.3e}); first bad index {tuple(int(i) for i in bad.nonzero()[0])}")


def tol(dtype):
    return (2e-5, 2e-5) if dtype == torch.float32 else (2e-2, 2e-2)


def _neighbour16(t, up):
    """The next value of the calling build's 16-bit format above (`up`) or below each element of the container `t`."""
    bits = t.view(torch.int16).to(torch.int32) & 0xffff
    mag = bits & 0x7fff
    o = torch.where(bits >= 0x8000, -mag, mag) + (1 if up else -1)          # the format's values in order; -0 and +0 are one
    return (o.abs() | torch.where(o < 0, 0x8000, 0)).to(torch.int16).view(torch.bfloat16)


def _fail(what, bad, ratio, got, ref, delta):
    """Raise for the elements `bad`, naming the worst one by `ratio` = err / delta (NaN results count as the worst)."""
    worst = torch.where(bad, torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")), torch.full_like(ratio, -1.0))
    i = tuple(int(v) for v in np.unravel_index(int(worst.argmax()), tuple(ratio.shape)))
    raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the gate; worst err / delta {float(ratio[i]):.3f} at {i}: "
                         f"got {float(got[i])!r}, reference {float(ref[i])!r}, delta {float(delta[i]):.3e}")


def close16(got, ref64, delta, what):
    """The rounding-bracket gate of a 16-bit result.  `got`: a 16-bit container of the calling build; `ref64`: the fp64 reference; `delta`
    (fp64, broadcast against ref64): the bound on the error of the fp32 value the kernel holds BEFORE its store.  Holds where
        lp((ref64 - delta).float()) <= f32(got) <= lp((ref64 + delta).float()),
    i.e. where the stored value is the round-to-nearest-even 16-bit rounding of some fp32 value within delta of the truth (rounding is monotonic:
    exact, no ulp arithmetic at binade edges).  Every element is gated; NaN fails.  Feeds record() like close().  Returns the worst err / delta,
    err = the distance from ref64 to the nearest real number that rounds to `got` (<= 1 where the gate holds, ties aside)."""
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16, (what, got.dtype)
    ref64 = ref64.detach().cpu().double()
    delta = delta.detach().cpu().double().expand_as(ref64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    g = f32(got).double()
    lo, hi = f32(lp((ref64 - delta).float())).double(), f32(lp((ref64 + delta).float())).double()
    if _errs is not None:
        _errs[what] = max(_errs.get(what, 0.0), float((g - ref64).abs().max()) / (float(ref64.abs().max()) + 1e-30))
    # the reals that round to got: between the midpoints to its two neighbours
    below, above = (g + f32(_neighbour16(got, False)).double()) / 2, (g + f32(_neighbour16(got, True)).double()) / 2
    err = torch.maximum(torch.maximum(below - ref64, ref64 - above), torch.zeros_like(g))
    ratio = torch.where(err > 0, err / delta.clamp_min(1e-300), torch.zeros_like(err))          # (NaN where got is NaN)
    bad = ~((lo <= g) & (g <= hi))
    if bool(bad.any()):
        _fail(what, bad, ratio, g, ref64, delta)
    return float(ratio.max())


def close32(got, ref64, delta, what):
    """close16's companion for an fp32 result: |got - ref64| <= delta + 2^-24 |ref64| (the error before the store, and the store's own rounding),
    every element, NaN fails.  Returns the worst err / (delta + 2^-24 |ref64|)."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32, (what, got.dtype)
    ref64 = ref64.detach().cpu().double()
    lim = delta.detach().cpu().double().expand_as(ref64) + 2.0 ** -24 * ref64.abs()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err = (got.double() - ref64).abs()
    if _errs is not None:
        _errs[what] = max(_errs.get(what, 0.0), float(err.max()) / (float(ref64.abs().max()) + 1e-30))
    ratio = torch.where(err > 0, err / lim.clamp_min(1e-300), torch.zeros_like(err))
    bad = ~(err <= lim)
    if bool(bad.any()):
        _fail(what, bad, ratio, got.double(), ref64, lim)
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ GEMM
def row_blocks(M, N, limit=1 << 22):
    """Row slices of an [M, N] result of at most `limit` elements each: the fp64 references of the large shapes are made block by block."""
    step = max(1, limit // N)
    return [slice(r, min(M, r + step)) for r in range(0, M, step)]


def gemm_ref64(a, b, bias):
    """fp64 a b^T + bias on the (rounded) operands, and the accumulation term of DESIGN.md section 7b,
        delta_acc = 2 (K + 1) 2^-24 (|a| |b|^T + |bias|):
    at most one fp32 ulp of a partial sum per addition whichever way the matrix unit rounds -- twice Higham's bound of a K-term dot product."""
    a64, b64 = f32(a).double(), f32(b).double()
    ref = a64 @ b64.t()
    mag = a64.abs() @ b64.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    return ref, 2 * (a.shape[1] + 1) * 2.0 ** -24 * mag


def gelu_fit_bound(dtype, M, N, K):
    """The documented bound of the erf form behind maest_gemm_nt's GELU epilogue at this shape under the options in force (epilogue_cases.e_fit):
    libm for fp32 operands, the four-term fit in the 256-row-tile kernels, Abramowitz-Stegun 7.1.26 in the 128 x 128 kernel."""
    from tests import epilogue_cases as EC
    if dtype == torch.float32:
        return 0.0
    big = M >= max(512, ops.get_option("gemm_min_m")) and N >= 256 and N % 256 == 0 and K % 64 == 0
    return EC.E_FIT4 if big else EC.E_FIT5


def gate_gelu(g, aux, a, b, bias, fit, what):
    """GELU outputs of a GEMM on random operands under the rounding bracket: gelu within delta_acc * 1.13 + delta_g (1.13 = max |gelu'|), gelu'
    within delta_acc * 0.80 + delta_dg (0.80 = max |gelu''| = 2 phi(0)); delta_g, delta_dg: epilogue_cases.deltas.  Every element, block by block."""
    from tests import epilogue_cases as EC
    worst = 0.0
    for r in row_blocks(a.shape[0], b.shape[0]):
        x, dacc = gemm_ref64(a[r], b, bias)
        g64, dg64 = EC.gelu_ref(x)
        dgl, ddl, _ = EC.deltas(x, g64, fit)
        for got, ref, delta, name in ((g, g64, dacc * 1.13 + dgl, "gelu"), (aux, dg64, dacc * 0.80 + ddl, "gelu' (aux_out)")):
            if got is not None:
                gate = close16 if got.dtype == torch.bfloat16 else close32
                worst = max(worst, gate(got[r], ref, delta, f"{what}: {name} under the rounding bracket"))
    return worst


def case_gemm(dev, dtype, M, N, K, seed=0, identity=True, wscale=1.0):
    """wscale: the scale of the weights b (1 / sqrt(K): most GELU arguments inside |x| < 3, where the function bends)."""
    a = lp(rnd((M, K), seed), dtype)
    b = lp(rnd((N, K), seed + 1, wscale), dtype)
    bias = rnd((N,), seed + 2)
    ref = f32(a) @ f32(b).t() + bias
    # fp32 accumulation-order noise of a K-term dot product of N(0,1) operands: ~ 4e-7 * K absolute
    rt, at = 1e-5, 4e-7 * K / math.sqrt(K / 64)
    c = ops.gemm_nt(a.to(dev), b.to(dev), bias.to(dev), out_dtype=torch.float32)
    close(c, ref, rt, at * math.sqrt(K / 64), "gemm none")
    note("gemm none (unrounded operands)", c, lambda: rnd((M, K), seed).double() @ rnd((N, K), seed + 1).double().t() + bias.double())
    # asymmetric A = I check of the output orientation
    if identity and M >= K and dtype == torch.float32:
        eye = torch.zeros(M, K)
        eye[:K, :K] = torch.eye(K)
        c = ops.gemm_nt(eye.to(dev), b.to(dev), None, out_dtype=torch.float32)
        close(c[:K], b.float().t(), 0, 1e-6, "gemm identity (transpose-detecting)")
    # GELU epilogue with aux_out
    aux = torch.empty((M, N), dtype=dtype, device=dev)
    g = ops.gemm_nt(a.to(dev), b.to(dev), bias.to(dev), out_dtype=dtype, epi=ops.EPI_GELU, aux_out=aux)
    rt2, at2 = (1e-5, at) if dtype == torch.float32 else (t16(1e-2, 2.5e-3), t16(1e-2, 2.5e-3))
    xr = ref.clone().requires_grad_(True)
    F.gelu(xr).sum().backward()
    close(aux, xr.grad, rt2, max(at2 * math.sqrt(K / 64), 2e-6), "gemm gelu aux (= gelu' saved for backward)")
    close(g, F.gelu(ref), rt2, at2 * math.sqrt(K / 64), "gemm gelu")
    gate_gelu(g, aux, a, b, bias, gelu_fit_bound(dtype, M, N, K), "gemm")
    # residual epilogue
    res = rnd((M, N), seed + 3)
    c = ops.gemm_nt(a.to(dev), b.to(dev), bias.to(dev), out_dtype=torch.float32, epi=ops.EPI_RESIDUAL,
                    aux_in=res.to(dev))
    close(c, ref + res, rt, at * math.sqrt(K / 64), "gemm residual")
    # mul epilogue (dgrad through GELU: acc * saved gelu')
    pre = lp(rnd((M, N), seed + 4), dtype)
    c = ops.gemm_nt(a.to(dev), b.to(dev), None, out_dtype=dtype, epi=ops.EPI_MUL, aux_in=pre.to(dev))
    close(c, (ref - bias) * f32(pre), rt2, at2 * math.sqrt(K / 64), "gemm mul")
    for r in row_blocks(M, N):          # (acc * pre: one multiply, one rounding -- the accumulation term times |pre|)
        x, dacc = gemm_ref64(a[r], b, None)
        p64 = f32(pre[r]).double()
        (close16 if dtype == torch.bfloat16 else close32)(c[r], x * p64, dacc * p64.abs(), "gemm mul under the rounding bracket")
    # split-K atomic accumulate
    acc = torch.zeros((M, N), dtype=torch.float32, device=dev)
    ops.gemm_nt(a.to(dev), b.to(dev), None, out=acc, epi=ops.EPI_ATOMIC, split_k=3)
    close(acc, ref - bias, rt, at * math.sqrt(K / 64), "gemm split-k")


def _same_products(new, old, exact, what, K=64):
    """The one-wave-per-SIMD GEMM against the 8-wave kernel on the same operands.  `exact` (the host emulator, whose MFMA twins add the k terms
    one by one in both shapes): bit for bit.  On the device the two kernels use different matrix instructions since round 6 (16x16x32 against
    32x32x16: 32 against 16 products per rounding step), so their fp32 sums differ in the last bits: fp32 outputs within 4e-7 sqrt(K) of the output
    scale, bf16 outputs within one bf16 ulp and at most 2 % of the elements different at all."""
    if exact:
        assert torch.equal(new, old), what
        return
    a, b = f32(new), f32(old)
    scale = float(b.abs().max()) + 1e-30
    diff = (a - b).abs()
    if new.dtype == torch.float32:
        assert float(diff.max()) <= 4e-7 * math.sqrt(K) * scale + 1e-30, f"{what}: max |diff| {float(diff.max()):.3e} of scale {scale:.3e}"
    else:
        ulp = t16(2.0 ** -7, 2.0 ** -10) * torch.maximum(a.abs(), b.abs()) + 1e-30      # one 16-bit ulp is 2^-8 .. 2^-7 (half: 2^-11 .. 2^-10) of the value
        assert bool((diff <= ulp).all()), f"{what}: more than one 16-bit ulp apart (max ratio {float((diff / ulp).max()):.2f})"
        assert float((diff > 0).float().mean()) <= 0.02, f"{what}: {100 * float((diff > 0).float().mean()):.2f} % of the elements differ"


def case_gemm_one_wave_per_simd(dev, M, N, K, seed=11, only=None, pair=True, both_bias=False, exact=None):
    """gemm_nt256o_kernel (gemm_nt_ow.hip: bf16 operands, the default of the 256 x 256 path) against the 8-wave kernel it replaces
    (gemm_variant = 3): the same products summed in the same order and the same epilogue arithmetic -- bit for bit, in every
    epilogue form, ragged last tile row included -- and against the oracle's fp32 matmul."""
    dt = torch.bfloat16
    a = lp(rnd((M, K), seed), dt).to(dev)
    w = lp(rnd((N, K), seed + 1) * 0.1, dt).to(dev)
    bias = rnd((N,), seed + 2).to(dev)
    res = rnd((M, N), seed + 3).to(dev)
    mul = lp(rnd((M, N), seed + 4), dt).to(dev)
    ref = f32(a).cpu() @ f32(w).cpu().t() + bias.cpu()
    forms = [("none -> bf16", dict(out_dtype=dt)), ("none -> fp32", dict(out_dtype=torch.float32)),
             ("gelu -> bf16", dict(out_dtype=dt, epi=ops.EPI_GELU)), ("gelu -> fp32", dict(out_dtype=torch.float32, epi=ops.EPI_GELU)),
             ("residual -> fp32", dict(out_dtype=torch.float32, epi=ops.EPI_RESIDUAL, aux_in=res)),
             ("mul -> bf16", dict(out_dtype=dt, epi=ops.EPI_MUL, aux_in=mul))]
    for name, kw in forms:
        if only is not None and name not in only:
            continue
        for b in ((bias, None) if (only is None or both_bias) else (bias,)):
            new = ops.gemm_nt(a, w, b, **kw)
            with ops.options(gemm_variant=3):
                old = ops.gemm_nt(a, w, b, **kw)
            _same_products(new, old, str(dev) == "cpu" if exact is None else exact,
                           f"one-wave-per-SIMD GEMM differs from the 8-wave kernel: {name}, bias {b is not None}", K)
    c = ops.gemm_nt(a, w, bias, out_dtype=torch.float32)
    close(c, ref, 1e-5, 4e-7 * K, "one-wave-per-SIMD GEMM vs fp32 matmul")
    if not pair:
        return
    aux_n = torch.empty((M, N), dtype=dt, device=dev)
    aux_o = torch.empty((M, N), dtype=dt, device=dev)
    g_n = ops.gemm_nt(a, w, bias, out_dtype=dt, epi=ops.EPI_GELU, aux_out=aux_n)
    with ops.options(gemm_variant=3):
        g_o = ops.gemm_nt(a, w, bias, out_dtype=dt, epi=ops.EPI_GELU, aux_out=aux_o)
    _same_products(g_n, g_o, str(dev) == "cpu", "GELU of the pair form differs between the two 256 x 256 kernels", K)
    _same_products(aux_n, aux_o, str(dev) == "cpu", "GELU' of the pair form differs between the two 256 x 256 kernels", K)
    close(g_n, F.gelu(ref), t16(1e-2, 2.5e-3), t16(1e-2, 2.5e-3) * math.sqrt(K / 64), "one-wave-per-SIMD GEMM: gelu")
    gate_gelu(g_n, aux_n, a.cpu(), w.cpu(), bias.cpu(), gelu_fit_bound(dt, M, N, K), "one-wave-per-SIMD GEMM")


def case_gemm_rowdot(dev, dtype, M, N, K, ntok, seed=7):
    """maest_gemm_nt_rowdot: C = A B^T + bias in `dtype`, and rowdot[item, 64-column group, row in item] = the dot
    product of the STORED row segment of C with `other` -- the attention backward's delta out of the dgrad GEMM's
    epilogue.  Reference: the products of the returned C itself (exactly the values the kernel multiplied)."""
    a = lp(rnd((M, K), seed), dtype)
    b = lp(rnd((N, K), seed + 1), dtype)
    bias = rnd((N,), seed + 2)
    other = lp(rnd((M, N), seed + 3), dtype)
    c, rd = ops.gemm_nt_rowdot(a.to(dev), b.to(dev), other.to(dev), ntok, out_dtype=dtype, bias=bias.to(dev))
    ref = f32(a) @ f32(b).t() + bias
    rt, at = (1e-5, 4e-7 * K) if dtype == torch.float32 else (t16(1e-2, 2.5e-3), t16(1e-2, 2.5e-3) * math.sqrt(K / 64))
    close(c, ref, rt, at, "gemm rowdot: C")
    for r in row_blocks(M, N):
        ref64, dacc = gemm_ref64(a[r], b, bias)
        (close16 if dtype == torch.bfloat16 else close32)(c[r], ref64, dacc, "gemm rowdot: C under the rounding bracket")
    assert rd.shape == (M // ntok, N // 64, ntok)
    want = (f32(c).cpu() * f32(other)).reshape(M // ntok, ntok, N // 64, 64).sum(-1).permute(0, 2, 1)
    close(rd, want, 1e-5, 1e-5 * math.sqrt(64) * float(f32(c).abs().max()), "gemm rowdot: per-(row, group) dot products")
    if dtype == torch.bfloat16:
        # bf16: the call above took gemm_nt256o_kernel where the shape has 256-row tiles; the 8-wave kernel's row-dot epilogue does the
        # same arithmetic in the same order
        with ops.options(gemm_variant=3):
            c3, rd3 = ops.gemm_nt_rowdot(a.to(dev), b.to(dev), other.to(dev), ntok, out_dtype=dtype, bias=bias.to(dev))
        _same_products(c, c3, str(dev) == "cpu", "row-dot epilogue: C differs between the one-wave-per-SIMD and 8-wave kernels", K)
        close(rd, rd3, t16(1e-2, 2.5e-3), 1e-2 * math.sqrt(64) * float(f32(c).abs().max()) * t16(2.0 ** -7, 2.0 ** -10), "row-dot epilogue: dot products of the two kernels")


def case_gemm_tn(dev, dtype, K, M, N, seed=3, lda_pad=0, splits=(1, 3, 0)):
    """wgrad form: out[M,N] += a[K,M]^T b[K,N], colsum[M] += a.sum(0); ragged K (token tail)."""
    a_full = lp(rnd((K, M + lda_pad), seed), dtype)
    a = a_full[:, :M]
    b = lp(rnd((K, N), seed + 1), dtype)
    ref = f32(a).t() @ f32(b)
    ref_cs = f32(a).sum(0)
    at = 4e-7 * K + (0 if dtype == torch.float32 else t16(1e-3, 2.5e-4))
    for sk in splits:
        out = torch.zeros((M, N), dtype=torch.float32, device=dev)
        cs = torch.zeros(M, dtype=torch.float32, device=dev)
        a_dev = a_full.to(dev)[:, :M]
        ops.gemm_tn(a_dev, b.to(dev), out, colsum=cs, split_k=sk, M=M, N=N)
        close(out, ref, 1e-5, at, f"gemm_tn split_k={sk}")
        close(cs, ref_cs, 1e-5, at, f"gemm_tn colsum split_k={sk}")
        note("gemm_tn (unrounded operands)", out, lambda: rnd((K, M + lda_pad), seed)[:, :M].double().t() @ rnd((K, N), seed + 1).double())
        note("gemm_tn colsum (unrounded operands)", cs, lambda: rnd((K, M + lda_pad), seed)[:, :M].double().sum(0))
    # the deterministic split-K combine of the 256-tile kernel (tn_reduce=1; where the shape takes it): partial tiles through a
    # workspace, summed in split order by a second kernel -- bit-reproducible, and ACCUMULATING into `out` like the atomics
    a_dev, b_dev = a_full.to(dev)[:, :M], b.to(dev)
    with ops.options(tn_reduce=1):
        outs = []
        for _ in range(1 if _lib.host_emulation() else 2):
            out = torch.zeros((M, N), dtype=torch.float32, device=dev)
            ops.gemm_tn(a_dev, b_dev, out, split_k=0, M=M, N=N)
            outs.append(out)
        close(outs[0], ref, 1e-5, at, "gemm_tn (workspace combine)")
        if ops.gemm_tn_workspace_bytes(dtype, M, N, K) > 0 and len(outs) == 2:
            assert torch.equal(outs[0], outs[1]), "gemm_tn through the workspace must be bit-reproducible"
            ops.gemm_tn(a_dev, b_dev, outs[1], split_k=0, M=M, N=N)            # second call accumulates
            close(outs[1], 2 * ref, 1e-5, 2 * at, "gemm_tn accumulates into a non-zero C")
    # transpose-detecting: A = [I | 0] picks rows of B
    if dtype == torch.float32 and K >= M:
        eye = torch.zeros(K, M)
        eye[:M, :M] = torch.eye(M)
        out = torch.zeros((M, N), dtype=torch.float32, device=dev)
        ops.gemm_tn(eye.to(dev), b.to(dev), out)
        close(out, b.float()[:M], 0, 1e-6, "gemm_tn identity")


# ------------------------------------------------------------------------------------- transposes
def case_transpose(dev, dtype, rows, cols):
    src = lp(rnd((rows, cols), 5), dtype)
    ld = ops.round_up(rows, 64)
    out = ops.transpose(src.to(dev), ld)
    assert out.shape == (cols, ld)
    close(out[:, :rows], src.t(), 0, 0, "transpose")
    assert float(f32(out[:, rows:]).abs().sum()) == 0.0, "transpose pad must be zero"
    w = rnd((rows, cols), 6)
    d, dt_ = ops.cast_weights(w.to(dev), dtype, want=True, want_t=True)
    close(d, lp(w, dtype), 0, 0, "cast")
    close(dt_, lp(w, dtype).t(), 0, 0, "cast transposed")
    # many parameters, one launch (ragged shapes, NULL outputs)
    # (sides that are multiples of 4 take the kernel's quad path -- 16-byte loads, 8-byte stores --, the others the element-wise one)
    ws = [rnd((rows, cols), 60), rnd((cols, 33), 61), rnd((65, 64), 62), rnd((132, 72), 63), rnd((64, 256), 64)]
    for want, want_t in ((True, True), (False, True), (True, False)):
        outs = ops.cast_weights_multi([t.to(dev) for t in ws], dtype, want=want, want_t=want_t)
        for t, (o, ot) in zip(ws, outs):
            assert (o is None) == (not want) and (ot is None) == (not want_t)
            if o is not None:
                close(o, lp(t, dtype), 0, 0, "cast multi")
            if ot is not None:
                close(ot, lp(t, dtype).t(), 0, 0, "cast multi transposed")


    # leading rows of the PLAIN copy scaled before the rounding (the q rows of a qkv projection, MAEST_BF16_QS); the transposed copy is not
    for t in (rnd((132, 72), 65), rnd((70, 33), 66)):
        (o, ot), = ops.cast_weights_multi([t.to(dev)], dtype, want=True, want_t=True, scaled_rows=[40], row_scale=0.1803)
        want_o = t.clone()
        want_o[:40] *= 0.1803
        close(o, lp(want_o, dtype), 0, 0, "cast multi, scaled leading rows")
        close(ot, lp(t, dtype).t(), 0, 0, "cast multi, transposed copy unscaled")


# --------------------------------------------------------------------------------------- LayerNorm
def case_layernorm(dev, dtype, rows):
    x = rnd((rows, 768), 7, 2.0) + 0.3
    g = 1.0 + rnd((768,), 8, 0.1)
    b = rnd((768,), 9, 0.1)
    y, mean, rstd = ops.layernorm_fwd(x.to(dev), g.to(dev), b.to(dev), 1e-6, dtype, save_stats=True)
    ref = F.layer_norm(x, (768,), g, b, 1e-6)
    rt, at = (1e-5, 1e-5) if dtype == torch.float32 else (t16(1e-2, 2.5e-3), t16(1e-2, 2.5e-3))
    close(y, ref, rt, at, "layernorm fwd")
    if dtype == torch.bfloat16:         # the 16-bit rounding of a value the fp32 build's gate accepts
        ref64 = F.layer_norm(x.double(), (768,), g.double(), b.double(), 1e-6)
        close16(y, ref64, 1e-5 + 1e-5 * ref64.abs(), "layernorm fwd under the rounding bracket")
    close(mean, x.mean(1), 1e-5, 1e-6, "layernorm mean")
    close(rstd, 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-6), 1e-5, 1e-6, "layernorm rstd")
    # residual add fused into the LayerNorm that follows it: x_new = x + delta exactly (one fp32 add per element),
    # y / statistics = those of the plain kernel on x_new, bit for bit
    delta = lp(rnd((rows, 768), 12, 0.5), dtype)
    xn, y2, mean2, rstd2 = ops.add_layernorm_fwd(x.to(dev), delta.to(dev), g.to(dev), b.to(dev), 1e-6, dtype, save_stats=True)
    assert torch.equal(xn.cpu(), x + f32(delta)), "fused residual add must be the exact fp32 sum"
    y3, mean3, rstd3 = ops.layernorm_fwd(xn, g.to(dev), b.to(dev), 1e-6, dtype, save_stats=True)
    assert torch.equal(y2, y3) and torch.equal(mean2, mean3) and torch.equal(rstd2, rstd3)
    if dtype == torch.float32:
        # MAEST_SPLIT3_A output (the A operand of the split-bf16 product run as one bf16 GEMM over 3 K): rows [ hi | hi | lo ] with
        # hi = bf16(y), lo = bf16(y - hi) of the fp32 result, from both kernels
        s3 = ops.layernorm_fwd(x.to(dev), g.to(dev), b.to(dev), 1e-6, ops.SPLIT3).cpu()
        yf = y.cpu()
        hi = lp(yf)
        lo = lp(yf - f32(hi))
        assert s3.shape == (rows, 2304) and s3.dtype == torch.bfloat16
        assert torch.equal(s3[:, :768], hi) and torch.equal(s3[:, 768:1536], hi) and torch.equal(s3[:, 1536:], lo), "layernorm split3 rows"
        xn3, s3b = ops.add_layernorm_fwd(x.to(dev), delta.to(dev), g.to(dev), b.to(dev), 1e-6, ops.SPLIT3)
        y2f = y2.cpu()
        hi2 = lp(y2f)
        assert torch.equal(xn3, xn) and torch.equal(s3b.cpu(), torch.cat([hi2, hi2, lp(y2f - f32(hi2))], 1)), "add + layernorm split3 rows"
    # backward
    dy = lp(rnd((rows, 768), 10), dtype)
    dres = rnd((rows, 768), 11)
    xr = x.clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    F.layer_norm(xr, (768,), gr, br, 1e-6).backward(f32(dy))
    dg = torch.zeros(768, device=dev)
    db = torch.zeros(768, device=dev)
    dx, dx_lp = ops.layernorm_bwd(dy.to(dev), x.to(dev), g.to(dev), mean, rstd, dres.to(dev), dg, db, lp_dtype=dtype)
    close(dx, xr.grad + dres, 1e-4, 1e-5, "layernorm dx")
    close(dx_lp, xr.grad + dres, *((1e-4, 1e-5) if dtype == torch.float32 else (t16(1e-2, 2.5e-3), t16(1e-2, 2.5e-3))), "layernorm dx_lp")
    if dtype == torch.bfloat16:
        x64 = x.double().requires_grad_(True)
        F.layer_norm(x64, (768,), g.double(), b.double(), 1e-6).backward(f32(dy).double())
        dx64 = x64.grad + dres.double()
        close16(dx_lp, dx64, 1e-5 + 1e-4 * dx64.abs(), "layernorm dx_lp under the rounding bracket")
        _bits_equal(dx_lp, dx.cpu(), "layernorm dx_lp = the 16-bit rounding of the dx of the same kernel")
    close(dg, gr.grad, 1e-4, 1e-4 * math.sqrt(rows), "layernorm dgamma")
    close(db, br.grad, 1e-4, 1e-4 * math.sqrt(rows), "layernorm dbeta")
    # compact residual gradient (the first 2 tokens of every clip of n_tok tokens; zero for the others): bit for bit
    # the dense call on the scattered tensor
    for n_tok in (1, 3, 11):
        if rows % n_tok or n_tok < 2 and rows < 2:
            continue
        n_head = min(2, n_tok)
        clips = rows // n_tok
        dres_c = rnd((clips * n_head, 768), 13)
        dense = torch.zeros(clips, n_tok, 768)
        dense[:, :n_head] = dres_c.reshape(clips, n_head, 768)
        dg1, db1 = torch.zeros(768, device=dev), torch.zeros(768, device=dev)
        want, want_lp = ops.layernorm_bwd(dy.to(dev), x.to(dev), g.to(dev), mean, rstd, dense.reshape(rows, 768).to(dev),
                                          dg1, db1, lp_dtype=dtype)
        dg2, db2 = torch.zeros(768, device=dev), torch.zeros(768, device=dev)
        got, got_lp = ops.layernorm_bwd(dy.to(dev), x.to(dev), g.to(dev), mean, rstd, dres_c.to(dev), dg2, db2,
                                        lp_dtype=dtype, head_tokens=(n_tok, n_head))
        assert torch.equal(got, want) and torch.equal(got_lp, want_lp), f"compact dres, n_tok={n_tok}"


# --------------------------------------------------------------------------------------- attention
def _attn_ref(qkv, B, N, scale):
    q, k, v = qkv.reshape(B, N, 3, 12, 64).permute(2, 0, 3, 1, 4)
    att = ((q @ k.transpose(-2, -1)) * scale).softmax(-1)
    return (att @ v).transpose(1, 2).reshape(B * N, 768), torch.logsumexp((q @ k.transpose(-2, -1)) * scale, -1)


def case_attention(dev, dtype, B, N, seed=20, spike=False, bf16_tol=3e-2, fwd_tol=2e-2, qs=False):
    """16-bit tolerances: bf16_tol / fwd_tol in the bf16 build, an eighth of them in the half build.
    qs (bf16 only): the MAEST_BF16_QS contract -- the q columns of the tensor handed to the kernels hold q' = scale * log2(e) * q
    (rounded once); the oracle runs on q = q' / (scale * log2(e)) and dQ is compared as the gradient with respect to that q."""
    assert not qs or dtype == torch.bfloat16
    attn_fwd, attn_bwd = partial(ops.attn_fwd, q_prescaled=qs), partial(ops.attn_bwd, q_prescaled=qs)
    if dtype != torch.float32:
        bf16_tol, fwd_tol = t16(bf16_tol, bf16_tol / 8), t16(fwd_tol, fwd_tol / 8)
    qkv = lp(rnd((B * N, 2304), seed, 1.0), dtype)
    if spike:  # force a large running-max jump at a late key tile (online-softmax rescale branch)
        qf = f32(qkv).clone()
        key = min(N - 1, 70)
        qf[key, 768:768 + 64] = qf[3, 0:64] * 6.0
        qkv = lp(qf, dtype)
    scale = 0.125
    x = f32(qkv)
    if qs:
        c = scale * 1.4426950408889634
        qp = lp(f32(qkv[:, :768]) * c, dtype)          # what the row-scaled projection writes
        qkv = torch.cat([qp, qkv[:, 768:]], dim=1).contiguous()
        x = torch.cat([f32(qp) / c, x[:, 768:]], dim=1)
    out, lse = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True)
    x = x.requires_grad_(True)
    ref, ref_lse = _attn_ref(x, B, N, scale)
    rt, at = (2e-5, 2e-5) if dtype == torch.float32 else (fwd_tol, fwd_tol)
    close(out, ref, rt, at, "attention fwd")
    close(lse, ref_lse, 1e-4, 1e-4 if dtype == torch.float32 else fwd_tol, "attention lse")
    if dtype == torch.bfloat16:
        # the call above took the shape's default: the persistent one-wave-per-SIMD kernel for N > 320, four-wave workgroups with
        # LDS-DMA-fed tiles below.  Every form against the oracle: the four-wave DMA form (2), the register-staged form every other
        # dtype uses (1) -- those two bit for bit (the same products in the same order; only the tile staging differs) -- and the
        # persistent form (3) at this N whatever it is (its Q is pre-scaled by scale * log2 e and rounded to bf16 once more, its
        # row sums are those of the rounded probabilities: close, not equal)
        with ops.options(attn_fwd=2):
            out2, lse2 = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True)
        close(out2, ref, rt, at, "attention fwd (four-wave workgroups, LDS-DMA tiles)")
        with ops.options(attn_fwd=1):
            out1, lse1 = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True)
        close(out1, ref, rt, at, "attention fwd (register-staged tiles)")
        assert torch.equal(out1, out2) and torch.equal(lse1, lse2), "DMA-fed and register-staged attention forward differ"
        with ops.options(attn_fwd=3):
            out3, lse3 = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True)
            out3b, lse3b = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True)
        close(out3, ref, rt, at, "attention fwd (persistent)")
        close(lse3, ref_lse, 1e-4, fwd_tol, "attention lse (persistent)")
        assert torch.equal(out3, out3b) and torch.equal(lse3, lse3b), "the persistent attention forward does not repeat bit for bit"
        # other workgroup sizes of the four-wave form: the same per-wave arithmetic, other tile dealing (GPU only: the host emulator
        # takes seconds per launch and the CPU suite has to stay short)
        for nw in (() if _lib.host_emulation() else (5, 6, 8)):
            with ops.options(attn_fwd=2, attn_fwd_waves=nw):
                outw, lsew = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True)
            assert torch.equal(outw, out2) and torch.equal(lsew, lse2), f"attention forward with {nw} waves per workgroup differs"
    # backward (the oracle's autograd on the same rounded operands)
    dout = lp(rnd((B * N, 768), seed + 1), dtype)
    ref.backward(f32(dout))
    out_ref_lp = lp(ref.detach(), dtype)
    dqkv = attn_bwd(qkv.to(dev), out_ref_lp.to(dev), dout.to(dev), ref_lse.detach().contiguous().to(dev), B, N, scale)
    rt, at = (1e-4, 1e-4) if dtype == torch.float32 else (bf16_tol, bf16_tol)
    g = x.grad
    close(dqkv[:, 1536:], g[:, 1536:], rt, at, "attention dV")
    close(dqkv[:, 768:1536], g[:, 768:1536], rt, at, "attention dK")
    close(dqkv[:, :768], g[:, :768], rt, at, "attention dQ")
    if dtype == torch.bfloat16:
        # the two-kernel dK/dV + dQ form streams its tiles by LDS-DMA (unpadded, swizzled); the register-staged padded tiles
        # (attn_bwd = 4) run the same products in the same order: bit for bit, ragged last tiles included
        args = (qkv.to(dev), out_ref_lp.to(dev), dout.to(dev), ref_lse.detach().contiguous().to(dev), B, N, scale)
        with ops.options(attn_bwd=1):
            dq_dma = attn_bwd(*args)
        with ops.options(attn_bwd=4):
            dq_reg = attn_bwd(*args)
        close(dq_dma, g, rt, at, "attention backward (two-kernel, DMA-fed tiles)")
        assert torch.equal(dq_dma, dq_reg), "DMA-fed and register-staged two-kernel attention backward differ"
    if dtype == torch.bfloat16:
        # the pairing the model runs: the backward fed with the out / lse its OWN forward wrote (above: the oracle's), for the
        # four-wave form and for the persistent form -- whose lse is the log-sum of its rounded probabilities, so that the P the
        # backward recomputes does not sum to exactly 1 per row: inside the same tolerance against autograd
        for form, what in ((2, "four-wave"), (3, "persistent")):
            with ops.options(attn_fwd=form):
                o_f, lse_f = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True)
            dq_f = attn_bwd(qkv.to(dev), o_f, dout.to(dev), lse_f, B, N, scale)
            # (raw q through the persistent forward: that kernel rounds scale * log2(e) * q to bf16 a second time, the backward does
            # not -- on a forced spike the two disagree by ~1.5e-2 on the dominating exponent; the model feeds pre-scaled q, `qs`)
            k = 2.0 if (form == 3 and spike and not qs) else 1.0
            close(dq_f, g, k * rt, k * at, f"attention backward on the {what} forward's own out / lse")
    if dtype == torch.bfloat16 and N <= 320:
        # the call above took the fused one-pass kernel (bf16, <= 10 key blocks); the two-kernel dK/dV + dQ form must
        # agree with the oracle too, and the two with each other to bf16 rounding of the same quantities
        with ops.options(attn_bwd=1):
            dq2 = attn_bwd(qkv.to(dev), out_ref_lp.to(dev), dout.to(dev), ref_lse.detach().contiguous().to(dev), B, N, scale)
        close(dq2[:, 1536:], g[:, 1536:], rt, at, "attention dV (two-kernel)")
        close(dq2[:, 768:1536], g[:, 768:1536], rt, at, "attention dK (two-kernel)")
        close(dq2[:, :768], g[:, :768], rt, at, "attention dQ (two-kernel)")
        close(dqkv, f32(dq2), t16(2e-2, 2.5e-3), t16(2e-2, 2.5e-3), "fused vs two-kernel attention backward")
        if N > 256:
            # the default call above took the PERSISTENT form (one workgroup per CU walking its (batch, head) items); the
            # one-workgroup-per-item form against the oracle as well, and the two bit for bit (same sums in the same order)
            with ops.options(attn_bwd=3):
                dq4 = attn_bwd(qkv.to(dev), out_ref_lp.to(dev), dout.to(dev), ref_lse.detach().contiguous().to(dev), B, N, scale)
            close(dq4, g, rt, at, "attention backward (fused, one workgroup per item)")
            assert torch.equal(dq4, dqkv), "persistent and per-item fused attention backward differ"


def case_attention_head_rows(dev, dtype, B, N, seed=25):
    """The last block's attention: only the first two queries of every clip are wanted.  Forward: the rows the
    restricted kernel writes (the 32-row tile holding them) equal the complete kernel's bit for bit.  Backward (fused bf16
    kernel): equal -- to bf16 rounding of the same sums -- to the complete backward fed a dO that is zero beyond row 2, with
    dQ = 0 for every other query; shapes the fused kernel does not serve are refused loudly."""
    from maest_amd._lib import MaestHipError
    qkv = lp(rnd((B * N, 2304), seed, 1.0), dtype).to(dev)
    scale = 0.125
    tl = 2e-2 if dtype == torch.float32 else t16(2e-2, 2.5e-3)      # (two kernels' roundings of the same sums)
    # (the complete pass in the four-wave form the restricted pass is a subset of: above 320 tokens the default complete pass
    # is the persistent kernel, equal to rounding only -- checked next)
    with ops.options(attn_fwd=2 if dtype == torch.bfloat16 else 0):
        full, lse_full = ops.attn_fwd(qkv, B, N, scale, save_lse=True)
    part, lse_part = ops.attn_fwd(qkv, B, N, scale, save_lse=True, q_rows=2)
    nv = min(32, N)
    f3, p3 = full.reshape(B, N, 768), part.reshape(B, N, 768)
    assert torch.equal(p3[:, :nv], f3[:, :nv]), "restricted forward differs on the rows it computes"
    note("restricted forward (unrounded operands)", p3[:, :nv], lambda: _attn_ref(rnd((B * N, 2304), seed, 1.0), B, N, scale)[0].reshape(B, N, 768)[:, :nv])
    assert torch.equal(lse_part[:, :, :nv], lse_full[:, :, :nv])
    dflt, lse_dflt = ops.attn_fwd(qkv, B, N, scale, save_lse=True)
    close(dflt, full, tl, tl, "default complete forward vs four-wave form")
    close(lse_dflt.cpu(), lse_full.cpu(), 1e-4, tl, "default complete forward vs four-wave form (lse)")
    # gather / scatter of the head tokens' rows
    comp = ops.gather_head_rows(full, B, N, 2)
    assert torch.equal(comp.reshape(B, 2, 768), f3[:, :2])
    back = ops.scatter_head_rows(comp, B, N, 2, nv).reshape(B, N, 768)
    assert torch.equal(back[:, :2], f3[:, :2]) and not back[:, 2:nv].any()
    xf = rnd((B * N, 768), seed + 3).to(dev)
    assert torch.equal(ops.gather_head_rows(xf, B, N, 2).reshape(B, 2, 768), xf.reshape(B, N, 768)[:, :2])
    dout_c = lp(rnd((B * 2, 768), seed + 1), dtype).to(dev)
    dense = ops.scatter_head_rows(dout_c, B, N, 2, N)          # zero everywhere else
    if ops.attn_bwd_rows_supported(dtype, N):
        want = ops.attn_bwd(qkv, full, dense, lse_full, B, N, scale)
        got = ops.attn_bwd(qkv, part, ops.scatter_head_rows(dout_c, B, N, 2, nv), lse_part, B, N, scale, q_rows=2)
        close(got[:, 768:], want[:, 768:], tl, tl, "restricted attention backward dK, dV")
        g3, w3 = got.reshape(B, N, 2304), want.reshape(B, N, 2304)
        close(g3[:, :2, :768], w3[:, :2, :768], tl, tl, "restricted attention backward dQ")
        assert not g3[:, 2:, :768].any(), "queries without gradient must get dQ = 0"
        with ops.options(attn_bwd=1):
            two = ops.attn_bwd(qkv, full, dense, lse_full, B, N, scale)
        close(got[:, 768:], two[:, 768:], tl, tl, "restricted fused vs complete two-kernel backward")
    else:
        try:
            ops.attn_bwd(qkv, full, dense, lse_full, B, N, scale, q_rows=2)
        except MaestHipError as e:
            assert "q_rows" in str(e)
        else:
            raise AssertionError("restricted backward must be refused on shapes the fused kernel does not serve")


# ----------------------------------------------------------------------------- patch embed pieces
def case_patch_embed(dev, dtype, B, T, patchout=0, mix=False, seed=30, masked=False, stride=(10, 10)):
    """stride: (frequency, time) step of the 16 x 16 patches (models/maest.py:214-241; every published architecture: (10, 10))."""
    Fdim = 96
    x = rnd((B, Fdim, T), seed)
    Tp = (T - 16) // stride[1] + 1
    Fp = (Fdim - 16) // stride[0] + 1
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    keep = np.sort(rng.permutation(Tp)[: Tp - patchout]).astype(np.int32) if patchout else None
    Tk = Tp - patchout
    t_list = torch.arange(Tp) if keep is None else torch.from_numpy(keep).long()
    tok = torch.stack(torch.meshgrid(torch.arange(Fp), t_list, indexing="ij"), -1).reshape(-1, 2).to(torch.int32)
    tok_dev = tok.contiguous().to(dev)
    perm = lam = t_str = f_str = None
    xm = x
    if masked:
        # SpecMasking stripes per clip (helpers/spec_masking.py:27-33), applied by the loader BEFORE mixup; explicit
        # (start, width) lists incl. zero-width, edge-touching and overlapping stripes
        n_t, n_f = 5, 3
        t_str = torch.from_numpy(np.stack([rng.integers(0, T - 8, (B, n_t)), rng.integers(0, 9, (B, n_t))], -1).astype(np.int32))
        f_str = torch.from_numpy(np.stack([rng.integers(0, Fdim - 5, (B, n_f)), rng.integers(0, 6, (B, n_f))], -1).astype(np.int32))
        t_str[0, 0] = torch.tensor([T - 3, 8])          # runs past the right edge: clamped
        f_str[0, 0] = torch.tensor([Fdim - 2, 5])
        xm = torch.stack([O.spec_masking(x[b], [tuple(v) for v in t_str[b].tolist()], [tuple(v) for v in f_str[b].tolist()])
                          for b in range(B)])
    if mix:
        perm = torch.from_numpy(rng.permutation(B).astype(np.int32))
        lam = torch.from_numpy(rng.random(B).astype(np.float32))
        xm = O.mixup(xm, perm.long(), lam)
    cols = ops.patch_im2col(x.to(dev), tok_dev, dtype, stride=stride,
                            perm=None if perm is None else perm.to(dev), lam=None if lam is None else lam.to(dev),
                            t_stripes=None if t_str is None else t_str.to(dev), f_stripes=None if f_str is None else f_str.to(dev))
    if masked and not mix and dtype == torch.float32:
        # the fused predicate must equal the stand-alone kernel (maest_spec_mask) bit for bit
        xs = ops.spec_mask_(x.clone().to(dev), t_str.to(dev), f_str.to(dev))
        cols2 = ops.patch_im2col(xs, tok_dev, dtype, stride=stride)
        assert torch.equal(cols, cols2), "fused SpecMasking differs from spec_mask_ + im2col"
    # a float16 batch (what the reference's loader hands out, discogs/dataset.py:58-67) widened inside the load must
    # equal the same values passed as fp32, bit for bit
    xh = x.half()
    kw = dict(stride=stride, perm=None if perm is None else perm.to(dev), lam=None if lam is None else lam.to(dev),
              t_stripes=None if t_str is None else t_str.to(dev), f_stripes=None if f_str is None else f_str.to(dev))
    assert torch.equal(ops.patch_im2col(xh.to(dev), tok_dev, dtype, **kw),
                       ops.patch_im2col(xh.float().to(dev), tok_dev, dtype, **kw)), "fp16 input path differs from x.float()"
    ref = F.unfold(xm.unsqueeze(1), kernel_size=16, stride=stride)      # [B, 256, Fp*Tp]
    ref = ref.reshape(B, 256, Fp, Tp)
    if keep is not None:
        ref = ref[:, :, :, torch.from_numpy(keep).long()]
    ref = ref.permute(0, 2, 3, 1).reshape(B * Fp * Tk, 256)
    close(cols, lp(ref, dtype), 0, 1e-6 if dtype == torch.float32 else 0, "im2col")
    # token assembly vs oracle.tokens_from_patches
    Tt = (62 if T <= 640 else T // 10) if stride[1] == 10 else Tp + 1
    sd = {"cls_token": rnd((1, 1, 768), 40, .02), "dist_token": rnd((1, 1, 768), 41, .02),
          "new_pos_embed": rnd((1, 2, 768), 42, .02), "freq_new_pos_embed": rnd((1, 768, Fp, 1), 43, .02),
          "time_new_pos_embed": rnd((1, 768, 1, Tt), 44, .02)}
    toff = 0 if patchout == 0 else min(1, Tt - Tp)
    conv = rnd((B, 768, Fp, Tp), 45)
    want = O.tokens_from_patches(conv, sd, toffset=toff, t_keep=None if keep is None else keep.tolist())
    convk = conv if keep is None else conv[:, :, :, torch.from_numpy(keep).long()]
    patches = convk.permute(0, 2, 3, 1).reshape(B * Fp * Tk, 768).contiguous()
    x0 = ops.token_assemble(patches.to(dev), sd["cls_token"].reshape(768).to(dev), sd["dist_token"].reshape(768).to(dev),
                            sd["new_pos_embed"].reshape(2, 768).contiguous().to(dev),
                            sd["freq_new_pos_embed"].reshape(768, Fp).contiguous().to(dev),
                            sd["time_new_pos_embed"].reshape(768, Tt).contiguous().to(dev), toff, tok_dev, B)
    close(x0, want, 0, 1e-6, "token assemble")
    # backward of token assembly
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    convg = conv.clone().requires_grad_(True)
    dx0 = rnd(tuple(want.shape), 46)
    O.tokens_from_patches(convg, sdg, toffset=toff, t_keep=None if keep is None else keep.tolist()).backward(dx0)
    z = lambda *s: torch.zeros(*s, device=dev)
    d_cls, d_dist, d_np, d_fp, d_tp = z(768), z(768), z(2, 768), z(768, Fp), z(768, Tt)
    dp = ops.token_assemble_bwd(dx0.to(dev), B, Fp, Tt, toff, tok_dev, dtype, d_cls, d_dist, d_np, d_fp, d_tp)
    gk = convg.grad if keep is None else convg.grad[:, :, :, torch.from_numpy(keep).long()]
    close(dp, gk.permute(0, 2, 3, 1).reshape(B * Fp * Tk, 768), *((0, 1e-6) if dtype == torch.float32 else (t16(1e-2, 2.5e-3), t16(1e-2, 2.5e-3))), "dpatches")
    if dtype == torch.bfloat16:
        close16(dp, gk.permute(0, 2, 3, 1).reshape(B * Fp * Tk, 768).double(), torch.tensor(1e-6, dtype=torch.float64), "dpatches under the rounding bracket")
    close(d_cls, sdg["cls_token"].grad.reshape(768), 1e-5, 1e-5, "d cls")
    close(d_dist, sdg["dist_token"].grad.reshape(768), 1e-5, 1e-5, "d dist")
    close(d_np, sdg["new_pos_embed"].grad.reshape(2, 768), 1e-5, 1e-5, "d new_pos")
    close(d_fp, sdg["freq_new_pos_embed"].grad.reshape(768, Fp), 1e-4, 1e-4, "d freq_pos")
    close(d_tp, sdg["time_new_pos_embed"].grad.reshape(768, Tt), 1e-4, 1e-4, "d time_pos")


# ------------------------------------------------------------------------------------------- head
def case_head(dev, B, N):
    x = rnd((B, N, 768), 50, 1.5)
    g = 1.0 + rnd((768,), 51, 0.1)
    b = rnd((768,), 52, 0.1)
    cls, dist, feat, mean, rstd = ops.head_pool_fwd(x.to(dev), g.to(dev), b.to(dev), 1e-6, save_stats=True)
    xr = x.clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    xn = F.layer_norm(xr, (768,), gr, br, 1e-6)
    close(cls, xn[:, 0], 1e-5, 1e-5, "head cls")
    close(dist, xn[:, 1], 1e-5, 1e-5, "head dist")
    close(feat, (xn[:, 0] + xn[:, 1]) / 2, 1e-5, 1e-5, "head feat")
    dc, dd, df = rnd((B, 768), 53), rnd((B, 768), 54), rnd((B, 768), 55)
    ((xn[:, 0] * dc).sum() + (xn[:, 1] * dd).sum() + (((xn[:, 0] + xn[:, 1]) / 2) * df).sum()).backward()
    dg = torch.zeros(768, device=dev)
    db = torch.zeros(768, device=dev)
    dx = ops.head_pool_bwd(dc.to(dev), dd.to(dev), df.to(dev), x.to(dev), g.to(dev), mean, rstd, dg, db)
    close(dx, xr.grad, 1e-4, 1e-5, "head dx")
    close(dg, gr.grad, 1e-4, 1e-4, "head dgamma")
    close(db, br.grad, 1e-4, 1e-4, "head dbeta")
    emb = ops.embed_pool(x.to(dev))
    close(emb, torch.cat([x[:, 0], x[:, 1], x[:, 2:].mean(1)], 1), 1e-5, 1e-5, "embed pool")


def case_loss(dev, rows, cols):
    z = rnd((rows, cols), 60, 2.0)
    rng = np.random.Generator(np.random.PCG64(61))
    y = torch.from_numpy((rng.random((rows, cols)) < 0.1).astype(np.float32))
    perm = torch.from_numpy(rng.permutation(rows).astype(np.int32))
    lam = torch.from_numpy(rng.random(rows).astype(np.float32))
    zr = z.clone().requires_grad_(True)
    ym = O.mixup(y, perm.long(), lam)
    ref = F.binary_cross_entropy_with_logits(zr, ym)
    ref.backward()
    loss, dz = ops.bce_logits(z.to(dev), y.to(dev), 1.0, perm.to(dev), lam.to(dev))
    close(loss, ref.detach(), 1e-5, 1e-6, "bce loss")
    close(dz, zr.grad, 1e-4, 1e-8, "bce dlogits")
    loss2, _ = ops.bce_logits(z.to(dev), y.to(dev), 0.5)
    close(loss2, 0.5 * F.binary_cross_entropy_with_logits(z, y), 1e-5, 1e-6, "bce weighted")
    act = ops.sigmoid_mean(z.to(dev))
    close(act, torch.sigmoid(z).mean(0), 1e-5, 1e-6, "sigmoid mean")
    src = rnd((rows, cols), 62)
    out = torch.zeros(cols, device=dev)
    ops.colsum(src.to(dev), out)
    close(out, src.sum(0), 1e-4, 1e-4, "colsum")
    srcb = lp(src)
    out = torch.zeros(cols, device=dev)
    ops.colsum(srcb.to(dev), out)
    close(out, f32(srcb).sum(0), 1e-4, 1e-4, "colsum bf16")
    note("colsum 16-bit (unrounded operands)", out, lambda: src.double().sum(0))
    v = rnd((1000,), 63)
    w = ops.scale_(v.clone().to(dev), 0.25)
    close(w, v * 0.25, 0, 0, "scale")


def case_spec_mask(dev, B, T):
    x = rnd((B, 96, T), 70)
    rng = np.random.Generator(np.random.PCG64(71))
    ts = np.stack([rng.integers(0, T - 8, (B, 5)), rng.integers(0, 8, (B, 5))], -1).astype(np.int32)
    fs = np.stack([rng.integers(0, 96 - 5, (B, 3)), rng.integers(0, 5, (B, 3))], -1).astype(np.int32)
    want = torch.stack([O.spec_masking(x[b], [tuple(p) for p in ts[b]], [tuple(p) for p in fs[b]]) for b in range(B)])
    got = ops.spec_mask_(x.clone().to(dev), torch.from_numpy(ts).to(dev), torch.from_numpy(fs).to(dev))
    close(got, want, 0, 0, "spec mask")


def case_mel(dev, B, S, seed=80):
    from maest_amd.melspectrogram import MelSpectrogram
    rng = np.random.Generator(np.random.PCG64(seed))
    w = torch.from_numpy((rng.random((B, S), dtype=np.float32) * 2 - 1) * 0.5)
    mel = MelSpectrogram()
    got = mel(w.to(dev))
    want = O.logmel(w)
    assert got.shape == want.shape == (B, 96, 1 + S // 256)
    # north_star tolerance for floating point: 1e-3 relative (values are O(1) after log compression)
    close(got, want, 1e-3, 1e-3, "logmel")
    err = (got.cpu() - want).abs().max().item()
    assert err < 2e-4, f"logmel max abs err {err}"


# ------------------------------------------------------------------ on-disk mel chunks -> input
def case_melfile(dev, tmp_path, size=50, counts=(80, 30, 31, 50, 1, 45), offsets=(13, 0, 0, 0, 0, 20), seed=90):
    """MelFileReader (host plan + one device kernel) against the oracle restatement of the reference reader,
    bit-exact (float16 arithmetic reproduced on the device): plain slice, short files (even / odd padding),
    exact length, a single frame, and an offset that runs past the end of the file."""
    from maest_amd.melfile import MelFileReader
    from oracle import melfile_oracle as MO
    rd = MelFileReader(tmp_path, clip_length=1, sample_rate=size, hop_size=1)     # melspectrogram_size = size
    assert rd.melspectrogram_size == size
    rng = np.random.Generator(np.random.PCG64(seed))
    names = []
    for i, n in enumerate(counts):
        fr = (rng.random((n, 96), dtype=np.float32) * 5.0).astype("float16")
        name = f"clip{i}.mel"
        fr.tofile(tmp_path / name)
        names.append(name)
    for normalize in (True, False):
        got = rd.load_batch(names, dev, offsets=list(offsets), normalize=normalize)
        assert got.shape == (len(counts), 1, 96, size) and got.dtype == torch.float32
        for i, name in enumerate(names):
            want = MO.load_melspectrogram(tmp_path / name, size, 96, offsets[i])
            if normalize:
                want = MO.norm_func(want)
            assert want.dtype == np.float16
            w32 = torch.from_numpy(want.astype(np.float32))
            assert torch.equal(got[i].cpu(), w32), (
                f"melfile clip {i} normalize={normalize}: max diff {(got[i].cpu() - w32).abs().max().item()}")


# ------------------------------------------------------------------ second mel parameterisation
def case_augment_mel(dev, B, S, seed=95):
    """AugmentMelSTFT (csrc/mel2.hip) against the oracle restatement: eval mode, and training mode with the
    band-edge jitter and stripes replayed from the same torch seed."""
    from maest_amd.preprocess import AugmentMelSTFT
    rng = np.random.Generator(np.random.PCG64(seed))
    w = torch.from_numpy((rng.random((B, S), dtype=np.float32) * 2 - 1) * 0.5)
    m = AugmentMelSTFT().to(dev).eval()
    got = m(w.to(dev))
    want = O.augment_mel(w)
    assert got.shape == want.shape == (B, 128, 1 + (S - 1) // 320)
    close(got, want, 1e-3, 1e-3, "augment mel (eval)")
    # training: the reference draws fmin, fmax (torch.randint x2), then the frequency and the time stripe (rand x2 each)
    m = AugmentMelSTFT(fmin_aug_range=10, fmax_aug_range=2000).to(dev).train()
    torch.manual_seed(7)
    got = m(w.to(dev))
    torch.manual_seed(7)
    fmin = 0.0 + torch.randint(10, (1,)).item()
    fmax = m.fmax + 2000 // 2 - torch.randint(2000, (1,)).item()
    T = want.shape[-1]
    v = torch.rand(1) * 48; mv = torch.rand(1) * (128 - v); fs = (int(mv.long()), int(v.long()))
    v = torch.rand(1) * 192; mv = torch.rand(1) * (T - v); ts = (int(mv.long()), int(v.long()))
    want = O.augment_mel(w, fmin=fmin, fmax=fmax, f_stripe=fs, t_stripe=ts)
    close(got, want, 1e-3, 1e-3, "augment mel (train)")


# ------------------------------------------------------------------ stochastic weight averaging
def case_swa(dev):
    shapes = [(768, 33), (5,), (4097,), (3, 1, 16, 16)]
    avg = [rnd(sh, 110 + i) for i, sh in enumerate(shapes)]
    want = [a.clone() for a in avg]
    got = [a.clone().to(dev) for a in avg]
    for step in range(3):
        cur = [rnd(sh, 120 + 10 * step + i) for i, sh in enumerate(shapes)]
        inv = 1.0 / (step + 2)
        ops.swa_update_multi(got, [c.to(dev) for c in cur], inv)
        want = [w + (c - w) * inv for w, c in zip(want, cur)]
    for g, w in zip(got, want):
        close(g, w, 1e-6, 1e-7, "swa running mean")


# ------------------------------------------------------------------------------------- split-bf16 ("bf16x3") products
def case_split_precision(dev, M=512, N=256, K=192, B=1, Ntok=75):
    """fp32 tensors with the matrix products as three bf16 MFMAs on hi/lo operand splits (common.h: mma_chunk2):
    the 256-tile NT GEMM (every epilogue path shares the main loop: checked on bias + residual) and the attention
    forward, against fp64 references.  Gate: 1e-4 of the output scale -- 40x tighter than plain bf16 operands manage
    (~4e-3) and an order of magnitude inside the 1e-3 parity gate; plain-bf16 results on the same data are asserted
    to be well OUTSIDE it, so the test cannot pass on a silently taken bf16 path."""
    a, b, bias, res = rnd((M, K), 50), rnd((N, K), 51), rnd((N,), 52), rnd((M, N), 53)
    ref = (a.double() @ b.double().t() + bias.double() + res.double())
    scale = ref.abs().max().item()
    with ops.options(gemm_min_m=512):
        c = ops.gemm_nt(a.to(dev), b.to(dev), bias.to(dev), out_dtype=torch.float32, epi=ops.EPI_RESIDUAL,
                        aux_in=res.to(dev), x3=True)
    qkv = rnd((B * Ntok, 2304), 54)
    out, lse = ops.attn_fwd(qkv.to(dev), B, Ntok, 0.125, save_lse=True, x3=True)
    # backward products: the wgrad form (256-tile TN kernel) and the attention backward
    ta, tb = rnd((288, 256), 55), rnd((288, 512), 56)
    tout = torch.zeros((256, 512), dtype=torch.float32, device=dev)
    tcs = torch.zeros(256, dtype=torch.float32, device=dev)
    with ops.options(gemm_variant=4):
        ops.gemm_tn(ta.to(dev), tb.to(dev), tout, colsum=tcs, split_k=0, x3=True)
    xq = qkv.double().requires_grad_(True)
    oref, lref = _attn_ref(xq, B, Ntok, 0.125)
    dout = rnd((B * Ntok, 768), 57)
    oref.backward(dout.double())
    dqkv = ops.attn_bwd(qkv.to(dev), oref.detach().float().to(dev), dout.to(dev), lref.detach().float().contiguous().to(dev),
                        B, Ntok, 0.125, x3=True)
    tref = ta.double().t() @ tb.double()
    et = (tout.double().cpu() - tref).abs().max().item() / tref.abs().max().item()
    assert et < 1e-4, f"split-bf16 TN GEMM: {et:.2e} of the output scale"
    assert (tcs.double().cpu() - ta.double().sum(0)).abs().max().item() < 1e-4
    eb = (dqkv.double().cpu() - xq.grad).abs().max().item() / xq.grad.abs().max().item()
    assert eb < 1e-4, f"split-bf16 attention backward: {eb:.2e} of the gradient scale"
    e = (c.double().cpu() - ref).abs().max().item() / scale
    assert e < 1e-4, f"split-bf16 GEMM: {e:.2e} of the output scale"
    with ops.options(gemm_min_m=512):
        c16 = ops.gemm_nt(lp(a).to(dev), lp(b).to(dev), bias.to(dev), out_dtype=torch.float32,
                          epi=ops.EPI_RESIDUAL, aux_in=res.to(dev))
    e16 = (c16.double().cpu() - ref).abs().max().item() / scale
    assert e16 > 10 * e, f"plain bf16 operands ({e16:.2e}) should be far coarser than the split ({e:.2e})"
    # the same three-term product as ONE bf16 GEMM over 3 K (MAEST_SPLIT3_A x MAEST_SPLIT3_B rows; the bf16 kernels, fp32 output): the weight
    # rows come from maest_cast_weights_multi, the activation rows are built here as the LayerNorm / attention kernels write them
    b3 = ops.cast_weights_multi([b.to(dev)], ops.SPLIT3)[0][0]
    bh = lp(b)
    assert torch.equal(b3.cpu(), torch.cat([bh, lp(b - f32(bh)), bh], 1)), "split3 weight rows"
    ah = lp(a)
    a3 = torch.cat([ah, ah, lp(a - f32(ah))], 1).contiguous()
    with ops.options(gemm_min_m=512):
        c3 = ops.gemm_nt(a3.to(dev), b3, bias.to(dev), out_dtype=torch.float32, epi=ops.EPI_RESIDUAL, aux_in=res.to(dev))
    e3 = (c3.double().cpu() - ref).abs().max().item() / scale
    assert e3 < 1e-4, f"split-bf16 GEMM as one bf16 GEMM over 3 K: {e3:.2e} of the output scale"
    # ... and the GELU epilogue writing its result in the same row form (the fc1 -> fc2 hand-over): hi / lo of the fp32-output epilogue's values
    gref = F.gelu(a.double() @ b.double().t() + bias.double())
    for big in (True, False):      # the staged epilogue form of the 256-row-tile kernel; the element-wise one of the 128 x 128 kernel (small M)
        with ops.options(gemm_min_m=512 if big else 1 << 30):
            gf = ops.gemm_nt(a3.to(dev), b3, bias.to(dev), out_dtype=torch.float32, epi=ops.EPI_GELU).cpu()
            g3 = ops.gemm_nt(a3.to(dev), b3, bias.to(dev), out_dtype=ops.SPLIT3, epi=ops.EPI_GELU).cpu()
        gh = lp(gf)
        assert g3.shape == (M, 3 * N) and torch.equal(g3[:, :N], g3[:, N:2 * N]), "split3 rows: the two hi thirds"
        same_kernel = (not big) or ops.gemm_split3_out_fast(M, N, 3 * K)
        if same_kernel:      # both outputs left the same main loop: the split of the very fp32 values
            assert torch.equal(g3, torch.cat([gh, gh, lp(gf - f32(gh))], 1)), f"GELU epilogue split3 rows (big = {big})"
        # (a build without the one-wave-per-SIMD kernel writes the fp32 form from the eight-wave kernel and the split form from the 128 x 128 one)
        rec = f32(g3[:, :N]).double() + f32(g3[:, 2 * N:]).double()
        assert (rec - gref).abs().max().item() / gref.abs().max().item() < 1e-4, "hi + lo of the split rows"
        assert (gf.double() - gref).abs().max().item() / gref.abs().max().item() < 1e-4
    o3 = ops.attn_fwd(qkv.to(dev), B, Ntok, 0.125, x3=True, out_split3=True).cpu()
    of = out.cpu()
    oh = lp(of)
    assert torch.equal(o3, torch.cat([oh, oh, lp(of - f32(oh))], 1)), "attention forward split3 rows"
    oref, lref = oref.detach(), lref.detach()
    eo = (out.double().cpu() - oref).abs().max().item() / oref.abs().max().item()
    el = (lse.double().cpu() - lref).abs().max().item()
    assert eo < 1e-4 and el < 1e-4, f"split-bf16 attention forward: out {eo:.2e}, lse {el:.2e}"
    # (the call above took the kernel that splits the K / V tiles once while staging them; the per-use split form behind attn_fwd = 1)
    with ops.options(attn_fwd=1):
        out1, lse1 = ops.attn_fwd(qkv.to(dev), B, Ntok, 0.125, save_lse=True, x3=True)
    eo1 = (out1.double().cpu() - oref).abs().max().item() / oref.abs().max().item()
    assert eo1 < 1e-4 and (lse1.double().cpu() - lref).abs().max().item() < 1e-4, f"split-bf16 attention forward (per-use split): {eo1:.2e}"
    return e, eo


# ------------------------------------------------------------------------------------- the half format's edges
def _half_bits_equal(got, want_f32, what):
    """`got` (a 16-bit container of the half build) holds exactly torch's .half() of `want_f32`: round to nearest even, +-inf past 65504,
    subnormals kept (not flushed).  NaN compared as NaN."""
    g = got.detach().cpu().view(torch.int16)
    w = want_f32.detach().cpu().half().view(torch.int16)
    nan = torch.isnan(want_f32.cpu())
    same = (g == w) | (nan & torch.isnan(got.detach().cpu().view(torch.float16)))
    if not bool(same.all()):
        i = tuple(int(v) for v in (~same).nonzero()[0])
        raise AssertionError(f"{what}: {int((~same).sum())} values differ from torch's .half(); first at {i}: fp32 {float(want_f32.cpu()[i])!r} -> "
                             f"{float(got.detach().cpu().view(torch.float16)[i])!r}, want {float(want_f32.cpu()[i].half())!r}")


# fp32 values at the half format's edges: around 65504 (the largest finite half; 65520 is the tie that rounds to inf), past it, the
# smallest normal (6.1035e-5), the subnormal range down to its smallest step (5.96e-8) and the ties below it, and round-to-even ties
EDGE_VALUES = [0.0, -0.0, 1.0, -1.0, 65504.0, -65504.0, 65519.99, -65519.99, 65520.0, -65520.0, 65535.0, 1.0e5, -3.0e38, 6.1035156e-5,
               6.0e-5, -3.0e-5, 1.0e-5, 1.0e-6, -1.0e-7, 5.96e-8, 2.9802322e-8, 2.99e-8, 1.0e-8, 2049.0, 2051.0, 1.0009765625, 0.33333334]


# ... and at bfloat16's: round-to-even ties at the 8-bit boundary (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6, 257 -> 256, 259 -> 260) and
# their neighbours, the largest finite bf16 (3.3895e38 = MAX_BF16; MAX_BF16 + 2^119 = 3.3962e38 is the tie that rounds to inf) up to
# the largest fp32, the smallest normal (1.1755e-38) and the subnormal range -- fp32's own -- down to bf16's smallest step
# 2^-133 = 9.1835e-41, the tie 2^-134 below it (to even: 0) and fp32's smallest step
MAX_BF16 = (2.0 - 2.0 ** -7) * 2.0 ** 127
EDGE_VALUES_BF16 = [0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, -(1.0 + 3 * 2.0 ** -8),
                    257.0, 259.0, -257.0, 258.5, MAX_BF16, -MAX_BF16, MAX_BF16 + 2.0 ** 119, -(MAX_BF16 + 2.0 ** 119),
                    MAX_BF16 + 2.0 ** 119 - 2.0 ** 104, 3.4e38, 3.4028234e38, -3.4028234e38, 2.0 ** -126, -(2.0 ** -126), 1.0e-38, -7.0e-39,
                    2.0 ** -127, 1.0e-40, 2.0 ** -133, -(2.0 ** -133), 2.0 ** -134, 2.0 ** -134 + 2.0 ** -149, 3 * 2.0 ** -134, 1.0e-41, 2.0 ** -149,
                    0.33333334]


def _bits_equal(got, want_f32, what):
    """`got` (a 16-bit container of the calling thread's build) holds exactly lp(want_f32): torch's .half() in the half build, torch's
    .bfloat16() in the bf16 build -- round to nearest even, +-inf past the tie above the largest finite value, subnormals kept (not
    flushed).  NaN compared as NaN."""
    if f16_build():
        return _half_bits_equal(got, want_f32, what)
    g = got.detach().cpu().view(torch.int16)
    w = want_f32.detach().cpu().bfloat16().view(torch.int16)
    same = (g == w) | (torch.isnan(want_f32.cpu()) & torch.isnan(got.detach().cpu().float()))
    if not bool(same.all()):
        i = tuple(int(v) for v in (~same).nonzero()[0])
        raise AssertionError(f"{what}: {int((~same).sum())} values differ from torch's .bfloat16(); first at {i}: fp32 {float(want_f32.cpu()[i])!r} -> "
                             f"{float(got.detach().cpu().float()[i])!r}, want {float(want_f32.cpu()[i].bfloat16())!r}")


def edge_values(shape, seed):
    """[shape] fp32: the edge values of the calling thread's 16-bit format first (EDGE_VALUES / EDGE_VALUES_BF16), then magnitudes
    log-uniform over 1e-9 .. 1e6 (half) / 1e-44 .. 3e38 (bf16) with random signs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(np.prod(shape))
    edges, lo, hi = (EDGE_VALUES, 1e-9, 1e6) if f16_build() else (EDGE_VALUES_BF16, 1e-44, 3e38)
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)
    v[: len(edges)] = edges
    return torch.from_numpy(v.astype(np.float32)).reshape(shape)


def case_half_conversions(dev, M=512, N=256, K=64, forms=({},)):
    """Every fp32 -> 16-bit conversion of cast_weights(_multi), cast_rows and a GEMM's 16-bit output equals lp() of the fp32 value -- in
    the half build torch's .half(), in the bf16 build torch's .bfloat16() -- bit for bit.  The GEMM's fp32 results are chosen:
    out[m, n] = x[m] * 1 + bias[n] with x 16-bit values (0, +- the largest finite one and its neighbour, the smallest normal, ...) and fp32
    biases, so that the sums straddle the largest finite value, sit on round-to-even ties and fill the subnormal range; `forms`:
    ops.options of the kernels to take (each its own epilogue conversion)."""
    w = edge_values((70, 130), 300)
    d, dt_ = ops.cast_weights(w.to(dev), torch.bfloat16, want=True, want_t=True)
    _bits_equal(d, w, "cast_weights")
    _bits_equal(dt_, w.t(), "cast_weights transposed")
    ws = [edge_values((64, 256), 301), edge_values((33, 70), 302)]      # the quad path and the element-wise one
    for t, (o, ot) in zip(ws, ops.cast_weights_multi([t.to(dev) for t in ws], torch.bfloat16, want=True, want_t=True)):
        _bits_equal(o, t, "cast_weights_multi")
        _bits_equal(ot, t.t(), "cast_weights_multi transposed")
    r = ops.cast_rows(w.to(dev), torch.bfloat16, ld_dst=192)
    _bits_equal(r[:, :130], w, "cast_rows")
    assert not r[:, 130:].view(torch.int16).any(), "cast_rows pad must be zero"
    if f16_build():
        xs = torch.tensor([0.0, 65504.0, -65504.0, 65472.0, 1.0, -1.0, 6.1035156e-5, -3.0517578e-5, 0.5, 1024.0, 65440.0, -65472.0])
        bs = torch.tensor([0.0, 16.0, 15.99, 31.99, 32.0, 47.99, 48.0, -16.0, -15.99, 1.0e-7, -1.0e-7, 5.0e-8, 3.0e-8, 6.0e-5, 1.0e-5, 7.0e4])
        small = 1e-3
    else:
        # (MAX_BF16 + 2^119 is the tie to inf; 1 + 2^-8 and 1 + 3 * 2^-8 the ties to 1 and to 1 + 2^-6; 256 + 1 / + 3 those at 256)
        u = 2.0 ** 119
        xs = torch.tensor([0.0, MAX_BF16, -MAX_BF16, MAX_BF16 - 2 * u, 1.0, -1.0, 2.0 ** -126, -(2.0 ** -127), 0.5, 256.0, 2.0 ** -133, -256.0])
        bs = torch.tensor([0.0, u, 0.999 * u, 1.001 * u, 3 * u, -u, -0.999 * u, 2.0 ** -8, 3 * 2.0 ** -8, 2.0 ** -8 + 2.0 ** -20, -(2.0 ** -8), 1.0, 3.0,
                           1.0e-40, -1.0e-40, 2.0 ** -134, 4.7e-41, 1.0e-38, -5.0e-39, 3.4e38])
        small = 1e-37
    x = torch.where(torch.arange(M) < 2 * len(xs), xs[torch.arange(M) % len(xs)], 0.0)     # (the rest: +0 + bias)
    bias = torch.cat([bs, edge_values((N - len(bs),), 303) * small])
    a = torch.zeros(M, K)
    a[:, 0] = x
    b = torch.zeros(N, K)
    b[:, 0] = 1.0
    want = x[:, None] + bias[None, :]          # the fp32 sums (one rounding, as the epilogue's acc + bias)
    for kw in forms:
        with ops.options(**kw):
            c = ops.gemm_nt(lp(a).to(dev), lp(b).to(dev), bias.to(dev), out_dtype=torch.bfloat16)
        _bits_equal(c, want, f"gemm 16-bit output {kw}")


def _finite_except(t, bad, what):
    """Every element of `t` (a container or fp32) where `bad` is True is inf or NaN, every other one finite."""
    v = f32(t.detach()).cpu()
    fin = torch.isfinite(v)
    assert not bool(fin[bad].any()), f"{what}: {int(fin[bad].sum())} of {int(bad.sum())} outputs fed by an inf / NaN are finite"
    assert bool(fin[~bad].all()), f"{what}: {int((~fin[~bad]).sum())} outputs no inf / NaN reaches are not finite"


def case_nonfinite(dev, M=144, N=200, K=128, B=2, Ntok=40, rows=11, gemm_forms=({},), tn_forms=({},), attn_forms=({},)):
    """An inf or NaN in one 16-bit operand row reaches every output it feeds as inf / NaN -- never a finite value, never 0 -- and no other:
    the NT dgrad GEMM (fp32 and 16-bit output), the TN wgrad GEMM and its column sums (split-K, the workspace combine), the attention
    backward with one inf in dO (delta = rowsum(dO * O), dS = P * (dP - delta)) and layernorm_bwd.  GradScaler finds an overflowed step
    only through this.  *_forms: ops.options of the kernel forms to take."""
    inf, nan = float("inf"), float("nan")
    a = rnd((M, K), 400)
    a[3, 5], a[7, 9] = inf, nan
    b = rnd((N, K), 401)
    bad = torch.zeros(M, N, dtype=torch.bool)
    bad[3], bad[7] = True, True
    for kw in gemm_forms:
        with ops.options(**kw):
            for od in (torch.float32, torch.bfloat16):
                _finite_except(ops.gemm_nt(lp(a).to(dev), lp(b).to(dev), None, out_dtype=od), bad, f"gemm_nt -> {od} {kw}")
    # wgrad: out[m, n] = sum_k a[k, m] b[k, n], colsum[m] = sum_k a[k, m]
    ta, tb = rnd((K, M), 402), rnd((K, N), 403)
    ta[4, 10] = inf
    tb[6, 20] = nan
    bad = torch.zeros(M, N, dtype=torch.bool)
    bad[10], bad[:, 20] = True, True
    bad_cs = torch.zeros(M, dtype=torch.bool)
    bad_cs[10] = True
    for kw in tn_forms:
        for sk in (1, 0):
            with ops.options(**kw):
                out = torch.zeros((M, N), dtype=torch.float32, device=dev)
                cs = torch.zeros(M, dtype=torch.float32, device=dev)
                ops.gemm_tn(lp(ta).to(dev), lp(tb).to(dev), out, colsum=cs, split_k=sk)
            _finite_except(out, bad, f"gemm_tn split_k={sk} {kw}")
            _finite_except(cs, bad_cs, f"gemm_tn colsum split_k={sk} {kw}")
    # attention backward: dO[clip 0, query 5, head 2, d 7] = inf
    qkv = lp(rnd((B * Ntok, 2304), 404))
    dout = rnd((B * Ntok, 768), 405)
    dout[5, 2 * 64 + 7] = inf
    bad = torch.zeros(B, Ntok, 3, 12, 64, dtype=torch.bool)
    bad[0, 5, 0, 2] = True          # dQ of that query, head 2
    bad[0, :, 1, 2] = True          # dK of every key of clip 0, head 2
    bad[0, :, 2, 2, 7] = True       # dV[:, d = 7] of every key of clip 0, head 2
    bad = bad.reshape(B * Ntok, 2304)
    for kw in attn_forms:
        with ops.options(**kw):
            o, lse = ops.attn_fwd(qkv.to(dev), B, Ntok, 0.125, save_lse=True)
            d = ops.attn_bwd(qkv.to(dev), o, lp(dout).to(dev), lse, B, Ntok, 0.125)
        _finite_except(d, bad, f"attention backward {kw}")
    # layernorm backward: dy[3, 11] = inf
    x = rnd((rows, 768), 406, 2.0) + 0.3
    g, bb = 1.0 + rnd((768,), 407, 0.1), rnd((768,), 408, 0.1)
    _, mean, rstd = ops.layernorm_fwd(x.to(dev), g.to(dev), bb.to(dev), 1e-6, torch.bfloat16, save_stats=True)
    dy = rnd((rows, 768), 409)
    dy[3, 11] = inf
    dg, db = torch.zeros(768, device=dev), torch.zeros(768, device=dev)
    dx, dx_lp = ops.layernorm_bwd(lp(dy).to(dev), x.to(dev), g.to(dev), mean, rstd, None, dg, db, lp_dtype=torch.bfloat16)
    bad = torch.zeros(rows, 768, dtype=torch.bool)
    bad[3] = True
    _finite_except(dx, bad, "layernorm_bwd dx")
    _finite_except(dx_lp, bad, "layernorm_bwd dx (16-bit)")
    bad_c = torch.zeros(768, dtype=torch.bool)
    bad_c[11] = True
    _finite_except(dg, bad_c, "layernorm_bwd dgamma")
    _finite_except(db, bad_c, "layernorm_bwd dbeta")


# ------------------------------------------------------------------------------------- the memory contract (include/maest_hip.h, "Conventions")
# These cases run inside `with tests.guard.guarded():` only: the buffers ops allocates then come back filled with the guard's pattern, so
# "not written" is visible bit for bit, and every call is checked for accesses outside its operands.  No tolerance anywhere: bit patterns.
def _guard():
    from tests import guard
    assert guard.guarded._active is not None, "the memory-contract cases need tests.guard.guarded()"
    return guard


def case_contract_attention_rows(dev, dtype, B, N, seed=26):
    """maest_attn_fwd_rows with q_rows = 2: rows >= 32 of `out` and `lse` of EVERY clip are not written; the rows of the 32-row tile are.
    maest_scatter_head_rows: rows >= n_pad of every clip untouched, rows [n_head, n_pad) exactly zero, for n_pad in {2, 32, N}."""
    G = _guard()
    qkv = lp(rnd((B * N, 2304), seed, 1.0), dtype).to(dev)
    out, lse = ops.attn_fwd(qkv, B, N, 0.125, save_lse=True, q_rows=2)
    nv = min(32, N)
    o3 = out.reshape(B, N, 768)
    assert bool(G.untouched(o3[:, nv:]).all()), "attn_fwd_rows wrote output rows beyond the 32-row tile of the head tokens"
    assert bool(G.untouched(lse[:, :, nv:]).all()), "attn_fwd_rows wrote lse beyond the 32-row tile of the head tokens"
    assert not bool(G.untouched(o3[:, :nv]).any()) and not bool(G.untouched(lse[:, :, :nv]).any()), "rows of the head tokens' tile left unwritten"
    assert bool(torch.isfinite(f32(o3[:, :nv])).all()) and bool(torch.isfinite(lse[:, :, :nv]).all())
    comp = lp(rnd((B * 2, 768), seed + 1), dtype).to(dev)
    for n_pad in sorted({2, nv, N}):
        back = ops.scatter_head_rows(comp, B, N, 2, n_pad).reshape(B, N, 768)
        assert torch.equal(back[:, :2], comp.reshape(B, 2, 768)), f"scatter_head_rows n_pad={n_pad}: head rows"
        assert not bool(back[:, 2:n_pad].contiguous().view(torch.int16 if dtype != torch.float32 else torch.int32).any()), f"n_pad={n_pad}: rows [2, n_pad) must be zero"
        assert bool(G.untouched(back[:, n_pad:]).all()), f"scatter_head_rows n_pad={n_pad}: rows >= n_pad must stay untouched"


def case_contract_fully_written(dev, B=3, N=7):
    """maest_head_pool_bwd: every row >= 2 of dx exactly zero (written, not left); maest_embed_pool_bwd and maest_patch_im2col_bwd: fully
    written, no fill pattern left (the latter with its int32 workspace at exactly the documented minimum, which ops allocates)."""
    G = _guard()
    x = rnd((B, N, 768), 50, 1.5).to(dev)
    g, b = (1.0 + rnd((768,), 51, 0.1)).to(dev), rnd((768,), 52, 0.1).to(dev)
    cls, dist, feat, mean, rstd = ops.head_pool_fwd(x, g, b, 1e-6, save_stats=True)
    for t in (cls, dist, feat, mean, rstd):
        assert not bool(G.untouched(t).any()), "head_pool_fwd left an output element unwritten"
    dg, db = torch.zeros(768, device=dev), torch.zeros(768, device=dev)
    dx = ops.head_pool_bwd(rnd((B, 768), 53).to(dev), rnd((B, 768), 54).to(dev), rnd((B, 768), 55).to(dev), x, g, mean, rstd, dg, db)
    assert not bool(dx[:, 2:].contiguous().view(torch.int32).any()), "head_pool_bwd: rows >= 2 of dx must be exactly zero"
    assert not bool(G.untouched(dx[:, :2]).any())
    dxe, lpe = ops.embed_pool_bwd(rnd((B, 3 * 768), 56).to(dev), N, lp_dtype=torch.bfloat16)
    assert not bool(G.untouched(dxe).any()) and not bool(G.untouched(lpe).any()), "embed_pool_bwd left rows unwritten"
    Fdim, T, stride = 42, 46, (10, 10)
    Fp, Tp = (Fdim - 16) // 10 + 1, (T - 16) // 10 + 1
    tok = torch.tensor([(f, t) for f in range(Fp) for t in range(Tp) if (f, t) != (1, 2)], dtype=torch.int32).to(dev)      # one patch dropped
    perm = torch.tensor([2, 0, 1], dtype=torch.int32).to(dev)
    lam = torch.tensor([0.7, 0.35, 0.9]).to(dev)
    for dt, xdt in ((torch.float32, torch.float32), (torch.bfloat16, torch.float16)):
        dcols = lp(rnd((3 * tok.shape[0], 256), 57), dt).to(dev)
        for mix in (False, True):
            dxp = ops.patch_im2col_bwd(dcols, (3, Fdim, T), xdt, tok, perm=perm if mix else None, lam=lam if mix else None, stride=stride)
            assert not bool(G.untouched(dxp).any()), f"patch_im2col_bwd left samples unwritten ({dt}, mixup {mix})"
            assert bool(torch.isfinite(dxp.float()).all())


def case_contract_padded_leading_dims(dev, dtype, M, N, K, tn_K=None, pad=64):
    """Leading dimensions wider than the logical row: the pad columns of an output are bitwise untouched (or exactly zero where the header
    says zero), pad columns of an INPUT -- here holding the NaN pattern -- never reach a result; each result is bit-equal to the dense call."""
    G = _guard()
    it = torch.int32 if dtype == torch.float32 else torch.int16

    def wide(rows, cols, dt, src=None):
        w = G.fill_pattern_(torch.empty((rows, cols + pad), dtype=dt, device=dev))
        if src is not None:
            w[:, :cols] = src
        return w

    a, b = lp(rnd((M, K), 70), dtype).to(dev), lp(rnd((N, K), 71) * 0.1, dtype).to(dev)
    bias = rnd((N,), 72).to(dev)
    # outputs as column slices (ldc = ld_aux = N + pad)
    aux_d = torch.empty((M, N), dtype=dtype, device=dev)
    c_d = ops.gemm_nt(a, b, bias, out_dtype=dtype, epi=ops.EPI_GELU, aux_out=aux_d)
    cw, auxw = wide(M, N, dtype), wide(M, N, dtype)
    ops.gemm_nt(a, b, bias, out=cw[:, :N], epi=ops.EPI_GELU, aux_out=auxw[:, :N])
    assert torch.equal(cw[:, :N].contiguous().view(it), c_d.view(it)), "gemm_nt into a column slice differs from the dense call"
    assert torch.equal(auxw[:, :N].contiguous().view(it), aux_d.view(it)), "gemm_nt aux_out into a column slice differs from the dense call"
    assert bool(G.untouched(cw[:, N:]).all()) and bool(G.untouched(auxw[:, N:]).all()), "gemm_nt wrote pad columns of C / aux_out"
    # operands as column slices (lda = ldb = K + pad), NaN pattern in the pad
    c_f = ops.gemm_nt(a, b, bias, out_dtype=torch.float32)
    c_s = ops.gemm_nt(wide(M, K, dtype, a)[:, :K], wide(N, K, dtype, b)[:, :K], bias, out_dtype=torch.float32)
    assert torch.equal(c_s.view(torch.int32), c_f.view(torch.int32)), "gemm_nt on column-slice operands differs from the dense call"
    # wgrad with ldc > N
    Kt = tn_K or M
    ta, tb = lp(rnd((Kt, 136), 73), dtype).to(dev), lp(rnd((Kt, 200), 74), dtype).to(dev)
    o_d = torch.zeros((136, 200), dtype=torch.float32, device=dev)
    ops.gemm_tn(ta, tb, o_d, split_k=1)
    ow = wide(136, 200, torch.float32, 0.0)
    ops.gemm_tn(ta, tb, ow[:, :200], split_k=1)
    assert torch.equal(ow[:, :200].contiguous().view(torch.int32), o_d.view(torch.int32)), "gemm_tn into a column slice differs from the dense call"
    assert bool(G.untouched(ow[:, 200:]).all()), "gemm_tn wrote pad columns of C"
    # cast_rows / transpose: pad columns of dst are ZERO by the header
    src = rnd((70, 130), 75).to(dev)
    r = ops.cast_rows(src, dtype, ld_dst=192)
    assert torch.equal(r[:, :130].contiguous().view(it), lp(src.cpu(), dtype).to(dev).view(it)) and not bool(r[:, 130:].contiguous().view(it).any()), "cast_rows pad"
    s16 = lp(src.cpu(), dtype).to(dev)
    t = ops.transpose(s16, 128)
    assert torch.equal(t[:, :70].contiguous().view(it), s16.t().contiguous().view(it)) and not bool(t[:, 70:].contiguous().view(it).any()), "transpose pad"


def case_contract_ragged_tables(dev):
    """maest_logmel_rows_f16 / maest_resample: the last track ends exactly at the end of the input buffer, its rows / outputs exactly at the
    end of the output; then an n_blocks that over-covers the table, and an output with rows no track covers: nothing outside the tracks'
    rows changes, and the covered rows equal the first call's bit for bit."""
    G = _guard()
    from maest_amd import mel_extractor as X
    from maest_amd.melspectrogram import MelConstants
    consts = MelConstants(dev, 16000, 512, 96, norm_mean=0.0, norm_std=0.5)
    lens = [300, 64 * 256 + 77, 2563]                      # offsets 0, 320 (64-sample grid), then 3 past the grid: the element-wise fetch
    offs = [0, 320, 320 + 16512 + 3]
    buf = torch.zeros(offs[-1] + lens[-1])                  # the last track ends exactly at the buffer's end
    for o, n, s in zip(offs, lens, (1, 2, 3)):
        buf[o:o + n] = rnd((n,), 500 + s, 0.3)
    counts = [1 + n // 256 for n in lens]
    r0 = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    tab = torch.tensor([[o, n, 0, c, r] for o, n, c, r in zip(offs, lens, counts, r0)], dtype=torch.int64).to(dev)
    bs = torch.from_numpy(X._blocks(counts, 64)).to(dev)
    total = int(sum(counts))
    rows = ops.logmel_rows_f16(buf.to(dev), tab, bs, int(bs[-1]), total, consts)
    assert not bool(G.untouched(rows).any()) and bool(torch.isfinite(rows.float()).all())
    more = ops.logmel_rows_f16(buf.to(dev), tab, bs, int(bs[-1]) + 3, total + 5, consts)          # blocks past the table, rows past the tracks
    assert torch.equal(more[:total].view(torch.int16), rows.view(torch.int16)) and bool(G.untouched(more[total:]).all())
    # resampler 44.1 kHz -> 16 kHz (160 / 441)
    filt = X._filter(44100, torch.device(dev))
    ilen = [4417, 1000, 37]
    olen = [filt.out_length(n) for n in ilen]
    x = rnd((sum(ilen),), 600, 0.3).to(dev)
    ioff = np.concatenate([[0], np.cumsum(ilen)[:-1]]).astype(np.int64)
    ooff = np.concatenate([[0], np.cumsum(olen)[:-1]]).astype(np.int64)
    rtab = torch.from_numpy(np.stack([ioff, np.asarray(ilen, np.int64), ooff, np.asarray(olen, np.int64)], 1)).to(dev)
    rbs = torch.from_numpy(X._blocks(olen, 256)).to(dev)
    out = G.fill_pattern_(torch.empty(sum(olen), dtype=torch.float32, device=dev))
    ops.resample(x, rtab, rbs, int(rbs[-1]), filt, out)
    assert not bool(G.untouched(out).any()) and bool(torch.isfinite(out).all())
    out2 = G.fill_pattern_(torch.empty(sum(olen) + 7, dtype=torch.float32, device=dev))
    ops.resample(x, rtab, rbs, int(rbs[-1]) + 2, filt, out2)
    assert torch.equal(out2[:sum(olen)], out) and bool(G.untouched(out2[sum(olen):]).all())


def case_entries_without_a_wrapper(dev, dtype=torch.bfloat16, B=2, N=40):
    """The entry points ops reaches only through a more general sibling -- maest_gemm_tn (maest_gemm_tn_ws), maest_attn_fwd / maest_attn_bwd
    (the _rows forms), maest_layernorm_bwd (_headres), maest_patch_im2col (_strided) -- called directly, bit for bit against the sibling;
    and the two in-place scalers."""
    p, s, F32c, code = ops._p, ops._s, ops.DT[torch.float32], ops.DT[dtype]
    new = lambda *shape, dt=torch.float32: ops.torch.empty(shape, dtype=dt, device=dev)      # (ops.torch: filled by an active guard)
    ta, tb = lp(rnd((150, 136), 80), dtype).to(dev), lp(rnd((150, 200), 81), dtype).to(dev)
    want, cs_want = torch.zeros((136, 200), device=dev), torch.zeros(136, device=dev)
    ops.gemm_tn(ta, tb, want, colsum=cs_want, split_k=1)
    got, cs = torch.zeros((136, 200), device=dev), torch.zeros(136, device=dev)
    ops.call("maest_gemm_tn", p(ta), 136, p(tb), 200, code, p(got), 200, 136, 200, 150, p(cs), 1, s(ta))
    assert torch.equal(got, want) and torch.equal(cs, cs_want), "maest_gemm_tn differs from maest_gemm_tn_ws without a workspace"
    qkv = lp(rnd((B * N, 2304), 82), dtype).to(dev)
    o_w, lse_w = ops.attn_fwd(qkv, B, N, 0.125, save_lse=True)
    o, lse = new(B * N, 768, dt=dtype), new(B, 12, N)
    ops.call("maest_attn_fwd", p(qkv), p(o), p(lse), B, N, code, 0.125, s(qkv))
    assert torch.equal(o.view(torch.int16), o_w.view(torch.int16)) and torch.equal(lse, lse_w), "maest_attn_fwd differs from maest_attn_fwd_rows(q_rows = N)"
    dout = lp(rnd((B * N, 768), 83), dtype).to(dev)
    d_w = ops.attn_bwd(qkv, o_w, dout, lse_w, B, N, 0.125)
    d, delta = new(B * N, 2304, dt=dtype), new(B, 12, N)
    ops.call("maest_attn_bwd", p(qkv), p(o_w), p(dout), p(lse_w), p(delta), p(d), B, N, code, 0.125, s(qkv))
    assert torch.equal(d.view(torch.int16), d_w.view(torch.int16)), "maest_attn_bwd differs from maest_attn_bwd_rows(q_rows = N)"
    rows = 11
    x, g, b = (rnd((rows, 768), 84, 2.0) + 0.3).to(dev), (1.0 + rnd((768,), 85, 0.1)).to(dev), rnd((768,), 86, 0.1).to(dev)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-6, dtype, save_stats=True)
    dy, dres = lp(rnd((rows, 768), 87), dtype).to(dev), rnd((rows, 768), 88).to(dev)
    dg_w, db_w = torch.zeros(768, device=dev), torch.zeros(768, device=dev)
    dx_w, lp_w = ops.layernorm_bwd(dy, x, g, mean, rstd, dres, dg_w, db_w, lp_dtype=dtype)
    dg, db, dx, dxl = torch.zeros(768, device=dev), torch.zeros(768, device=dev), new(rows, 768), new(rows, 768, dt=dtype)
    ops.call("maest_layernorm_bwd", p(dy), 768, code, p(x), 768, p(g), p(mean), p(rstd), p(dres), p(dx), p(dxl), code, p(dg), p(db), rows, 768, s(x))
    assert torch.equal(dx, dx_w) and torch.equal(dxl.view(torch.int16), lp_w.view(torch.int16)), "maest_layernorm_bwd differs from the _headres form with n_head = 0"
    close(dg, dg_w, 1e-4, 1e-4 * math.sqrt(rows), "maest_layernorm_bwd dgamma (atomics)")
    xm = rnd((2, 96, 66), 89).to(dev)
    tok = torch.stack(torch.meshgrid(torch.arange(9), torch.arange(6), indexing="ij"), -1).reshape(-1, 2).to(torch.int32).contiguous().to(dev)
    c_w = ops.patch_im2col(xm, tok, dtype)
    c = new(2 * 54, 256, dt=dtype)
    ops.call("maest_patch_im2col", p(xm), F32c, 2, 96, 66, None, None, p(tok), 54, None, 0, None, 0, p(c), code, s(xm))
    assert torch.equal(c.view(torch.int16), c_w.view(torch.int16)), "maest_patch_im2col differs from the strided form at (10, 10)"
    v = rnd((1000,), 90)
    close(ops.affine_(v.clone().to(dev), 4.5, 5.0), (v + 4.5) / 5.0, 1e-6, 1e-7, "affine")
    close(ops.scale_dev_(v.clone().to(dev), torch.tensor([0.25]).to(dev)), v * 0.25, 0, 0, "scale by a device factor")
