"""The LayerNorm, head-pool and loss kernels on rows where fp32 is hard, shared by the emulator tests, the GPU tests
and tests/test_norm_gate_cpu.py (which feeds the same gates an fp32 restatement of the kernels' arithmetic, and that restatement with defects).

Rows (768 columns), each family a block of rows inside ONE tensor (inputs()):
    plain          2 N + 0.3                          the family of kernel_cases.case_layernorm: the control
    offset         300 + 0.5 N                        |mean| = 600 sigma
    outlier        N; columns 100, 400, 767 x 1000, column 300 + 2000
    near-constant  c + s N, (c, s) in NEAR            the variance straddles both values of eps; s = 0: rstd = 1 / sqrt(eps), y = beta
    tiny           1e-4 N
    huge           1e4 N + 3e3
Every entry point runs with eps = 1e-6 and eps = 1e-5 (norm.hip:2-3: the model passes both).

References are fp64 on the same fp32 inputs; every bound counts roundings of u = 2^-24 (half an fp32 ulp of 1).

Forward (norm.hip:22-32 ln_stats, its copies in regularise.hip:160-169 and the row kernels' (v - mu) * rs * g + b).  Per row mu, s' = sqrt(var + eps),
A = mean |x|:
    e_mu    = 20 u A                                  a 12-term lane sum, six butterfly adds, one multiply
    rho     = 32 u + (e_mu / s')^2 / 2                a mean error enters the variance in second order only; 768 squares summed, halved by the
                                                      root, then the root and the division
    mean    |got - mu| <= e_mu + u |mu|
    rstd    |got - 1 / s'| <= (rho + u) / s'
    y       delta_y = |gamma| / s' (e_mu + |x - mu| (rho + 4 u)) + 2 u (|y| + |beta|)
fp32 y: kernel_cases.close32; 16-bit y: close16; MAEST_SPLIT3_A rows: hi + lo within delta_y + 2^-16 |y|, the two hi thirds equal (bf16 build).
fwd_ref() asserts max delta_y / max |y| <= 1e-3 in every family: no family passes because its bound is wide.

Backward (norm.hip:166-187; the saved fp32 mean / rstd are INPUTS of the reference).  xh = (x - mean) rstd, gg = dy gamma, s1 = mean(gg),
s2 = mean(gg xh):
    delta_dx = rstd (4 u |gg| + 22 u mean |gg| + |xh| (24 u mean |gg xh| + 6 u |s2|) + 2 u |s1|) + 2 u |dx|      (+ u |dres|)
    dgamma / dbeta: deterministic_cases.sum_bound on the fp64 terms, n = rows + 3
head_pool_bwd forms d = d_cls + d_feat / 2 first (norm.hip:334-335, one more rounding of dy):  + rstd u (|gg| + mean |gg| + |xh| mean |gg xh|).

Loss (misc.hip:227-296), logits tiled from Z_VALUES, hard targets and mixup-softened ones:
    loss     finite, within weight / total (sum 4 u (max(z, 0) + |z t| + log1p e^-|z|) + 2 n u sum |term|), n = the documented add chain
             (misc.hip:221-226): terms per thread + 6 + waves per workgroup + ceil(blocks / 64) + 6
    dlogits  (4 u s(z) + u |s(z) - t|) weight / total, and the terms that bound leaves uncounted:
             2^-126 weight / total           expf(-z) is inf above z = 88.7 and 1 / (1 + .) subnormal before: s(z) < 2^-126 may read 0     misc.hip:284
             2^-149                          results below 2^-126 lie on the subnormal grid
             mixup-softened targets only (hard targets with weight 1 or 0.5 scale s - t = 0, +-1 or a value next to them, and keep the bound as stated):
             2 u (|y| l + |y_p| (1 - l)) weight / total   the mixed target: 1 - l rounded, the sum rounded                                 misc.hip:282
             3 u |s(z) - t| weight / total   inv = 1 / total rounded, and the two multiplies weight * (.) * inv                            misc.hip:276,285
    saturated (fp32 sigmoid exactly 0 or 1: z <= -89, z >= 20): bit for bit fl(fl(weight fl(s - t)) fl(1 / total)) -- for a weight that is a
             power of two and an exact s - t, ONE rounding of (s - t) weight times the rounded reciprocal
    sigmoid_mean within (rows + 4) u of the fp64 mean
"""
import math

import numpy as np
import torch

from maest_amd import ops
from tests import deterministic_cases as DC
from tests import regulariser_cases as RC
from tests.kernel_cases import _bits_equal, close16, close32, f16_build, f32, lp, rnd

U = 2.0 ** -24
COLS = 768
EPS = (1e-6, 1e-5)
FAMILIES = ("plain", "offset", "outlier", "near-constant", "tiny", "huge")
NEAR = ((0.0, 0.0), (0.0, 3e-4), (0.0, 1e-3), (0.0, 3e-3), (0.01, 1e-3), (0.01, 0.0))
OUTLIER_COLS, SHIFT_COL = (100, 400, 767), 300
SEED = 0x9E3779B97F4A7C15
INV_COLS = float(np.float32(1.0) / np.float32(COLS))      # the kernels' 1.0f / LN_COLS


# ------------------------------------------------------------------------------------------------ inputs
def family_rows(name, n, seed):
    z = rnd((n, COLS), seed)
    if name == "plain":
        return z * 2.0 + 0.3
    if name == "offset":
        return 300.0 + 0.5 * z
    if name == "outlier":
        x = z.clone()
        x[:, list(OUTLIER_COLS)] *= 1000.0
        x[:, SHIFT_COL] += 2000.0
        return x
    if name == "near-constant":
        c = torch.tensor([NEAR[i % len(NEAR)][0] for i in range(n)], dtype=torch.float32)[:, None]
        s = torch.tensor([NEAR[i % len(NEAR)][1] for i in range(n)], dtype=torch.float32)[:, None]
        return c + s * z
    if name == "tiny":
        return 1e-4 * z
    if name == "huge":
        return 1e4 * z + 3e3
    raise KeyError(name)


def inputs(per_family, loose=("plain", "offset", "outlier"), seed=700):
    """-> x [len(FAMILIES) * per_family + len(loose), 768], fam (the family index of every row), gamma, beta."""
    blocks = [family_rows(f, per_family, seed + i) for i, f in enumerate(FAMILIES)]
    blocks += [family_rows(f, 1, seed + 50 + i) for i, f in enumerate(loose)]
    fam = [i for i in range(len(FAMILIES)) for _ in range(per_family)] + [FAMILIES.index(f) for f in loose]
    return torch.cat(blocks), torch.tensor(fam), 1.0 + rnd((COLS,), seed + 90, 0.1), rnd((COLS,), seed + 91, 0.1)


def offset_delta(x, fam, dtype, seed=720):
    """A delta (in the operand type) that turns every plain row into an offset row and moves the others by half their own spread."""
    d = 0.5 * x[torch.arange(x.shape[0]).roll(1)] * (fam == fam.roll(1))[:, None]
    d[fam == 0] = 300.0 + 0.5 * rnd((int((fam == 0).sum()), COLS), seed)
    return lp(d, dtype)


# ------------------------------------------------------------------------------------------------ references and bounds
def fwd_ref(x, g, b, eps, fam=None):
    """fp64 LayerNorm of the fp32 rows `x` and the bounds of the module docstring."""
    x64, g64, b64 = x.double(), g.double(), b.double()
    mu = x64.mean(1)
    xc = x64 - mu[:, None]
    sig = torch.sqrt((xc * xc).mean(1) + float(np.float32(eps)))          # (the kernels receive eps as a float)
    e_mu = 20 * U * x64.abs().mean(1)
    rho = 32 * U + 0.5 * (e_mu / sig) ** 2
    y = xc / sig[:, None] * g64 + b64
    d_y = g64.abs() / sig[:, None] * (e_mu[:, None] + xc.abs() * (rho[:, None] + 4 * U)) + 2 * U * (y.abs() + b64.abs())
    if fam is not None:
        for i, name in enumerate(FAMILIES):
            m = fam == i
            if bool(m.any()):
                r = float(d_y[m].max() / y[m].abs().max())
                assert r <= 1e-3, f"family {name}: max delta_y / max |y| = {r:.2e}: the bound is too wide to gate anything"
    return dict(mean=mu, rstd=1.0 / sig, y=y, d_mean=e_mu, d_rstd=rho / sig, d_y=d_y)


def bwd_ref(dy, x, g, mean, rstd, dres=None, extra_dy_rounding=False):
    """fp64 LayerNorm backward from the fp32 inputs (saved statistics included) -> dx, delta_dx, and the terms of dgamma / dbeta."""
    dy, x, g, mean, rstd = (t.detach().cpu().double() for t in (dy, x, g, mean, rstd))
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = dy * g
    s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    mg, mgx = gg.abs().mean(1, keepdim=True), (gg * xh).abs().mean(1, keepdim=True)
    dx = rstd[:, None] * (gg - s1 - xh * s2)
    delta = rstd[:, None] * (4 * U * gg.abs() + 22 * U * mg + xh.abs() * (24 * U * mgx + 6 * U * s2.abs()) + 2 * U * s1.abs()) + 2 * U * dx.abs()
    if extra_dy_rounding:
        delta = delta + rstd[:, None] * U * (gg.abs() + mg + xh.abs() * mgx)
    if dres is not None:
        dres = dres.detach().cpu().double()
        dx, delta = dx + dres, delta + U * dres.abs()
    return dx, delta, dy * xh, dy


def per_family(gate, fam, got, ref, delta, what):
    """Run `gate` (close32 / close16) family by family over the rows -> {family: worst err / bound}."""
    got = got.detach().cpu()
    out = {}
    for i, name in enumerate(FAMILIES):
        m = fam == i
        if bool(m.any()):
            out[name] = gate(got[m], ref[m], delta[m], f"{what} [{name}]")
    return out


def merge(into, new, key):
    for f, r in new.items():
        into[(key, f)] = max(into.get((key, f), 0.0), r)


def check_split3(o, y, d_y, fam, what):
    """MAEST_SPLIT3_A rows [ hi | hi | lo ] as epilogue_cases.check_gelu treats them."""
    o = o.detach().cpu()
    assert o.shape == (y.shape[0], 3 * COLS) and torch.equal(o[:, :COLS].view(torch.int16), o[:, COLS:2 * COLS].view(torch.int16)), \
        f"{what}: the two hi thirds of the split rows differ"
    hi, lo = f32(o[:, :COLS]).double(), f32(o[:, 2 * COLS:]).double()
    lim = d_y + 2.0 ** -16 * y.abs()
    err = (hi + lo - y).abs()
    out = {}
    for i, name in enumerate(FAMILIES):
        m = fam == i
        if bool(m.any()):
            bad = ~(err[m] <= lim[m])
            ratio = torch.nan_to_num(err[m] / lim[m].clamp_min(1e-300), nan=float("inf"))
            assert not bool(bad.any()), f"{what} [{name}]: hi + lo of {int(bad.sum())} elements outside delta_y + 2^-16 |y|; worst ratio {float(ratio.max()):.3f}"
            out[name] = float(ratio.max())
    per_family(close16, fam, o[:, :COLS], y, d_y, f"{what}: hi third")
    return out


def check_fwd(y, mean, rstd, x_in, g, b, eps, fam, what, ref=None):
    """The forward gates on one entry point's outputs for the fp32 rows it normalised (`x_in`).  y: fp32, 16-bit or (SPLIT3) [rows, 2304]."""
    r = fwd_ref(x_in.detach().cpu(), g, b, eps, fam) if ref is None else ref
    worst = {}
    if y is not None:
        if y.shape[1] == 3 * COLS:
            merge(worst, check_split3(y, r["y"], r["d_y"], fam, f"{what}: y split3"), "y split3")
        else:
            gate = close16 if y.dtype == torch.bfloat16 else close32
            merge(worst, per_family(gate, fam, y, r["y"], r["d_y"], f"{what}: y"), "y")
    if mean is not None:
        merge(worst, per_family(close32, fam, mean, r["mean"], r["d_mean"], f"{what}: mean"), "mean")
        merge(worst, per_family(close32, fam, rstd, r["rstd"], r["d_rstd"], f"{what}: rstd"), "rstd")
    return worst


def check_bwd(dx, dx_lp, dg, db, dy, x, g, mean, rstd, dres, fam, what, n=None, extra_dy_rounding=False):
    dx64, delta, tg, tb = bwd_ref(f32(dy) if dy.dtype == torch.bfloat16 else dy, x, g, mean, rstd, dres, extra_dy_rounding)
    worst = {}
    merge(worst, per_family(close32, fam, dx, dx64, delta, f"{what}: dx"), "dx")
    if dx_lp is not None:
        if dx_lp.dtype == torch.bfloat16:
            merge(worst, per_family(close16, fam, dx_lp, dx64, delta, f"{what}: dx_lp"), "dx_lp")
            _bits_equal(dx_lp, dx.detach().cpu(), f"{what}: dx_lp = the 16-bit rounding of the dx of the same kernel")
        else:
            assert torch.equal(dx_lp, dx), f"{what}: fp32 dx_lp differs from dx"
    if dg is not None:
        n = x.shape[0] + 3 if n is None else n
        DC.sum_bound(dg.cpu(), tg.sum(0), tg.abs().sum(0), n, f"{what}: dgamma")
        DC.sum_bound(db.cpu(), tb.sum(0), tb.abs().sum(0), n, f"{what}: dbeta")
    return worst


def show(name, worst):
    """Print {(output, family): worst err / bound}, one line per output."""
    outs = sorted({k[0] for k in worst})
    for o in outs:
        print(f"{name}: {o}: " + ", ".join(f"{f} {worst[(o, f)]:.3f}" for f in FAMILIES if (o, f) in worst))
    return worst


# ------------------------------------------------------------------------------------------------ the fp32 restatement
def _lanes(x):
    """[R, 768] -> [R, 64 lanes, 12]: lane l holds columns i * 256 + 4 l + e in the order (i, e) (norm.hip:15-21)."""
    R = x.shape[0]
    return x.reshape(R, 3, 64, 4).permute(0, 2, 1, 3).reshape(R, 64, 12)


def _unlanes(v):
    R = v.shape[0]
    return v.reshape(R, 64, 3, 4).permute(0, 2, 1, 3).reshape(R, COLS)


def _wave_sum(s):
    """common.h wave_sum: v += shfl_xor(v, m) for m = 32 .. 1 (every lane ends with the same bits)."""
    idx = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ m]
    return s[:, 0]


def _lane_sum(v):
    s = torch.zeros(v.shape[:2], dtype=torch.float32)
    for i in range(12):
        s = s + v[:, :, i]
    return s


FWD_DEFECTS = ("one-pass variance", "variance without the mean", "divisor 767", "eps dropped", "eps outside the root", "the other eps")
BWD_DEFECTS = ("no s1", "s2 off by 1e-3")
LOSS_DEFECTS = ("no abs in log1p(exp(-|z|))", "unmixed targets")
OLD_GATE_BLIND = ("one-pass variance", "eps dropped", "eps outside the root", "the other eps")


def restate_fwd(x, g, b, eps, defect=None):
    """ln_stats and the row kernels' output expression in fp32, in the kernel's order -> y, mean, rstd."""
    assert x.dtype == torch.float32 and (defect is None or defect in FWD_DEFECTS)
    if defect == "the other eps":
        eps = EPS[1] if eps == EPS[0] else EPS[0]
    if defect == "eps dropped":
        eps = 0.0
    v = _lanes(x)
    mu = _wave_sum(_lane_sum(v)) * INV_COLS
    d = v if defect == "variance without the mean" else v - mu[:, None, None]
    if defect == "one-pass variance":
        var = _wave_sum(_lane_sum(v * v)) * INV_COLS - mu * mu
    else:
        var = _wave_sum(_lane_sum(d * d)) * (float(np.float32(1.0) / np.float32(767.0)) if defect == "divisor 767" else INV_COLS)
    rs = 1.0 / (torch.sqrt(var) + eps) if defect == "eps outside the root" else 1.0 / torch.sqrt(var + eps)
    y = (x - mu[:, None]) * rs[:, None] * g + b
    return y, mu, rs


def restate_bwd(dy, x, g, mean, rstd, dres=None, defect=None):
    """layernorm_bwd_kernel's row math in fp32, in the kernel's order -> dx."""
    assert defect is None or defect in BWD_DEFECTS
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = dy * g
    s1 = _wave_sum(_lane_sum(_lanes(gg))) * INV_COLS
    s2 = _wave_sum(_lane_sum(_lanes(gg * xh))) * INV_COLS
    if defect == "no s1":
        s1 = torch.zeros_like(s1)
    if defect == "s2 off by 1e-3":
        s2 = s2 * 1.001
    dx = rstd[:, None] * (gg - s1[:, None] - xh * s2[:, None])
    return dx if dres is None else dx + dres


# ------------------------------------------------------------------------------------------------ LayerNorm cases
def case_layernorm_fwd(dev, dtype, per_family_rows):
    """maest_layernorm_fwd: y in `dtype` (and, fp32 in the bf16 build, MAEST_SPLIT3_A), mean, rstd; both eps."""
    x, fam, g, b = inputs(per_family_rows)
    worst = {}
    for eps in EPS:
        ref = fwd_ref(x, g, b, eps, fam)
        y, mean, rstd = ops.layernorm_fwd(x.to(dev), g.to(dev), b.to(dev), eps, dtype, save_stats=True)
        for k, r in check_fwd(y, mean, rstd, x, g, b, eps, fam, f"layernorm_fwd eps={eps}", ref).items():
            worst[k] = max(worst.get(k, 0.0), r)
        # all-zero rows pin the arithmetic exactly: mean = 0, rstd = fl(1 / fl(sqrt(fl(eps)))), y = beta (rounded once for a 16-bit y)
        zero = (x == 0).all(1)
        nz = int(zero.sum())
        assert nz > 0
        assert torch.equal(rstd.cpu()[zero], (1.0 / torch.sqrt(torch.zeros(1) + eps)).expand(nz)), f"eps={eps}: rstd of an all-zero row is not fl(1 / sqrt(eps))"
        assert not bool(mean.cpu()[zero].ne(0).any()), f"eps={eps}: mean of an all-zero row"
        if dtype == torch.bfloat16:
            _bits_equal(y.cpu()[zero], b.expand(nz, COLS).contiguous(), f"eps={eps}: y of an all-zero row is not beta")
        else:
            assert torch.equal(y.cpu()[zero], b.expand(nz, COLS)), f"eps={eps}: y of an all-zero row is not beta"
        if dtype == torch.float32:
            if not f16_build():
                s3 = ops.layernorm_fwd(x.to(dev), g.to(dev), b.to(dev), eps, ops.SPLIT3)
                for k, r in check_fwd(s3, None, None, x, g, b, eps, fam, f"layernorm_fwd eps={eps}", ref).items():
                    worst[k] = max(worst.get(k, 0.0), r)
    return show(f"layernorm_fwd {dtype}", worst)


def case_add_layernorm_fwd(dev, dtype, per_family_rows):
    """maest_add_layernorm_fwd: x_out bit-equal to the fp32 sum, the statistics and y gated on x_out; the delta turns plain rows into offset rows."""
    x, fam, g, b = inputs(per_family_rows)
    delta = offset_delta(x, fam, dtype)
    fam_out = fam.clone()
    fam_out[fam == 0] = FAMILIES.index("offset")
    want = f32(delta) + x
    worst = {}
    for eps in EPS:
        xn, y, mean, rstd = ops.add_layernorm_fwd(x.to(dev), delta.to(dev), g.to(dev), b.to(dev), eps, dtype, save_stats=True)
        assert torch.equal(xn.cpu().view(torch.int32), want.view(torch.int32)), "add_layernorm_fwd: x_out is not the fp32 sum"
        ref = fwd_ref(want, g, b, eps, fam_out)
        for k, r in check_fwd(y, mean, rstd, want, g, b, eps, fam_out, f"add_layernorm_fwd eps={eps}", ref).items():
            worst[k] = max(worst.get(k, 0.0), r)
        if dtype == torch.float32 and not f16_build():
            xn3, s3 = ops.add_layernorm_fwd(x.to(dev), delta.to(dev), g.to(dev), b.to(dev), eps, ops.SPLIT3)
            assert torch.equal(xn3, xn)
            for k, r in check_fwd(s3, None, None, want, g, b, eps, fam_out, f"add_layernorm_fwd eps={eps}", ref).items():
                worst[k] = max(worst.get(k, 0.0), r)
    return show(f"add_layernorm_fwd {dtype}", worst)


def _mixed_path_site(step, p, B, start):
    """The first drop-path site from `start` whose mask both keeps and drops a clip."""
    for site in range(start, start + 64):
        k = RC.path_keep(SEED, step, site, p, B)
        if k.any() and not k.all():
            return site
    raise AssertionError("no mixed drop-path mask")


def case_drop_add_layernorm_fwd(dev, dtype, per_family_rows, n_tok):
    """maest_drop_add_layernorm_fwd (regularise.hip:160-182 keeps its own copy of the statistics): nothing dropped -- the gates of
    add_layernorm_fwd, and whether it is bit-equal to it --; element keep 0.9 and path keep 0.8 with the masks of regulariser_cases, rows
    per clip n_tok and 2.  Dropping cases: delta = x / 4 in the operand type, so that x + delta * multiplier does not cancel and
    2 u |x_out| holds the two roundings of the multiplier and the add; y and the statistics are gated on the x_out the kernel wrote."""
    x, fam, g, b = inputs(per_family_rows)
    rows = x.shape[0]
    assert rows % n_tok == 0
    step, worst = 3, {}
    snap = ops.rng_state(SEED, dev, step=step)
    # nothing dropped
    delta = offset_delta(x, fam, dtype)
    fam_out = fam.clone()
    fam_out[fam == 0] = FAMILIES.index("offset")
    want = f32(delta) + x
    for eps in EPS:
        xn, y, mean, rstd = ops.drop_add_layernorm_fwd(x.to(dev), delta.to(dev), g.to(dev), b.to(dev), eps, dtype, rows // n_tok, n_tok, n_tok,
                                                       (16, 0.0), (17, 0.0), snap, save_stats=True)
        assert torch.equal(xn.cpu().view(torch.int32), want.view(torch.int32)), "drop_add_layernorm_fwd, nothing dropped: x_out is not the fp32 sum"
        for k, r in check_fwd(y, mean, rstd, want, g, b, eps, fam_out, f"drop_add_layernorm_fwd (nothing dropped) eps={eps}").items():
            worst[k] = max(worst.get(k, 0.0), r)
        _, y2, mean2, rstd2 = ops.add_layernorm_fwd(x.to(dev), delta.to(dev), g.to(dev), b.to(dev), eps, dtype, save_stats=True)
        same = torch.equal(y.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), y2.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)) \
            and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
        print(f"drop_add_layernorm_fwd {dtype} eps={eps}, nothing dropped: bit-equal to add_layernorm_fwd: {same}")
    # element keep 0.9, path keep 0.8
    pe, pp = 0.1, 0.2
    delta = lp(0.25 * x, dtype)
    for rpc in (n_tok, 2):
        B = rows // rpc
        n = B * rpc
        site_p = _mixed_path_site(step, pp, B, 17)
        me = torch.from_numpy(RC.elem_keep(SEED, step, 16, pe, B, n_tok, COLS, tokens=range(rpc)).astype(np.float64) * float(RC.scale(pe)))
        mp = torch.from_numpy(RC.path_keep(SEED, step, site_p, pp, B).astype(np.float64) * float(RC.scale(pp))).reshape(B, 1, 1)
        xo64 = (x[:n].double().reshape(B, rpc, COLS) + (f32(delta[:n]).double().reshape(B, rpc, COLS) * me) * mp).reshape(n, COLS)
        for eps in EPS:
            xn, y, mean, rstd = ops.drop_add_layernorm_fwd(x[:n].to(dev), delta[:n].to(dev), g.to(dev), b.to(dev), eps, dtype, B, n_tok, rpc,
                                                           (16, pe), (site_p, pp), snap, save_stats=True)
            what = f"drop_add_layernorm_fwd (keep 0.9 / 0.8, {rpc} rows per clip) eps={eps}"
            for k, r in per_family(close32, fam[:n], xn, xo64, U * xo64.abs(), f"{what}: x_out").items():      # (close32 adds the second u |x_out|)
                worst[("x_out", k)] = max(worst.get(("x_out", k), 0.0), r)
            dropped = (mp.reshape(B) == 0).repeat_interleave(rpc)
            assert torch.equal(xn.cpu()[dropped], x[:n][dropped]), f"{what}: a dropped clip's rows are not x"
            for k, r in check_fwd(y, mean, rstd, xn, g, b, eps, fam[:n], what).items():
                worst[k] = max(worst.get(k, 0.0), r)
    return show(f"drop_add_layernorm_fwd {dtype}", worst)


BWD_MODES = ("no dres", "dres", "compact dres")


def case_layernorm_bwd(dev, dtype, per_family_rows, blocks=(None, 2), deterministic=(0, 1), eps_values=EPS, modes=BWD_MODES):
    """maest_layernorm_bwd / _headres fed the statistics its own forward wrote: without dres, with a dense one, with the compact one of
    (n_tok, n_head) = (5, 2); ln_bwd_blocks at the default and at 2 (a workgroup walks several row groups); default and ordered sums.
    (The emulator tests split the product: an ordered launch costs them seconds whatever the row count.)"""
    x, fam, g, b = inputs(per_family_rows)
    rows = x.shape[0]
    dy = lp(rnd((rows, COLS), 730), dtype)
    dres = rnd((rows, COLS), 731)
    r5 = rows - rows % 5
    dres_c = rnd((r5 // 5 * 2, COLS), 732)
    dense = torch.zeros(r5 // 5, 5, COLS)
    dense[:, :2] = dres_c.reshape(r5 // 5, 2, COLS)
    dense = dense.reshape(r5, COLS)
    worst = {}
    xd, gd, dyd = x.to(dev), g.to(dev), dy.to(dev)
    for eps in eps_values:
        _, mean, rstd = ops.layernorm_fwd(xd, gd, b.to(dev), eps, dtype, save_stats=True)
        for nb in blocks:
            for det in deterministic:
                with ops.options(**({} if nb is None else {"ln_bwd_blocks": nb})), ops.thread_options(deterministic=det):
                    for name, n, dr, dr_ref, ht in (("no dres", rows, None, None, None), ("dres", rows, dres, dres, None),
                                                    ("compact dres", r5, dres_c, dense, (5, 2))):
                        if name not in modes:
                            continue
                        dg, db = torch.zeros(COLS, device=dev), torch.zeros(COLS, device=dev)
                        dx, dx_lp = ops.layernorm_bwd(dyd[:n], xd[:n], gd, mean[:n], rstd[:n], None if dr is None else dr.to(dev), dg, db,
                                                      lp_dtype=dtype, head_tokens=ht)
                        what = f"layernorm_bwd eps={eps} blocks={nb} deterministic={det} {name}"
                        for k, r in check_bwd(dx, dx_lp, dg, db, dy[:n], x[:n], g, mean[:n], rstd[:n], dr_ref, fam[:n], what).items():
                            worst[k] = max(worst.get(k, 0.0), r)
    return show(f"layernorm_bwd {dtype}", worst)


# ------------------------------------------------------------------------------------------------ head pooling
def head_inputs(N=5, seed=760):
    """x [B = families, N, 768]: the cls row of clip b from family b, its dist row from the next family; the patch rows plain."""
    B = len(FAMILIES)
    x = rnd((B, N, COLS), seed, 2.0) + 0.3
    fam_c = torch.arange(B)
    fam_d = (fam_c + 1) % B
    near = family_rows("near-constant", len(NEAR), seed + 1)
    for bi in range(B):
        for tok, f in ((0, int(fam_c[bi])), (1, int(fam_d[bi]))):
            x[bi, tok] = near[(3 * bi + tok) % len(NEAR)] if FAMILIES[f] == "near-constant" else family_rows(FAMILIES[f], 1, seed + 10 * bi + tok)[0]
    x[0, 1] = 0.0       # (an exactly constant row whichever near-constant row was drawn)
    fam_d[0] = FAMILIES.index("near-constant")
    return x, fam_c, fam_d, 1.0 + rnd((COLS,), seed + 90, 0.1), rnd((COLS,), seed + 91, 0.1)


def case_head_pool(dev, N=5):
    """maest_head_pool_fwd (cls, dist, feat, mean, rstd) and maest_head_pool_bwd on the families; both eps."""
    x, fam_c, fam_d, g, b = head_inputs(N)
    B = x.shape[0]
    dc, dd, df = rnd((B, COLS), 770), rnd((B, COLS), 771), rnd((B, COLS), 772)
    worst = {}
    for eps in EPS:
        cls, dist, feat, mean, rstd = ops.head_pool_fwd(x.to(dev), g.to(dev), b.to(dev), eps, save_stats=True)
        rc, rd = fwd_ref(x[:, 0], g, b, eps, fam_c), fwd_ref(x[:, 1], g, b, eps, fam_d)
        for k, r in check_fwd(cls, mean[:, 0], rstd[:, 0], x[:, 0], g, b, eps, fam_c, f"head_pool_fwd eps={eps}: cls", rc).items():
            worst[("cls " + k[0], k[1])] = max(worst.get(("cls " + k[0], k[1]), 0.0), r)
        for k, r in check_fwd(dist, mean[:, 1], rstd[:, 1], x[:, 1], g, b, eps, fam_d, f"head_pool_fwd eps={eps}: dist", rd).items():
            worst[("dist " + k[0], k[1])] = max(worst.get(("dist " + k[0], k[1]), 0.0), r)
        # feat = (cls + dist) / 2: the two errors halved, one add (close32 counts it), an exact halving
        merge(worst, per_family(close32, fam_c, feat, (rc["y"] + rd["y"]) / 2, (rc["d_y"] + rd["d_y"]) / 2 + U * (rc["y"].abs() + rd["y"].abs()) / 2,
                                f"head_pool_fwd eps={eps}: feat"), "feat")
        for d_feat in (df, None):
            dg, db = torch.zeros(COLS, device=dev), torch.zeros(COLS, device=dev)
            dx = ops.head_pool_bwd(dc.to(dev), dd.to(dev), None if d_feat is None else d_feat.to(dev), x.to(dev), g.to(dev), mean, rstd, dg, db)
            assert not bool(dx[:, 2:].cpu().ne(0).any()), "head_pool_bwd: a patch row's dx is not zero"
            x2 = x[:, :2].reshape(2 * B, COLS)
            dy2 = torch.stack([dc.double(), dd.double()], 1) + (0.0 if d_feat is None else 0.5 * d_feat.double()[:, None])
            fam2 = torch.stack([fam_c, fam_d], 1).reshape(2 * B)
            what = f"head_pool_bwd eps={eps} d_feat={d_feat is not None}"
            for k, r in check_bwd(dx[:, :2].reshape(2 * B, COLS), None, dg, db, dy2.reshape(2 * B, COLS), x2, g, mean.reshape(2 * B), rstd.reshape(2 * B),
                                  None, fam2, what, n=2 * B + 3, extra_dy_rounding=True).items():
                worst[k] = max(worst.get(k, 0.0), r)
    return show("head_pool", worst)


# ------------------------------------------------------------------------------------------------ loss
Z_VALUES = (0.0, 1e-8, -1e-8, 1.0, -1.0, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4)
LOSS_SHAPES = ((64, 400), (7, 519))


def loss_inputs(rows, cols, seed=780):
    """Logits tiled from Z_VALUES (every value meets both hard targets in every row), hard targets, a permutation and mixing weights."""
    idx = torch.arange(rows * cols).reshape(rows, cols)
    z = torch.tensor(Z_VALUES, dtype=torch.float32)[idx % len(Z_VALUES)]
    y = ((idx // len(Z_VALUES)) % 4 == 1).float()
    rng = np.random.Generator(np.random.PCG64(seed))
    perm = torch.from_numpy(rng.permutation(rows).astype(np.int32))
    lam = torch.from_numpy(rng.random(rows).astype(np.float32))
    return z, y, perm, lam


def loss_chain(rows, cols, training):
    """The length of the documented add chain (misc.hip:221-226) of the launch form."""
    total = rows * cols
    blocks, threads = (min(256, -(-total // 256)), 256) if training else (1, 1024)
    return -(-total // (blocks * threads)) + 6 + threads // 64 + -(-blocks // 64) + 6


def loss_ref(z, y, perm, lam, weight, training):
    """fp64 loss, dlogits, sigmoid and their bounds from the fp32 inputs."""
    rows, cols = z.shape
    total = rows * cols
    z64, t, tabs = z.double(), y.double(), None
    if perm is not None:
        l = lam.double()[:, None]
        yp = y.double()[perm.long()]
        t, tabs = t * l + yp * (1 - l), y.double().abs() * l + yp.abs() * (1 - l)
    soft = torch.log1p(torch.exp(-z64.abs()))
    term = z64.clamp_min(0) - z64 * t + soft
    n = loss_chain(rows, cols, training)
    loss = weight * term.sum() / total
    d_loss = weight / total * float((4 * U * (z64.clamp_min(0) + (z64 * t).abs() + soft)).sum() + 2 * n * U * term.abs().sum())
    sg = torch.sigmoid(z64)
    dz = (sg - t) * weight / total
    d_dz = (4 * U * sg + U * (sg - t).abs()) * weight / total
    d_dz = d_dz + 2.0 ** -126 * weight / total + 2.0 ** -149                      # misc.hip:284: the fp32 range; the subnormal grid
    if tabs is not None:          # a soft target: its own roundings (misc.hip:282), and s - t no longer 0 or +-1 in front of the scaling (misc.hip:276,285)
        d_dz = d_dz + (2 * U * tabs + 3 * U * (sg - t).abs()) * weight / total
    return dict(loss=loss, d_loss=d_loss, dz=dz, d_dz=d_dz, sg=sg, t=t, total=total)


def mixed32(y, perm, lam):
    """The fp32 target of misc.hip:230-234."""
    if perm is None:
        return y
    l = lam[:, None]
    return y * l + y[perm.long()] * (1.0 - l)


def saturated_dz(z, t32, weight, total):
    """-> (mask, the exact dlogits of misc.hip:284-285 where the fp32 sigmoid is exactly 0 or 1)."""
    sg = 1.0 / (1.0 + torch.exp(-z))
    mask = (z <= -89.0) | (z >= 20.0)
    assert bool(((sg == 0) | (sg == 1))[mask].all())
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(total), dtype=torch.float32)
    return mask, (torch.tensor(weight, dtype=torch.float32) * (sg - t32)) * inv


def check_loss(loss, dz, z, y, perm, lam, weight, what):
    """The gates of the module docstring on one maest_bce_logits call; dz None: the loss-only launch form.  -> {output: worst err / bound}"""
    r = loss_ref(z, y, perm, lam, weight, dz is not None)
    got = float(loss)
    assert math.isfinite(got), f"{what}: the loss is {got}"
    err = abs(got - float(r["loss"]))
    lim = r["d_loss"] + U * abs(float(r["loss"]))
    assert err <= lim, f"{what}: loss {got!r} against {float(r['loss'])!r}: error {err:.3e} outside {lim:.3e}"
    worst = {"loss": err / lim}
    if dz is not None:
        dz = dz.detach().cpu()
        e = (dz.double() - r["dz"]).abs()
        bad = ~(e <= r["d_dz"])
        ratio = torch.nan_to_num(e / r["d_dz"], nan=float("inf"))
        if bool(bad.any()):
            i = tuple(int(v) for v in np.unravel_index(int(torch.where(bad, ratio, -torch.ones_like(ratio)).argmax()), tuple(ratio.shape)))
            raise AssertionError(f"{what}: dlogits: {int(bad.sum())} elements outside the gate; worst err / bound {float(ratio[i]):.3f} at {i}: z = {float(z[i])!r}, "
                                 f"t = {float(r['t'][i])!r}, got {float(dz[i])!r}, reference {float(r['dz'][i])!r}")
        worst["dlogits"] = float(ratio.max())
        mask, want = saturated_dz(z, mixed32(y, perm, lam), weight, r["total"])
        assert torch.equal(dz[mask].view(torch.int32), want[mask].view(torch.int32)), \
            f"{what}: dlogits of a saturated logit is not (0 - t) or (1 - t) times weight / total bit for bit"
    return worst


def check_sigmoid_mean(act, z, what):
    ref = torch.sigmoid(z.double()).mean(0)
    err = (act.detach().cpu().double() - ref).abs()
    lim = (z.shape[0] + 4) * U
    assert bool((err <= lim).all()), f"{what}: sigmoid_mean off by {float(err.max()):.3e}, bound {lim:.3e}"
    return float(err.max()) / lim


def case_loss(dev, shapes=LOSS_SHAPES):
    """maest_bce_logits in both launch forms and maest_sigmoid_mean on the tiled logits, hard and mixup-softened targets, weights 1 and 0.5."""
    worst = {}
    for rows, cols in shapes:
        z, y, perm, lam = loss_inputs(rows, cols)
        for mix in (False, True):
            for weight in (1.0, 0.5):
                p, l = (perm, lam) if mix else (None, None)
                pd, ld = (perm.to(dev), lam.to(dev)) if mix else (None, None)
                what = f"bce_logits {rows} x {cols} mixed={mix} weight={weight}"
                loss, dz = ops.bce_logits(z.to(dev), y.to(dev), weight, pd, ld)
                for k, r in check_loss(loss, dz, z, y, p, l, weight, what + " (training form)").items():
                    worst[(k, "training")] = max(worst.get((k, "training"), 0.0), r)
                loss, none = ops.bce_logits(z.to(dev), y.to(dev), weight, pd, ld, want_grad=False)
                assert none is None
                for k, r in check_loss(loss, None, z, y, p, l, weight, what + " (loss-only form)").items():
                    worst[(k, "loss only")] = max(worst.get((k, "loss only"), 0.0), r)
        worst[("sigmoid_mean", f"{rows} x {cols}")] = check_sigmoid_mean(ops.sigmoid_mean(z.to(dev)), z, f"sigmoid_mean {rows} x {cols}")
    print("loss: " + ", ".join(f"{k[0]} ({k[1]}) {v:.3f}" for k, v in worst.items()))
    return worst


def restate_loss(z, y, perm, lam, weight, training, defect=None):
    """misc.hip:227-296 in fp32 in the documented order -> loss, dlogits (None for the loss-only form), sigmoid_mean."""
    assert defect is None or defect in LOSS_DEFECTS
    rows, cols = z.shape
    total = rows * cols
    t = y if defect == "unmixed targets" else mixed32(y, perm, lam)
    soft = torch.log(1.0 + torch.exp(-z)) if defect == "no abs in log1p(exp(-|z|))" else torch.log1p(torch.exp(-z.abs()))
    term = (z.clamp_min(0) - z * t + soft).reshape(-1)
    blocks, threads = (min(256, -(-total // 256)), 256) if training else (1, 1024)
    per = -(-total // (blocks * threads))
    pad = torch.zeros(per * blocks * threads, dtype=torch.float32)
    pad[:total] = term
    pad = pad.reshape(per, blocks, threads)
    acc = torch.zeros(blocks, threads)
    for k in range(per):
        acc = acc + pad[k]          # (a thread past the end adds nothing: + 0 is exact)
    waves = acc.reshape(blocks * threads // 64, 64)
    waves = _wave_sum(waves).reshape(blocks, threads // 64)
    part = torch.zeros(blocks)
    for w in range(threads // 64):
        part = part + waves[:, w]
    if not training:
        w32 = torch.tensor(weight, dtype=torch.float32)
        return w32 * part[0] / torch.tensor(float(total), dtype=torch.float32), None
    lane = torch.zeros(64)
    padded = torch.zeros(-(-blocks // 64) * 64)
    padded[:blocks] = part
    for k in range(padded.numel() // 64):
        lane = lane + padded[k * 64:(k + 1) * 64]
    scale = torch.tensor(weight, dtype=torch.float32) / torch.tensor(float(total), dtype=torch.float32)
    loss = scale * _wave_sum(lane[None])[0]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(total), dtype=torch.float32)
    dz = (torch.tensor(weight, dtype=torch.float32) * (1.0 / (1.0 + torch.exp(-z)) - t)) * inv
    return loss, dz
