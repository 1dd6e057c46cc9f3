"""Cases of the deterministic mode (include/maest_hip.h: MAEST_OPT_DETERMINISTIC) shared by the emulator tests (CPU, tiny shapes) and
the GPU tests.  Three kinds:

  * exact order: the TN GEMM on integer operands whose per-split partials are exact in fp32 and whose sum depends on the order they
    are added in -- 2^24, 1, 1, -2^24 over four forced splits, for C and for colsum.  The documented order (ascending splits from 0,
    the destination last) gives C0 + 0 exactly; adding the destination first, or the splits in any other order, gives C0 + 1 or
    C0 + 2.  Compared bit for bit with an fp32 loop in the documented order.
  * repeatable: every entry point with an ordered form, three times on cancellation-heavy inputs (magnitudes 2^-12 .. 2^12, random signs:
    a changed summation order changes bits); the three results must be bit-identical, and inside the standard bound of a recursive fp32
    sum against fp64,  |fl(sum) - sum| <= n u sum |terms|  with n the number of terms and u = 2^-24 (Higham, Accuracy and Stability of
    Numerical Algorithms, eq. 4.4) -- doubled for the rounding of the terms themselves; where a term is formed from a difference
    (LayerNorm's xhat = (x - mean) rstd) its magnitude is taken from the operands of the difference, (|x| + |mean|) rstd.
    token_assemble_bwd and colsum are also held bit for bit to an fp32 loop in their documented order.
  * still right: the existing cases of tests/kernel_cases.py, with their own gates, run under the option (the test files do that).
"""
import numpy as np
import torch

from maest_amd import ops
from tests import kernel_cases as KC

U32 = 2.0 ** -24


def heavy(shape, seed, dev="cpu"):
    """sign * 2^u, u uniform over [-12, 12]: sums of these cancel heavily, so their fp32 value depends on the order of the adds.
    On a GPU the large operands are drawn there (torch's generator: the same values for the same seed and device type)."""
    if torch.device(dev).type == "cuda":
        g = torch.Generator(device=dev).manual_seed(seed)
        mag = torch.exp2(torch.rand(shape, generator=g, device=dev) * 24.0 - 12.0)
        return mag * (torch.randint(0, 2, shape, generator=g, device=dev).float() * 2.0 - 1.0)
    rng = np.random.Generator(np.random.PCG64(seed))
    mag = np.exp2(rng.uniform(-12.0, 12.0, shape))
    return torch.from_numpy((mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32))


def same_bits(runs, what):
    for i, r in enumerate(runs[1:], 1):
        for k, (a, b) in enumerate(zip(runs[0], r)):
            if a is None and b is None:
                continue
            assert torch.equal(a.contiguous().view(torch.uint8) if a.dtype != torch.float32 else a.view(torch.int32),
                               b.contiguous().view(torch.uint8) if b.dtype != torch.float32 else b.view(torch.int32)), \
                f"{what}: run {i} differs from run 0 in result {k}"


def sum_bound(got, ref64, abs_sum64, n, what):
    """|got - ref| <= 2 n u sum |terms| (module docstring), elementwise."""
    err = (got.detach().to(ref64.device).double() - ref64).abs()
    lim = 2.0 * n * U32 * abs_sum64 + 1e-30
    worst = float((err / lim).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: error {float(err.max()):.3e} outside the summation bound (ratio {worst:.2f})"


# ------------------------------------------------------------------------------------------------ exact order
def exact_order_operands(K, M, N, what, f16):
    """A [K, M], B [K, N] with one non-zero token row per quarter of K (= per split of four) such that the split partials are
    2^24, 1, 1, -2^24: for C (`what` = "c"; half build: 2^12 * 2^12 products) or for colsum ("colsum": 2^24 directly in bf16 and fp32,
    2^12 rows of 2^12 in the half build)."""
    a, b = torch.zeros(K, M), torch.zeros(K, N)
    q = K // 4
    rows = [s * q + (5 + 37 * s) % q for s in range(4)]        # somewhere inside each split's range, a different slice each
    if what == "c":
        big = 2.0 ** 12 if f16 else 2.0 ** 24
        for s, (va, vb) in enumerate([(big, 2.0 ** 24 / big), (1.0, 1.0), (1.0, 1.0), (-big, 2.0 ** 24 / big)]):
            a[rows[s]], b[rows[s]] = va, vb
    elif not f16:
        for s, va in enumerate([2.0 ** 24, 1.0, 1.0, -2.0 ** 24]):
            a[rows[s]] = va
    else:
        assert q >= 4096, "half build: a split needs 2^12 rows of 2^12 for a column-sum partial of 2^24"
        a[0:4096], a[rows[1]], a[rows[2]], a[3 * q:3 * q + 4096] = 2.0 ** 12, 1.0, 1.0, -(2.0 ** 12)
    return a, b, q


def documented_order(c0, partials):
    """dest = dest + (((0 + p[0]) + p[1]) + ...), every operation rounded to fp32."""
    s = np.zeros_like(c0, dtype=np.float32)
    for p in partials:
        s = (s + p.astype(np.float32)).astype(np.float32)
    return (c0.astype(np.float32) + s).astype(np.float32)


def case_exact_order(dev, dtype, K, M, N, expect_bytes=None, colsum=True):
    """Four forced splits under the option; C and colsum start from small non-zero integers.  expect_bytes(splits) -> the workspace
    size of the kernel form the caller's options select: asserted, so that the case knows which form it ran."""
    f16 = KC.f16_build() and dtype == torch.bfloat16
    rng = np.random.Generator(np.random.PCG64(M * 7 + N))
    with ops.thread_options(deterministic=1):
        nbytes = ops.gemm_tn_workspace_bytes(dtype, M, N, K, 4)
        assert nbytes > 0, "no workspace form for this shape under the option"
        if expect_bytes is not None:
            assert nbytes == expect_bytes(4), (nbytes, expect_bytes(4))
        for what in ("c", "colsum") if colsum else ("c",):
            if what == "colsum" and f16 and K < 4 * 4096:
                continue                                            # (the half build's column-sum case needs K >= 2^14: GPU only)
            a, b, q = exact_order_operands(K, M, N, what, f16)
            c0 = rng.integers(-8, 9, (M, N)).astype(np.float32)
            cs0 = rng.integers(-8, 9, (M,)).astype(np.float32)
            out, cs = torch.from_numpy(c0.copy()).to(dev), torch.from_numpy(cs0.copy()).to(dev)
            ops.gemm_tn(KC.lp(a, dtype).to(dev), KC.lp(b, dtype).to(dev), out, colsum=cs, split_k=4, M=M, N=N)
            a64, b64 = a.double().numpy(), b.double().numpy()
            pc = [a64[s * q:(s + 1) * q].T @ b64[s * q:(s + 1) * q] for s in range(4)]       # exact: integers below 2^25
            pcs = [a64[s * q:(s + 1) * q].sum(0) for s in range(4)]
            want_c, want_cs = documented_order(c0, pc), documented_order(cs0, pcs)
            if what == "c":
                assert np.array_equal(want_c, c0), "the documented order gives C0 + 0"
                d = out.cpu().numpy() - want_c
                assert np.array_equal(out.cpu().numpy(), want_c), \
                    f"C is not the documented-order sum: C - C0 in [{d.min()}, {d.max()}] (another order gives +1 / +2)"
                if f16:
                    continue                                        # (the half build's colsum partials are not the C case's)
            d = cs.cpu().numpy() - want_cs
            assert np.array_equal(cs.cpu().numpy(), want_cs), \
                f"colsum ({what} operands) is not the documented-order sum: off by [{d.min()}, {d.max()}]"


def ws_bytes_256(M, N):
    return lambda splits: splits * (M // 256) * (N // 256) * 65536 * 4 + splits * (N // 256) * M * 4


def ws_bytes_small(M, N):
    mp, npad = -(-M // 128) * 128, -(-N // 128) * 128
    return lambda splits: splits * (mp * npad + mp) * 4


# ------------------------------------------------------------------------------------------------ repeatable
def case_repeat_gemm_tn(dev, dtype, K, M, N, split_k=0, lda_pad=0, runs=3):
    a_full = KC.lp(heavy((K, M + lda_pad), 300 + K, dev), dtype)       # (operands and the fp64 reference stay on `dev`)
    b = KC.lp(heavy((K, N), 301 + K, dev), dtype)
    a_dev, b_dev = a_full[:, :M], b
    res = []
    with ops.thread_options(deterministic=1):
        for _ in range(runs):
            out = torch.zeros((M, N), dtype=torch.float32, device=dev)
            cs = torch.zeros(M, dtype=torch.float32, device=dev)
            ops.gemm_tn(a_dev, b_dev, out, colsum=cs, split_k=split_k, M=M, N=N)
            res.append((out, cs))
    same_bits(res, f"gemm_tn K={K} M={M} N={N} split_k={split_k}")
    a64, b64 = KC.f32(a_full[:, :M]).double(), KC.f32(b).double()
    sum_bound(res[0][0], a64.t() @ b64, a64.abs().t() @ b64.abs(), K, "gemm_tn C")
    sum_bound(res[0][1], a64.sum(0), a64.abs().sum(0), K, "gemm_tn colsum")


def case_repeat_layernorm_bwd(dev, dtype, rows, head_tokens=None, runs=3):
    """dgamma / dbeta three times under the option; dx and dx_lp bit for bit those of the default form (the row math is the same,
    the parked rows included)."""
    x = KC.rnd((rows, 768), 310, 2.0) + 0.3
    g = 1.0 + KC.rnd((768,), 311, 0.1)
    dy = KC.lp(heavy((rows, 768), 312 + rows), dtype)
    mean, var = x.mean(1), x.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    if head_tokens is None:
        dres = KC.rnd((rows, 768), 313)
    else:
        n_tok, n_head = head_tokens
        dres = KC.rnd((rows // n_tok * n_head, 768), 313)
    args = (dy.to(dev), x.to(dev), g.to(dev), mean.to(dev), rstd.to(dev), dres.to(dev))

    def run():
        dg, db = torch.zeros(768, device=dev), torch.zeros(768, device=dev)
        dx, dx_lp = ops.layernorm_bwd(*args, dg, db, lp_dtype=dtype, head_tokens=head_tokens)
        return dg, db, dx, dx_lp
    base = run()
    with ops.thread_options(deterministic=1):
        res = [run() for _ in range(runs)]
    same_bits(res, f"layernorm_bwd rows={rows} head_tokens={head_tokens}")
    same_bits([base[2:], res[0][2:]], "layernorm_bwd dx / dx_lp against the default form")
    xh = ((x.double() - mean.double()[:, None]) * rstd.double()[:, None])
    xmag = (x.double().abs() + mean.double().abs()[:, None]) * rstd.double()[:, None]
    d64 = KC.f32(dy).double()
    sum_bound(res[0][0], (d64 * xh).sum(0), (d64.abs() * xmag).sum(0), rows + 8, "layernorm dgamma")
    sum_bound(res[0][1], d64.sum(0), d64.abs().sum(0), rows + 8, "layernorm dbeta")


def case_repeat_head_pool_bwd(dev, B, N=5, runs=3):
    x = KC.rnd((B, N, 768), 320, 1.5)
    g = 1.0 + KC.rnd((768,), 321, 0.1)
    b = KC.rnd((768,), 322, 0.1)
    dc, dd = heavy((B, 768), 323), heavy((B, 768), 324)
    _, _, _, mean, rstd = ops.head_pool_fwd(x.to(dev), g.to(dev), b.to(dev), 1e-6, save_stats=True)
    res = []
    with ops.thread_options(deterministic=1):
        for _ in range(runs):
            dg, db = torch.zeros(768, device=dev), torch.zeros(768, device=dev)
            dx = ops.head_pool_bwd(dc.to(dev), dd.to(dev), None, x.to(dev), g.to(dev), mean, rstd, dg, db)
            res.append((dg, db, dx))
    same_bits(res, f"head_pool_bwd B={B}")
    x2 = x[:, :2].double()
    rs = 1.0 / torch.sqrt(x2.var(2, unbiased=False, keepdim=True) + 1e-6)
    xh = (x2 - x2.mean(2, keepdim=True)) * rs
    xmag = (x2.abs() + x2.mean(2, keepdim=True).abs()) * rs
    d = torch.stack([dc, dd], 1).double()
    sum_bound(res[0][0], (d * xh).sum((0, 1)), (d.abs() * xmag).sum((0, 1)), 2 * B + 8, "head dgamma")
    sum_bound(res[0][1], d.sum((0, 1)), d.abs().sum((0, 1)), 2 * B + 8, "head dbeta")


def case_repeat_token_assemble_bwd(dev, dtype, B, runs=3):
    """A 3 x 3 token grid left by patchout (time columns 0, 2, 3 of 5): three kept tokens share every frequency row and every time
    column.  The tables against an fp32 loop in the documented order: tokens ascending, clips ascending inside a token."""
    Fg, Tt, toff = 3, 6, 1
    tok = torch.tensor([[f, t] for f in range(Fg) for t in (0, 2, 3)], dtype=torch.int32)
    P = tok.shape[0]
    dx0 = heavy((B, 2 + P, 768), 330 + B)
    res = []
    with ops.thread_options(deterministic=1):
        for _ in range(runs):
            z = lambda *s: torch.full(s, 0.25, device=dev)              # (accumulated: a non-zero start)
            outs = [z(768), z(768), z(2, 768), z(768, Fg), z(768, Tt)]
            dp = ops.token_assemble_bwd(dx0.to(dev), B, Fg, Tt, toff, tok.to(dev), dtype, *outs)
            res.append((dp, *outs))
    same_bits(res, f"token_assemble_bwd B={B}")
    d = dx0.numpy()

    def walk(tokens):
        s = np.zeros(768, dtype=np.float32)
        for n in tokens:
            for b in range(B):
                s = (s + d[b, n]).astype(np.float32)
        return (np.float32(0.25) + s).astype(np.float32)
    dp, d_cls, d_dist, d_np, d_fp, d_tp = (t.cpu() for t in res[0])
    assert torch.equal(KC.f32(dp), KC.f32(KC.lp(dx0[:, 2:].reshape(B * P, 768), dtype))), "dpatches"
    assert np.array_equal(d_cls.numpy(), walk([0])) and np.array_equal(d_np[0].numpy(), walk([0])), "d_cls / d_new_pos[0]"
    assert np.array_equal(d_dist.numpy(), walk([1])) and np.array_equal(d_np[1].numpy(), walk([1])), "d_dist / d_new_pos[1]"
    for f in range(Fg):
        assert np.array_equal(d_fp[:, f].numpy(), walk([2 + j for j in range(P) if int(tok[j, 0]) == f])), f"d_freq_pos[:, {f}]"
    for t in range(Tt):
        assert np.array_equal(d_tp[:, t].numpy(), walk([2 + j for j in range(P) if toff + int(tok[j, 1]) == t])), f"d_time_pos[:, {t}]"


def case_repeat_colsum(dev, dtype, rows, cols, runs=3):
    """maest_colsum: chunks of 512 rows summed from 0 in ascending row order, the chunk sums in ascending order, the destination last."""
    src = KC.lp(heavy((rows, cols), 340 + rows), dtype)
    res = []
    with ops.thread_options(deterministic=1):
        for _ in range(runs):
            out = torch.full((cols,), 0.25, device=dev)
            ops.colsum(src.to(dev), out)
            res.append((out,))
    same_bits(res, f"colsum rows={rows}")
    s = KC.f32(src).numpy()
    tot = np.zeros(cols, dtype=np.float32)
    for r0 in range(0, rows, 512):
        part = np.zeros(cols, dtype=np.float32)
        for r in range(r0, min(r0 + 512, rows)):
            part = (part + s[r]).astype(np.float32)
        tot = (tot + part).astype(np.float32)
    assert np.array_equal(res[0][0].cpu().numpy(), (np.float32(0.25) + tot).astype(np.float32)), "colsum: not the documented order"
