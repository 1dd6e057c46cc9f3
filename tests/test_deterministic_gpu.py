"""GPU (`-m gpu`): the deterministic mode (MAEST_OPT_DETERMINISTIC, MAEST(deterministic=True)).

  * kernel level, the cases of tests/deterministic_cases.py at the device's shapes: the documented order of the TN GEMM's split-K
    combine bit for bit in every kernel form (small, eight-wave, one-wave-per-SIMD) and both 16-bit flavours; every ordered form three
    times on cancellation-heavy inputs, bit-identical and inside the summation bound; the existing gates of tests/kernel_cases.py under
    the option; all of it once more between NaN bands (tests/guard.py);
  * model level: two fresh models from one seed through three training steps + AdamW are bit-identical in loss and every parameter
    (bf16, fp16 under GradScaler, fp32; depth 2 and 12; autograd path and gradient sink); deterministic=True against False from the same
    state inside the gates of the oracle comparisons; off means off."""
import numpy as np
import pytest
import torch

from maest_amd import _lib, ops
from maest_amd.maest import MAEST
from maest_amd.module import Module
from tests import deterministic_cases as DC
from tests import guard
from tests import kernel_cases as KC
from tests import norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _flavour(name):
    import contextlib
    return _lib.flavour("f16") if name == "f16" else contextlib.nullcontext()


# ------------------------------------------------------------------------------------------------ documented order, exact
@pytest.mark.parametrize("flavour", ["bf16", "f16"])
@pytest.mark.parametrize("form", ["small", "eight-wave", "one-wave-per-simd"])
def test_exact_order(form, flavour, gemm_options):
    """768 x 768 over 1024 tokens in four forced splits (the small kernel: the ragged head shape 400 x 768); the half build's column
    sums over 2^14 tokens (2^12 rows of 2^12 per split)."""
    if form == "eight-wave":
        gemm_options(gemm_variant=3)
    elif form == "one-wave-per-simd":
        assert _lib.kernel_forms() & _lib.FORM_GEMM_TN_OW, "the one-wave-per-SIMD wgrad kernel is not in this build"
    M, N = (400, 768) if form == "small" else (768, 768)
    want = DC.ws_bytes_small(M, N) if form == "small" else DC.ws_bytes_256(M, N)
    with _flavour(flavour):
        DC.case_exact_order(DEV, BF, 1024, M, N, expect_bytes=want)
        if flavour == "f16":
            DC.case_exact_order(DEV, BF, 16384, M, N, expect_bytes=want)


@pytest.mark.parametrize("shape", [(400, 768), (768, 768)])
def test_exact_order_fp32_operands(shape):
    M, N = shape
    DC.case_exact_order(DEV, torch.float32, 1024, M, N, expect_bytes=DC.ws_bytes_small(M, N) if M == 400 else DC.ws_bytes_256(M, N))


# ------------------------------------------------------------------------------------------------ repeatable, and still right
@pytest.mark.parametrize("K,M,N,split_k", [(74240, 2304, 768, 0), (74240, 768, 768, 0), (74240, 3072, 768, 0), (74240, 768, 3072, 3),
                                           (74240, 768, 768, 14), (74240, 768, 256, 0), (64, 400, 768, 0), (1121, 400, 768, 0),
                                           (2300, 2304, 768, 5)])
def test_repeat_gemm_tn(K, M, N, split_k):
    """the production wgrad shapes at 74240 tokens (automatic splits and the side stream's 3 / 14), the patch-embedding wgrad and the
    ragged head, which the 256-tile kernels refuse, a ragged K"""
    DC.case_repeat_gemm_tn(DEV, BF, K, M, N, split_k=split_k)


@pytest.mark.parametrize("flavour", ["bf16", "f16"])
def test_repeat_gemm_tn_ragged_m_and_both_flavours(flavour, gemm_options):
    with _flavour(flavour):
        DC.case_repeat_gemm_tn(DEV, BF, 7, 519, 768, lda_pad=57)
        DC.case_repeat_gemm_tn(DEV, BF, 9280, 768, 768)
        DC.case_repeat_gemm_tn(DEV, torch.float32, 2300, 768, 768)
        gemm_options(gemm_variant=3)
        DC.case_repeat_gemm_tn(DEV, BF, 9280, 768, 768)


def test_gemm_tn_cases_under_the_option(gemm_options):
    with ops.thread_options(deterministic=1):
        KC.case_gemm_tn(DEV, BF, 74240, 768, 768, splits=(0, 5))
        KC.case_gemm_tn(DEV, BF, 1121, 768, 3072)
        KC.case_gemm_tn(DEV, torch.float32, 1121, 768, 3072)
        KC.case_gemm_tn(DEV, BF, 64, 400, 768)
        KC.case_gemm_tn(DEV, BF, 7, 519, 768, lda_pad=57)
        gemm_options(gemm_variant=3)
        KC.case_gemm_tn(DEV, BF, 2300, 2304, 768, splits=(0,))


def test_gemm_tn_without_a_workspace_has_one_writer():
    """maest_gemm_tn / a workspace one byte short: one split, one writer per element -- three runs bit-identical"""
    a, b = KC.lp(DC.heavy((2300, 768), 1, DEV)), KC.lp(DC.heavy((2300, 768), 2, DEV))
    s = ops._s(a)
    with ops.thread_options(deterministic=1):
        need = ops.gemm_tn_workspace_bytes(BF, 768, 768, 2300)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        outs = []
        for short in (None, None, None, 1, 1):
            out, cs = torch.zeros(768, 768, device=DEV), torch.zeros(768, device=DEV)
            _lib.call("maest_gemm_tn_ws", ops._p(a), 768, ops._p(b), 768, _lib.BF16, ops._p(out), 768, 768, 768, 2300, ops._p(cs), 0,
                      None if short is None else ops._p(ws), 0 if short is None else need - short, s)
            outs.append((out, cs))
    DC.same_bits(outs, "gemm_tn without a (sufficient) workspace")
    a64, b64 = KC.f32(a).double(), KC.f32(b).double()
    DC.sum_bound(outs[0][0], a64.t() @ b64, a64.abs().t() @ b64.abs(), 2300, "gemm_tn C, one split")


@pytest.mark.parametrize("blocks,rows", [(2, 1), (2, 5), (2, 33), (2, 11), (1024, 33), (1024, 4099), (1024, 20483)])
def test_repeat_layernorm_bwd(blocks, rows, gemm_options):
    gemm_options(ln_bwd_blocks=blocks)
    DC.case_repeat_layernorm_bwd(DEV, BF, rows)


@pytest.mark.parametrize("flavour", ["bf16", "f16"])
def test_repeat_layernorm_bwd_head_rows_and_fp32(flavour, gemm_options):
    with _flavour(flavour):
        DC.case_repeat_layernorm_bwd(DEV, BF, 3 * 5, head_tokens=(5, 2))
        DC.case_repeat_layernorm_bwd(DEV, BF, 256 * 5, head_tokens=(5, 2))
        DC.case_repeat_layernorm_bwd(DEV, torch.float32, 4099)


def test_layernorm_head_and_embedding_cases_under_the_option(gemm_options):
    with ops.thread_options(deterministic=1):
        KC.case_layernorm(DEV, BF, 1123)
        KC.case_layernorm(DEV, torch.float32, 33)
        KC.case_head(DEV, 70, 5)
        KC.case_patch_embed(DEV, BF, 5, 626, patchout=30, mix=True)
        gemm_options(ln_bwd_blocks=2)
        KC.case_layernorm(DEV, BF, 11)


@pytest.mark.parametrize("flavour,dtype", [("bf16", torch.float32), ("bf16", BF), ("f16", BF)])
def test_layernorm_bwd_on_hard_rows_under_the_option(flavour, dtype):
    """tests/norm_cases.py: the parked form (ln_bwd_blocks default: 97 workgroups; 2: a workgroup walks 49 row groups)
    and head_pool_bwd's single workgroup inside the bounds the counted roundings allow"""
    with _flavour(flavour):
        NC.case_layernorm_bwd(DEV, dtype, 64, deterministic=(1,))
        if dtype == torch.float32:
            with ops.thread_options(deterministic=1):
                NC.case_head_pool(DEV)


@pytest.mark.parametrize("B", [1, 3, 256])
def test_repeat_head_pool_bwd(B):
    DC.case_repeat_head_pool_bwd(DEV, B)


@pytest.mark.parametrize("B", [1, 5])
def test_token_tables_in_the_documented_order(B):
    DC.case_repeat_token_assemble_bwd(DEV, BF, B)
    DC.case_repeat_token_assemble_bwd(DEV, torch.float32, B)


def test_colsum_in_the_documented_order():
    DC.case_repeat_colsum(DEV, BF, 1100, 400)
    DC.case_repeat_colsum(DEV, torch.float32, 7, 519)


# ------------------------------------------------------------------------------------------------ under the guard
def test_guard_ordered_forms(gemm_options):
    """Every ordered form between NaN bands: the workspace at exactly the reported size (ops.gemm_tn allocates that), the parked rows
    inside dx_out, dgamma / dbeta and the tables' bands intact, const arguments unchanged."""
    import faulthandler
    faulthandler.dump_traceback_later(240, exit=True)
    try:
        with guard.guarded() as g:
            DC.case_repeat_gemm_tn(DEV, BF, 9280, 768, 768, runs=1)                 # one-wave-per-SIMD kernel
            DC.case_repeat_gemm_tn(DEV, torch.float32, 2300, 768, 768, runs=1)      # eight-wave kernel
            DC.case_repeat_gemm_tn(DEV, BF, 1121, 400, 768, runs=1)                 # small kernel, ragged
            DC.case_repeat_gemm_tn(DEV, BF, 7, 519, 768, lda_pad=57, runs=1)
            DC.case_repeat_layernorm_bwd(DEV, BF, 4099, runs=1)
            DC.case_repeat_layernorm_bwd(DEV, BF, 15, head_tokens=(5, 2), runs=1)
            DC.case_repeat_head_pool_bwd(DEV, 70, runs=1)
            DC.case_repeat_token_assemble_bwd(DEV, BF, 5, runs=1)
            DC.case_repeat_colsum(DEV, BF, 1100, 400, runs=1)
            gemm_options(gemm_variant=3)
            DC.case_repeat_gemm_tn(DEV, BF, 9280, 768, 768, runs=1)                 # eight-wave kernel, 16-bit operands
    finally:
        faulthandler.cancel_dump_traceback_later()
    for name in ("maest_gemm_tn_ws", "maest_layernorm_bwd_headres", "maest_head_pool_bwd", "maest_token_assemble_bwd", "maest_colsum"):
        assert g.calls[name], name


# ------------------------------------------------------------------------------------------------ model level
# B = 3 clips of 96 x 100 mel: 9 x 9 patches, 7 of the 9 time columns kept (several kept tokens per frequency row and time column)
KEEP = [0, 1, 3, 4, 6, 7, 8]
# the gates of the oracle comparisons of tests/test_model_gpu.py (fp32: test_odd_size_training_step_matches_the_oracle; bf16 / fp16:
# test_g5_training_step_loss_and_gradients / test_g5_training_step_in_fp16_with_a_scaled_loss): max |a - b| <= tol * max |b| per gradient
GATE = {"fp32": 1e-3, "bf16": 1e-2, "fp16": 1e-3}


def _batch(seed=400):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = torch.from_numpy(rng.standard_normal((3, 1, 96, 100), dtype=np.float32))
    y = torch.from_numpy((rng.random((3, 400)) < 0.05).astype(np.float32))
    perm = torch.from_numpy(rng.permutation(3))
    lam = torch.from_numpy(rng.uniform(0.5, 1, 3).astype(np.float32))
    return x.to(DEV), y.to(DEV), (perm, lam), (2, torch.tensor(KEEP))


def _model(depth, precision, deterministic, seed=77):
    torch.manual_seed(seed)
    net = MAEST(depth=depth, precision=precision, drop_rate=0.1, drop_path_rate=0.2, deterministic=deterministic)
    net.set_regulariser_seed(5)
    return net.to(DEV).train()


def _three_steps(depth, precision, sink):
    from maest_amd.dist import GradReducer
    net = _model(depth, precision, True)
    mod = Module(net=net, mixup_alpha=0.3, lr=1e-3)
    opt = mod.get_optimizer(net.parameters())
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 14) if precision == "fp16" else None
    red = None
    if sink:
        red = GradReducer(net.named_parameters(), bucket_mb=8, skip=("head_dist.weight", "head_dist.bias"))
        net._grad_sink = red
    x, y, mix, po = _batch()
    losses = []
    for it in range(3):
        if red is not None:
            red.reset()
        loss = mod.training_step((x, None, y), it, _mixup=mix, _patchout=po)
        (scaler.scale(loss) if scaler else loss).backward()
        if red is not None:
            red.finish()
        if scaler:
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()
        if red is None:
            opt.zero_grad(set_to_none=True)
        losses.append(loss.detach().clone())
    net._grad_sink = None
    torch.cuda.synchronize()
    if scaler:
        assert scaler.get_scale() == 2.0 ** 14, "a step was skipped: non-finite gradients"
    return losses, {n: p.detach().clone() for n, p in net.named_parameters()}


@pytest.mark.parametrize("depth,precision,sink", [(2, "bf16", False), (2, "fp16", False), (2, "fp32", False), (2, "bf16", True),
                                                  (2, "fp16", True), (2, "fp32", True), (12, "bf16", False), (12, "fp16", False),
                                                  (12, "fp32", False), (12, "bf16", True)])
def test_two_runs_from_one_seed_are_bit_identical(depth, precision, sink):
    la, pa = _three_steps(depth, precision, sink)
    lb, pb = _three_steps(depth, precision, sink)
    for i, (a, b) in enumerate(zip(la, lb)):
        assert torch.equal(a, b), f"loss of step {i}: {a.item()!r} vs {b.item()!r}"
    moved = 0
    for n in pa:
        assert torch.equal(pa[n], pb[n]), f"{n}: max difference {(pa[n] - pb[n]).abs().max().item():.3e} after three steps"
        moved += int(bool((pa[n] != 0).any()))
    assert moved > 10


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_deterministic_gradients_are_the_same_sums_in_another_order(precision):
    """deterministic=True against False from the same state (same masks: the generator is re-seeded), every gradient inside the gate the
    oracle comparison of that mode uses; and twice True: bit-identical"""
    net = _model(12, precision, False)
    mod = Module(net=net, mixup_alpha=0.3)
    x, y, mix, po = _batch()
    S = 2.0 ** 14 if precision == "fp16" else 1.0
    grads = []
    for det in (False, True, True):
        net.deterministic = det
        net.set_regulariser_seed(5)
        net.zero_grad(set_to_none=True)
        (mod.training_step((x, None, y), 0, _mixup=mix, _patchout=po) * S).backward()
        grads.append({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    assert len(grads[0]) > 150 and list(grads[0]) == list(grads[1])
    worst = 0.0
    for n, ref in grads[0].items():
        assert torch.equal(grads[1][n], grads[2][n]), n
        e = ((grads[1][n] - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
        worst = max(worst, e)
        assert e < GATE[precision], f"{n}: {e:.3e}"
    print(f"{precision}: worst relative difference of a gradient, ordered against atomic sums: {worst:.2e}")


def test_off_means_off():
    """deterministic=False (and the default None with nothing set) launches the same entry points, name by name, as a model that never
    heard of the switch, and its forward is bit-identical; True launches the same ENTRY POINTS too (the ordered forms live inside them)"""
    import torch.nn.functional as F
    x, y, mix, po = _batch()

    def run(net):
        net.set_regulariser_seed(5)
        with ops.KernelTimer(kinds=None) as t:
            logits, feats = net(x, _patchout=po)
            F.binary_cross_entropy_with_logits(logits.float(), y).backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), [r[0] for r in t.records]
    plain, off, on = _model(2, "bf16", None), _model(2, "bf16", False), _model(2, "bf16", True)
    assert ops.get_option("deterministic") == 0
    zp, names_p = run(plain)
    zo, names_o = run(off)
    zt, names_t = run(on)
    assert names_o == names_p == names_t and len(names_p) > 40
    assert torch.equal(zo, zp) and torch.equal(zt, zp)
    assert ops.get_option("deterministic") == 0, "a pass left its override behind"
