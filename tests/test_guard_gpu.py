"""GPU (`-m gpu`): the cases of the kernel tests once more on a real MI355X inside tests/guard.py's guarded(), at the shapes that have
tails: every tensor argument in an arena with NaN-pattern bands, every buffer ops allocates pre-filled with the pattern.  The hand-scheduled
kernels (gemm_nt_ow, gemm_tn_ow, attn_fwd_pw) run their real address arithmetic only here; a stray load reads a NaN of the band (and
shows in the result), a stray store changes a band (and is reported with entry point, argument and byte offset).  The cases keep
their assertions and tolerances.  Every test is an ordinary assertion: nothing here provokes a fault, the bands are memory the test
owns.  (The mutation tests that make a kernel touch a band on purpose are tests/test_emu_guard.py's, on the emulator only.)"""
import pytest
import torch

from maest_amd import _lib, ops
from tests import guard
from tests import kernel_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
COVERED = set()          # entry points the tests below require a guarded call of (tests/test_guard_cpu.py walks _lib.SIGNATURES against it)
LIMIT = 600              # seconds, per test (tests.guard.covering)
covers = lambda *entries: guard.covering(COVERED, *entries, limit=LIMIT)


# ------------------------------------------------------------------------------------------------ GEMM NT
@pytest.mark.parametrize("opts", [{}, {"gemm_variant": 3}, {"gemm_tail": 2}, {"gemm_wgs": 8}], ids=["default", "variant3", "tail2", "wgs8"])
@covers("maest_gemm_nt")
def test_guard_gemm_nt_ragged_rows_big_tiles(opts, gemm_options):
    """2637 = 10 x 256 + 77 rows through the one-wave-per-SIMD kernel, the eight-wave kernel, 128-row tiles and 8 persistent workgroups."""
    gemm_options(gemm_min_m=512, **opts)
    KC.case_gemm(DEV, BF, 2637, 768, 768, identity=False)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@covers("maest_gemm_nt")
def test_guard_gemm_nt_ragged_n(dtype, gemm_options):
    gemm_options(gemm_min_m=512)
    KC.case_gemm(DEV, dtype, 300, 519, 768)


@covers("maest_gemm_nt")
def test_guard_gemm_nt_offset_pointer_tail_launch(gemm_options):
    """66000 rows: 65536 in 256-row tiles, the last 464 (3.6 tiles of 128) in a second launch through offset pointers -- whose last
    tile ends the operands and the outputs."""
    KC.case_gemm(DEV, BF, 66000, 768, 768, identity=False)


@covers("maest_gemm_nt_rowdot")
def test_guard_gemm_rowdot(gemm_options):
    gemm_options(gemm_min_m=512)
    KC.case_gemm_rowdot(DEV, BF, 1120, 768, 768, 560)
    KC.case_gemm_rowdot(DEV, torch.float32, 1120, 768, 768, 560)


@covers("maest_gemm_nt", "maest_gemm_tn_ws", "maest_cast_rows", "maest_transpose")
def test_guard_padded_leading_dimensions(gemm_options):
    KC.case_contract_padded_leading_dims(DEV, BF, 300, 519, 768, tn_K=1121)
    gemm_options(gemm_min_m=512)
    KC.case_contract_padded_leading_dims(DEV, BF, 2637, 768, 768, tn_K=1121)
    KC.case_contract_padded_leading_dims(DEV, torch.float32, 1120, 256, 768, tn_K=150)


# ------------------------------------------------------------------------------------------------ GEMM TN
@pytest.mark.parametrize("dtype", [torch.float32, BF])
@covers("maest_gemm_tn_ws")
def test_guard_gemm_tn_token_tail(dtype):
    KC.case_gemm_tn(DEV, dtype, 1121, 768, 3072)
    KC.case_gemm_tn(DEV, dtype, 7, 519, 768, lda_pad=57)


@covers("maest_gemm_tn_ws")
def test_guard_gemm_tn_production_shape_and_workspace():
    """74240 tokens through gemm_tn256o_kernel, automatic and 5 splits; inside the case (tn_reduce = 1) the split-K workspace at exactly
    the size maest_gemm_tn_workspace_bytes reports."""
    with ops.options(tn_reduce=1):
        assert ops.gemm_tn_workspace_bytes(BF, 768, 768, 74240) > 0          # the case's tn_reduce = 1 call does take a workspace
    KC.case_gemm_tn(DEV, BF, 74240, 768, 768, splits=(0, 5))


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("BN", [(3, 281), (2, 321), (1, 875), (1, 129)])
@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows")
def test_guard_attention_bf16(BN):
    KC.case_attention(DEV, BF, *BN)


@pytest.mark.parametrize("BN", [(2, 321), (13, 875)])
@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows")
def test_guard_attention_prescaled_q(BN):
    KC.case_attention(DEV, BF, *BN, qs=True)


@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows")
def test_guard_attention_fp32():
    KC.case_attention(DEV, torch.float32, 1, 129)


@pytest.mark.parametrize("BN", [(3, 290), (1, 29)])
@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows", "maest_gather_head_rows", "maest_scatter_head_rows")
def test_guard_attention_head_rows(BN):
    KC.case_attention_head_rows(DEV, BF, *BN)
    KC.case_contract_attention_rows(DEV, BF, *BN)


@covers("maest_attn_fwd_rows", "maest_scatter_head_rows")
def test_guard_attention_head_rows_fp32_contract():
    KC.case_contract_attention_rows(DEV, torch.float32, 2, 129)


@covers("maest_gemm_nt", "maest_gemm_tn_ws", "maest_attn_fwd_rows", "maest_attn_bwd_rows", "maest_cast_weights_multi")
def test_guard_split_precision():
    KC.case_split_precision(DEV)


@covers("maest_gemm_tn", "maest_attn_fwd", "maest_attn_bwd", "maest_layernorm_bwd", "maest_patch_im2col", "maest_affine_f32",
        "maest_scale_dev_f32")
def test_guard_entries_without_a_wrapper():
    KC.case_entries_without_a_wrapper(DEV, B=2, N=281)


# ------------------------------------------------------------------------------------------------ the rest of the model
@pytest.mark.parametrize("dtype", [torch.float32, BF])
@covers("maest_layernorm_fwd", "maest_add_layernorm_fwd", "maest_layernorm_bwd_headres")
def test_guard_layernorm(dtype):
    KC.case_layernorm(DEV, dtype, 1123)


@covers("maest_patch_im2col_strided", "maest_token_assemble", "maest_token_assemble_bwd", "maest_patch_im2col_bwd",
        "maest_head_pool_fwd", "maest_head_pool_bwd", "maest_embed_pool", "maest_embed_pool_bwd")
def test_guard_patch_embed_and_head():
    KC.case_patch_embed(DEV, torch.float32, 3, 626, patchout=5, mix=True, masked=True, stride=(16, 13), seed=36)
    KC.case_patch_embed(DEV, BF, 3, 626, patchout=5, mix=True, masked=True, stride=(16, 13), seed=36)
    KC.case_head(DEV, 5, 281)
    KC.case_contract_fully_written(DEV, B=3, N=281)


@covers("maest_bce_logits", "maest_sigmoid_mean", "maest_colsum", "maest_scale_f32", "maest_transpose", "maest_cast_weights",
        "maest_cast_weights_multi", "maest_swa_update_multi", "maest_melfile_assemble", "maest_spec_mask")
def test_guard_small_cases(tmp_path):
    KC.case_loss(DEV, 7, 519)
    KC.case_transpose(DEV, BF, 1121, 768)
    KC.case_transpose(DEV, torch.float32, 1121, 768)
    KC.case_swa(DEV)
    KC.case_melfile(DEV, tmp_path)
    KC.case_spec_mask(DEV, 4, 626)


# ------------------------------------------------------------------------------------------------ mel front ends
@covers("maest_logmel", "maest_logmel_bwd")
def test_guard_logmel_forward_and_backward():
    from tests import test_waveform_grad_gpu as WG
    KC.case_mel(DEV, 1, 5000, seed=82)
    KC.case_mel(DEV, 3, 40001, seed=83)          # odd clip length: clips 1, 2 start off the 8-byte grid (the element-wise fetch)
    WG.test_logmel_bwd_kernel_matches_float64_autograd()


@covers("maest_augment_mel", "maest_augment_mel_bwd")
def test_guard_augment_mel_forward_and_backward():
    from maest_amd.preprocess import AugmentMelSTFT
    from tests import augment_mel_grad_cases as C
    S = 33333
    KC.case_augment_mel(DEV, 2, S)
    aug = AugmentMelSTFT().eval()
    wave, g = KC.rnd((2, S), 1, 0.3), KC.rnd((2, 128, 1 + (S - 1) // 320), 2)
    got, _ = C.module_grad(aug, wave, g, DEV)
    C.check(got, wave, g, aug, "guarded, S = 33333")


@covers("maest_logmel_rows_f16", "maest_resample")
def test_guard_mel_extractor_ragged_tracks():
    from maest_amd import mel_extractor as X
    from tests import test_mel_extract_gpu as MX
    KC.case_contract_ragged_tables(DEV)
    rates = [44100, 48000, 16000]
    waves = [MX._seeded(r * 3 + 17 * i, 60 + i) for i, r in enumerate(rates)]
    rows = X.extract(waves, rates, MX.DEV)
    res = X.resample_batch(waves[:1], 44100, MX.DEV)[0]
    w16 = torch.from_numpy(waves[2]).to(MX.DEV)
    assert torch.equal(MX._bits(rows[2]), MX._bits(MX._plain_rows(w16)))           # the 16 kHz track: maest_logmel's own frames
    assert torch.equal(MX._bits(X.extract([res], 16000, MX.DEV)[0]), MX._bits(rows[0]))
    assert all(bool(torch.isfinite(r.float()).all()) for r in rows)


# ------------------------------------------------------------------------------------------------ regularisers
@covers("maest_rng_advance", "maest_dropout", "maest_drop_add", "maest_drop_add_layernorm_fwd", "maest_drop_cast")
def test_guard_regularisers_dense_and_head_token_layouts():
    """The kernel-level regulariser checks of tests/test_emu_regularisers.py (numpy masks, bit-exact fp32 values) on the device, in the
    dense layout and with 2 rows per clip; their tensors are created where the library runs."""
    import numpy as np
    import torch.nn.functional as F
    from tests import regulariser_cases as RC
    from tests import test_emu_regularisers as R
    st = ops.rng_state(R.SEED, DEV, step=7)
    snap = ops.rng_advance(st)
    assert snap.cpu().numpy().view(np.uint32).tolist() == [R.SEED & 0xFFFFFFFF, R.SEED >> 32, 7, 0] and int(st[2]) == 8
    B, N, step = 5, 281, 2
    elem, path = R.PARTS[0]
    for rpc in (N, 2):
        rows = B * rpc
        me, mp = R._branch_mult(B, N, rpc, elem, path, step)
        x, d = KC.rnd((rows, 768), 1), KC.rnd((rows, 768), 2)
        g, b = 1 + 0.1 * KC.rnd((768,), 3), 0.1 * KC.rnd((768,), 4)
        sn = ops.rng_state(R.SEED, DEV, step=step)
        want = (x.reshape(B, rpc, 768) + R._apply(d.reshape(B, rpc, 768), me, mp)).reshape(rows, 768)
        assert torch.equal(ops.drop_add(x.to(DEV), d.to(DEV), B, N, rpc, elem, path, sn).cpu(), want)
        x_new, y, mean, rstd = ops.drop_add_layernorm_fwd(x.to(DEV), d.to(DEV), g.to(DEV), b.to(DEV), 1e-6, torch.float32, B, N, rpc, elem,
                                                          path, sn, save_stats=True)
        assert torch.equal(x_new.cpu(), want)
        KC.close(y, F.layer_norm(want, (768,), g, b, 1e-6), 1e-6, 2e-6, "drop_add_layernorm_fwd y")
        src = KC.rnd((rows, 768), 5)
        dst = ops.drop_cast(src.to(DEV), torch.float32, B, N, rpc, elem, path, sn)
        assert torch.equal(dst.cpu(), R._apply(src.reshape(B, rpc, 768), me, mp).reshape(rows, 768))
        keep = RC.elem_keep(R.SEED, step, 42, 0.1, B, N, 768, tokens=range(rpc)).reshape(rows, 768)
        ones, aux = torch.ones(rows, 768, device=DEV), torch.full((rows, 768), 2.0, device=DEV)
        ops.dropout_(ones, aux, B, N, rpc, 42, 0.1, sn)
        assert np.array_equal(ones.cpu().numpy(), keep.astype(np.float32) * RC.scale(0.1))
        assert np.array_equal(aux.cpu().numpy(), 2 * keep.astype(np.float32) * RC.scale(0.1))


# ------------------------------------------------------------------------------------------------ the half build
@covers("maest_gemm_nt", "maest_attn_fwd_rows", "maest_attn_bwd_rows")
def test_guard_f16_flavour(gemm_options):
    gemm_options(gemm_min_m=512)
    with _lib.flavour("f16"):
        KC.case_gemm(DEV, BF, 2637, 768, 768, identity=False)
        KC.case_attention(DEV, BF, 2, 321)
