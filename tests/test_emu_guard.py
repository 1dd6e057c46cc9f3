"""CPU (`-m "not gpu"`): the cases of the emulator tests once more inside tests/guard.py's guarded(): every tensor argument in an arena
with NaN-pattern bands, every buffer ops allocates pre-filled with the pattern.  The cases keep all their assertions and tolerances; on
top come the bitwise checks of the guard (bands intact, const arguments unchanged) and the memory-contract cases of
tests/kernel_cases.py.  One or two shapes per entry point, with ragged M / N / K / token counts and a last clip of a batch; trimmed to
keep the CPU suite short.  At the end: the proof that the guard can fail -- mutated CALLS (never kernels), each
reported by name.  These tests carry no `gpu` marker: the mutations make a kernel touch a band on purpose, which belongs on the
emulator only."""
import pytest
import torch

from maest_amd import _lib, ops
from tests import guard
from tests import kernel_cases as KC

BF = torch.bfloat16
COVERED = set()          # entry points the tests below require a guarded call of (tests/test_guard_cpu.py walks _lib.SIGNATURES against it)
covers = lambda *entries: guard.covering(COVERED, *entries)


@pytest.fixture
def emu16():
    from tests.emu import build_emu
    if not build_emu.available():
        pytest.skip("host clang for the emulator build is not available")
    _lib._testing_override(build_emu.build(), build_emu.build(f16=True))
    yield "cpu"
    _lib._testing_restore()


# ------------------------------------------------------------------------------------------------ GEMMs
@pytest.mark.parametrize("dtype", [torch.float32, BF])
@covers("maest_gemm_nt")
def test_guard_gemm_ragged(emu, dtype):
    KC.case_gemm(emu, dtype, 150, 200, 64 if dtype == torch.float32 else 128)      # ragged M and N of the 128 x 128 kernel
    # (N = 51, the scalar epilogue: test_guard_padded_leading_dimensions)


@covers("maest_gemm_nt")
def test_guard_gemm_256_row_tiles(emu, gemm_options):
    """The one-wave-per-SIMD kernel's twin and the eight-wave kernel on a ragged second tile row (520 rows); one workgroup walking both
    tiles; 128-row tiles forced onto 4.5 tiles (576 rows)."""
    gemm_options(gemm_min_m=512, gemm_tail=0)
    KC.case_gemm_one_wave_per_simd(emu, 520, 256, 128, only=("none -> bf16", "residual -> fp32"), pair=False)
    gemm_options(gemm_wgs=1)
    KC.case_gemm_one_wave_per_simd(emu, 520, 256, 64, only=("mul -> bf16",), pair=False)
    gemm_options(gemm_wgs=0, gemm_tail=2)
    KC.case_gemm(emu, BF, 576, 256, 128, identity=False)


@covers("maest_gemm_nt_rowdot")
def test_guard_gemm_rowdot(emu, gemm_options):
    KC.case_gemm_rowdot(emu, BF, 150, 128, 128, 75)
    gemm_options(gemm_min_m=512, gemm_tail=2)
    KC.case_gemm_rowdot(emu, BF, 576, 256, 128, 96)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@covers("maest_gemm_tn_ws")
def test_guard_gemm_tn_ragged(emu, dtype):
    if dtype == BF:          # (fp32: four times the emulated MFMAs; a ragged K = 70 runs in test_guard_padded_leading_dimensions)
        KC.case_gemm_tn(emu, dtype, 150, 136, 200)              # K = 150: the token tail
    KC.case_gemm_tn(emu, dtype, 40, 24, 72, lda_pad=8)


@covers("maest_gemm_tn_ws")
def test_guard_gemm_tn_256_tiles_and_workspace(emu, gemm_options):
    """gemm_tn256o_kernel's twin with 5 + 4 slices, and (inside the case, tn_reduce = 1) the split-K workspace at exactly the size
    maest_gemm_tn_workspace_bytes reports."""
    gemm_options(gemm_variant=4)
    with ops.options(tn_reduce=1):
        assert ops.gemm_tn_workspace_bytes(BF, 256, 512, 288) > 0          # the case's tn_reduce = 1 call does take a workspace
    KC.case_gemm_tn(emu, BF, 288, 256, 512, splits=(2,))


@covers("maest_gemm_nt", "maest_gemm_tn_ws", "maest_cast_rows", "maest_transpose")
def test_guard_padded_leading_dimensions(emu):
    KC.case_contract_padded_leading_dims(emu, BF, 150, 200, 128)
    KC.case_contract_padded_leading_dims(emu, torch.float32, 70, 51, 64)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@covers("maest_transpose", "maest_cast_weights", "maest_cast_weights_multi")
def test_guard_transpose_and_casts(emu, dtype):
    KC.case_transpose(emu, dtype, 70, 130)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@covers("maest_layernorm_fwd", "maest_add_layernorm_fwd", "maest_layernorm_bwd_headres")
def test_guard_layernorm(emu, dtype):
    KC.case_layernorm(emu, dtype, 11)


# ------------------------------------------------------------------------------------------------ attention
@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows")
def test_guard_attention_bf16_last_clip_of_two(emu):
    """(B, N) = (2, 75): two key tiles, the second ragged; the last clip's tail rows end at the end of qkv / out / dout / lse.  Forward
    forms 0 / 1 / 2 / 3, backward fused, two-kernel (DMA-fed and register-staged)."""
    KC.case_attention(emu, BF, 2, 75)


@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows")
def test_guard_attention_fp32(emu):
    KC.case_attention(emu, torch.float32, 1, 40)


@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows", "maest_gather_head_rows", "maest_scatter_head_rows")
def test_guard_attention_head_rows(emu):
    KC.case_attention_head_rows(emu, BF, 2, 40)
    KC.case_contract_attention_rows(emu, BF, 2, 40)
    KC.case_contract_attention_rows(emu, torch.float32, 1, 20)


@covers("maest_gemm_tn", "maest_attn_fwd", "maest_attn_bwd", "maest_layernorm_bwd", "maest_patch_im2col", "maest_affine_f32",
        "maest_scale_dev_f32")
def test_guard_entries_without_a_wrapper(emu):
    KC.case_entries_without_a_wrapper(emu, B=2, N=24)


# ------------------------------------------------------------------------------------------------ embedding, head, loss
@covers("maest_patch_im2col_strided", "maest_token_assemble", "maest_token_assemble_bwd", "maest_spec_mask")
def test_guard_patch_embed(emu):
    KC.case_patch_embed(emu, torch.float32, 2, 70, patchout=1, mix=True, masked=True, stride=(16, 13), seed=35)
    KC.case_patch_embed(emu, BF, 2, 66, patchout=2)
    KC.case_spec_mask(emu, 2, 40)


@covers("maest_head_pool_fwd", "maest_head_pool_bwd", "maest_embed_pool", "maest_embed_pool_bwd", "maest_patch_im2col_bwd")
def test_guard_head_and_fully_written_outputs(emu):
    KC.case_head(emu, 3, 7)
    KC.case_contract_fully_written(emu)


@covers("maest_bce_logits", "maest_sigmoid_mean", "maest_colsum", "maest_scale_f32", "maest_swa_update_multi", "maest_melfile_assemble")
def test_guard_loss_swa_melfile(emu, tmp_path):
    KC.case_loss(emu, 7, 51)
    KC.case_swa(emu)
    KC.case_melfile(emu, tmp_path)


# ------------------------------------------------------------------------------------------------ mel front ends
@covers("maest_logmel", "maest_logmel_bwd")
def test_guard_logmel_forward_and_backward(emu):
    from tests import test_emu_logmel_bwd as LB
    KC.case_mel(emu, 2, 4001, seed=85)           # odd S: the second clip starts off the 8-byte grid; its tail ends the buffer
    LB._check(KC.rnd((2, 4001), 4101, 0.3), 4201, "guarded, B = 2, odd S")       # work = B * T * 512 floats exactly


@covers("maest_augment_mel", "maest_augment_mel_bwd")
def test_guard_augment_mel_forward_and_backward(emu):
    from tests import test_emu_augment_mel_bwd as AB
    KC.case_augment_mel(emu, 1, 4000)
    AB._eval_case(KC.rnd((2, 4001), 4101, 0.3), 4201, "guarded, B = 2, odd S")   # work = B * T * 1024 floats exactly


@covers("maest_logmel_rows_f16", "maest_resample")
def test_guard_mel_extractor_ragged_tracks(emu):
    from maest_amd import mel_extractor as X
    KC.case_contract_ragged_tables(emu)
    waves = [KC.rnd((r // 8 + 11 * i,), 40 + i, 0.3) for i, r in enumerate((44100, 16000, 8000))]
    rows = X.extract(waves, [44100, 16000, 8000], "cpu")
    assert all(bool(torch.isfinite(r.float()).all()) for r in rows)


# ------------------------------------------------------------------------------------------------ regularisers
@covers("maest_rng_advance", "maest_dropout", "maest_drop_add", "maest_drop_add_layernorm_fwd", "maest_drop_cast")
def test_guard_regularisers_dense_and_head_token_layouts(emu):
    from tests import test_emu_regularisers as R
    R.test_emu_rng_advance_snapshots_then_steps(emu)
    for rpc in (7, 2):
        R.test_emu_dropout_mask_is_the_numpy_mask(emu, 768, rpc, 0.1)
    for rpc in (6, 2):
        R.test_emu_drop_add_and_layernorm_fp32(emu, *R.PARTS[0], rpc)


# ------------------------------------------------------------------------------------------------ the half build
@covers("maest_gemm_nt", "maest_attn_fwd_rows", "maest_attn_bwd_rows", "maest_drop_add_layernorm_fwd")
def test_guard_f16_flavour(emu16):
    from tests import test_emu_regularisers as R
    with _lib.flavour("f16"):
        KC.case_gemm(emu16, BF, 150, 200, 128)
        KC.case_attention(emu16, BF, 1, 20)
    R.test_emu_drop_kernels_16bit(emu16, True, 2)


# ------------------------------------------------------------------------------------------------ the guard can fail
def _gemm_operands(M=70, N=51, K=64):
    return KC.rnd((M, K), 1).bfloat16(), KC.rnd((N, K), 2).bfloat16()


def test_guard_reports_a_read_past_the_end(emu):
    """attn_fwd on a qkv tensor one row short: the last key row of the last clip lies in the band -- that clip's result is NaN, the
    other clip's is not."""
    B, N = 2, 40
    qkv = KC.rnd((B * N, 2304), 3).bfloat16()
    with guard.guarded() as g:
        good = ops.attn_fwd(qkv, B, N, 0.125)
        bad = _attn_fwd_unchecked(qkv[:-1].clone(), B, N)          # a storage of B * N - 1 rows
    assert g.calls["maest_attn_fwd_rows"] == 2
    assert bool(torch.isfinite(good.float()).all())
    b3 = bad.float().reshape(B, N, 768)
    assert bool(torch.isfinite(b3[0]).all()) and bool(torch.isnan(b3[1]).all()), "the row in the band did not reach the last clip's result"


def _attn_fwd_unchecked(qkv, B, N):
    """ops.attn_fwd without its shape assertion (the mutation: a tensor one row short)."""
    out = ops.torch.empty((B * N, 768), dtype=qkv.dtype, device=qkv.device)
    ops.call("maest_attn_fwd_rows", ops._p(qkv), ops._p(out), None, B, N, ops.DT[qkv.dtype], 0.125, N, ops._s(qkv))
    return out


def test_guard_reports_a_write_past_the_end(emu):
    """gemm_nt into an `out` one row short: the last row's store lands in the rear band; the report names the entry, the argument and
    the offset."""
    a, b = _gemm_operands()
    out = torch.zeros((70, 51), dtype=torch.float32)[:-1].clone()          # 69 rows of storage
    with guard.guarded():
        with pytest.raises(guard.GuardError, match=r"maest_gemm_nt: argument 5: the band BEHIND the storage was modified, first at byte \+[0-3] "):
            ops.gemm_nt(a, b, None, out=out, M=70)


def test_guard_reports_use_before_write(emu):
    """EPI_ATOMIC accumulates into C: an output the caller did not zero -- under the guard: the pattern -- gives NaN, deterministically."""
    a, b = _gemm_operands()
    with guard.guarded():
        acc = ops.torch.empty((70, 51), dtype=torch.float32)
        ops.gemm_nt(a, b, None, out=acc, epi=ops.EPI_ATOMIC, split_k=2)
        assert bool(torch.isnan(acc).all())
        zero = torch.zeros((70, 51), dtype=torch.float32)
        ops.gemm_nt(a, b, None, out=zero, epi=ops.EPI_ATOMIC, split_k=2)
        assert bool(torch.isfinite(zero).all())


def test_guard_refuses_an_argument_it_did_not_relocate(emu):
    """A workspace withheld from relocation (as a wrapper that marshals a pointer past the layer would): "unguarded argument"."""
    tok = torch.tensor([[0, 0], [2, 0]], dtype=torch.int32)
    dcols = KC.rnd((2 * 2, 256), 13)
    n_work = 3 * 1
    with guard.guarded(withhold=lambda t: t.dtype == torch.int32 and t.numel() == n_work) as g:
        with pytest.raises(guard.GuardError, match="maest_patch_im2col_bwd: unguarded argument 15"):
            ops.patch_im2col_bwd(dcols, (2, 36, 16), torch.float32, tok)
    assert not g.calls
    with guard.guarded():                                     # and a pointer array element the layer cannot trace
        saved = ops._chk
        ops._chk = lambda *ts: None
        try:
            with pytest.raises(guard.GuardError, match=r"maest_swa_update_multi: unguarded argument 1\[0\]"):
                ops.swa_update_multi([torch.zeros(5)], [torch.ones(5)], 0.5)
        finally:
            ops._chk = saved


def test_guard_restores_ops_and_leaves_it_unchanged_when_off(emu):
    before = (ops.call, ops._p, ops._chk, ops.torch)
    with guard.guarded():
        assert ops.torch is not torch
        with pytest.raises(guard.GuardError, match="do not nest"):
            guard.guarded().__enter__()
    assert (ops.call, ops._p, ops._chk, ops.torch) == before and ops.torch is torch
    a, b = _gemm_operands()
    plain = ops.gemm_nt(a, b, None, out_dtype=torch.float32)
    with guard.guarded():
        guarded_ = ops.gemm_nt(a, b, None, out_dtype=torch.float32)
    assert torch.equal(plain, guarded_)
