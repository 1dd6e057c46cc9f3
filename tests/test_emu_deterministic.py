"""CPU (`-m "not gpu"`): the deterministic mode (MAEST_OPT_DETERMINISTIC, include/maest_hip.h) under the SIMT lockstep emulator, at the
smallest shapes at which each ordered form can go wrong.  The cases are tests/deterministic_cases.py's; the GPU runs them at the
device's shapes (tests/test_deterministic_gpu.py).  The emulator is sequential, so repeated runs can only differ through uninitialised
memory: what these tests pin is the documented ORDER (bit for bit against fp32 loops), the parked-row bookkeeping of the LayerNorm
backward, the workspace sizes under the guard, and that the existing gates of tests/kernel_cases.py hold under the option."""
import pytest
import torch

from maest_amd import _lib, ops
from tests import deterministic_cases as DC
from tests import guard
from tests import kernel_cases as KC

BF = torch.bfloat16


@pytest.fixture
def emu16():
    from tests.emu import build_emu
    if not build_emu.available():
        pytest.skip("host clang for the emulator build is not available")
    _lib._testing_override(build_emu.build(), build_emu.build(f16=True))
    yield "cpu"
    _lib._testing_restore()


# ------------------------------------------------------------------------------------------------ documented order, exact
def test_emu_exact_order_small_kernel(emu):
    """gemm_tn_kernel's workspace form: 136 x 200 (ragged in M and N: two tiles each way), K = 1024 = four splits of four slices"""
    DC.case_exact_order(emu, BF, 1024, 136, 200, expect_bytes=DC.ws_bytes_small(136, 200))


def test_emu_exact_order_small_kernel_fp32(emu):
    DC.case_exact_order(emu, torch.float32, 512, 40, 72, expect_bytes=DC.ws_bytes_small(40, 72))


def test_emu_exact_order_one_wave_per_simd_kernel(emu, gemm_options):
    """gemm_tn256o_kernel's twin leaves its accumulators in the layout tn256_reduce_kernel<true> reads: one 256 x 256 tile under
    gemm_variant = 4, K = 512 = four splits of four slices"""
    gemm_options(gemm_variant=4)
    assert _lib.kernel_forms() & _lib.FORM_GEMM_TN_OW
    DC.case_exact_order(emu, BF, 512, 256, 256, expect_bytes=DC.ws_bytes_256(256, 256))


def test_emu_exact_order_one_wave_per_simd_kernel_half_build(emu16, gemm_options):
    """the same in the half build (2^12 x 2^12 products; its column-sum case needs 2^14 tokens: GPU)"""
    gemm_options(gemm_variant=4)
    with _lib.flavour("f16"):
        DC.case_exact_order(emu16, BF, 512, 256, 256, expect_bytes=DC.ws_bytes_256(256, 256))


def test_emu_two_j_tiles_share_the_column_sums(emu, gemm_options):
    """256 x 512: the j-tiles of a split take its slices in turn, so a split's column sum is two rows of partials"""
    gemm_options(gemm_variant=4)
    DC.case_exact_order(emu, BF, 512, 256, 512, expect_bytes=DC.ws_bytes_256(256, 512))


# ------------------------------------------------------------------------------------------------ repeatable, and still right
def test_emu_repeat_gemm_tn(emu, gemm_options):
    DC.case_repeat_gemm_tn(emu, BF, 150, 136, 200)                   # automatic splits, ragged K
    DC.case_repeat_gemm_tn(emu, BF, 200, 24, 72, split_k=3, lda_pad=8)
    gemm_options(gemm_variant=4)
    DC.case_repeat_gemm_tn(emu, BF, 288, 256, 256, split_k=2)        # 5 + 4 slices on the one-wave-per-SIMD twin


def test_emu_gemm_tn_case_under_the_option(emu, gemm_options):
    with ops.thread_options(deterministic=1):
        KC.case_gemm_tn(emu, BF, 150, 136, 200)
        KC.case_gemm_tn(emu, torch.float32, 40, 24, 72, lda_pad=8)
        gemm_options(gemm_variant=4)
        KC.case_gemm_tn(emu, BF, 288, 256, 512, splits=(2,))


def test_emu_gemm_tn_without_a_workspace_has_one_writer(emu):
    """maest_gemm_tn (no workspace) under the option: one split -- the result does not depend on the split count asked for, and is the
    single-split result of the default form bit for bit"""
    a, b = KC.lp(DC.heavy((200, 24), 1)), KC.lp(DC.heavy((200, 72), 2))
    outs = []
    for det, sk in ((0, 1), (1, 3), (1, 0)):
        with ops.thread_options(deterministic=det):
            out, cs = torch.zeros(24, 72), torch.zeros(24)
            _lib.call("maest_gemm_tn", ops._p(a), a.stride(0), ops._p(b), b.stride(0), _lib.BF16, ops._p(out), 72, 24, 72, 200,
                      ops._p(cs), sk, None)
            outs.append((out, cs))
    DC.same_bits(outs, "maest_gemm_tn without a workspace")


@pytest.mark.parametrize("blocks,rows", [(2, 1), (2, 5), (2, 11), (3, 15), (1024, 33)])
def test_emu_repeat_layernorm_bwd(emu, gemm_options, blocks, rows):
    """rows = 4 blocks + 3 at caps of 2 and 3 workgroups (the grid-stride loop with a ragged last round), one row (one workgroup: the
    default form serves), five rows (two workgroups, four parked rows of five), 33 under the default cap"""
    gemm_options(ln_bwd_blocks=blocks)
    DC.case_repeat_layernorm_bwd(emu, BF, rows, runs=2)


def test_emu_repeat_layernorm_bwd_head_rows(emu, gemm_options):
    gemm_options(ln_bwd_blocks=2)
    DC.case_repeat_layernorm_bwd(emu, BF, 15, head_tokens=(5, 2), runs=2)
    DC.case_repeat_layernorm_bwd(emu, torch.float32, 10, head_tokens=(5, 2), runs=2)


def test_emu_layernorm_and_head_cases_under_the_option(emu):
    with ops.thread_options(deterministic=1):
        KC.case_layernorm(emu, BF, 33)
        KC.case_layernorm(emu, torch.float32, 11)
        KC.case_head(emu, 3, 5)


def test_emu_repeat_head_pool_bwd(emu):
    DC.case_repeat_head_pool_bwd(emu, 1, runs=2)
    DC.case_repeat_head_pool_bwd(emu, 7, runs=2)


@pytest.mark.parametrize("B", [1, 5])
def test_emu_token_tables_in_the_documented_order(emu, B):
    DC.case_repeat_token_assemble_bwd(emu, BF, B, runs=2)


def test_emu_patch_embed_case_under_the_option(emu):
    with ops.thread_options(deterministic=1):
        KC.case_patch_embed(emu, BF, 2, 66, patchout=2)


def test_emu_colsum_in_the_documented_order(emu):
    DC.case_repeat_colsum(emu, BF, 1100, 40, runs=2)        # three chunks, the last ragged
    DC.case_repeat_colsum(emu, torch.float32, 7, 300, runs=2)


# ------------------------------------------------------------------------------------------------ under the guard
def test_emu_guard_ordered_forms(emu, gemm_options):
    """Every ordered form between NaN bands: the workspace at exactly the reported size (ops.gemm_tn allocates that), the parked rows
    inside dx_out, dgamma / dbeta and the tables' bands intact, const arguments unchanged."""
    with guard.guarded() as g:
        DC.case_repeat_gemm_tn(emu, BF, 150, 136, 200, runs=1)
        DC.case_repeat_layernorm_bwd(emu, BF, 11, runs=1)
        DC.case_repeat_layernorm_bwd(emu, BF, 10, head_tokens=(5, 2), runs=1)
        DC.case_repeat_head_pool_bwd(emu, 3, runs=1)
        DC.case_repeat_token_assemble_bwd(emu, BF, 5, runs=1)
        DC.case_repeat_colsum(emu, BF, 600, 40, runs=1)
        gemm_options(gemm_variant=4)
        DC.case_repeat_gemm_tn(emu, BF, 288, 256, 512, split_k=2, runs=1)
    for name in ("maest_gemm_tn_ws", "maest_layernorm_bwd_headres", "maest_head_pool_bwd", "maest_token_assemble_bwd", "maest_colsum"):
        assert g.calls[name], name
