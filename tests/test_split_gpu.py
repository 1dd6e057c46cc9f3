"""GPU (`-m gpu`): the split-bf16 ("bf16x3") kernels -- what a plain `model.eval()(x)` runs -- at the shapes and edges the bf16 kernels get,
through the gate of tests/split_cases.py: the kernel's error against fp64 within 1.25 x (rms) / 2 x (max) of what an fp64 model of its
roundings shows, the same call on plain fp32 operands different, on plain bf16 operands at least 10 x outside.  Ragged last row tiles (every
real batch: 2 x 281, 3 x 281, 1120 rows), K below the five-unit prologue, the two-launch tail split, every epilogue, the row-dot side
output; the one-GEMM-over-3K route the default evaluation launches; the TN kernel at shapes it takes by default, every split_k, padded
leading dimensions, the workspace combine and the ordered mode; attention at N a multiple of 64 (the one unmasked case) and of 128, just
past a tile, the 30 s rows, the rescale spike, the head-row pass and the backward."""
import pytest
import torch

from maest_amd import _lib, ops
from tests import guard
from tests import split_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
COVERED = set()
LIMIT = 600              # seconds, per guarded test (tests.guard.covering)
covers = lambda *entries: guard.covering(COVERED, *entries, limit=LIMIT)

NT_SHAPES = [(549, 256, 32), (549, 256, 64), (549, 256, 96), (549, 256, 160), (562, 768, 3072), (843, 768, 768), (1120, 2304, 768)]


# ------------------------------------------------------------------------------------------------ NT GEMM
@pytest.mark.parametrize("shape", NT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_gemm_nt_ragged_rows(shape, gemm_options):
    """Ragged last row tiles; K = 32, 64, 96 below the five-unit prologue (1, 2, 3 stages) and 160 at it; 2 and 3 clips of 281, 2 of 560."""
    gemm_options(gemm_min_m=512)
    SC.case_nt(DEV, *shape)


def test_split_gemm_nt_two_launch_tail():
    """22172 rows x 768: 261 tiles = one round and 5: 85 row tiles in one launch, the last 412 rows in 128-row tiles (gemm_tail = 1, the default)."""
    assert ops.get_option("gemm_tail") == 1 and ops.get_option("gemm_min_m") <= 22172
    SC.case_nt(DEV, 22172, 768, 64)


@pytest.mark.parametrize("opts", [{}, {"gemm_epilogue": 0}, {"gemm_epilogue": 1}, {"gemm_tail": 2}], ids=["default", "epilogue0", "epilogue1", "tail2"])
def test_split_gemm_nt_epilogues(opts, gemm_options):
    """(843, 768, 768): MUL beside bias and RESIDUAL, in the two-pass and the four-pass epilogue form and in 128-row tiles."""
    gemm_options(gemm_min_m=512, **opts)
    SC.case_nt(DEV, 843, 768, 768, epis=("none + bias", "residual", "mul"), what=f"NT (843, 768, 768) {opts}")


@pytest.mark.parametrize("opts", [{}, {"gemm_tail": 2}], ids=["default", "tail2"])
def test_split_gemm_nt_gelu_with_side_output(opts, gemm_options):
    gemm_options(gemm_min_m=512, **opts)
    SC.case_nt_gelu(DEV, 843, 768, 768)


def test_split_gemm_nt_rowdot(gemm_options):
    gemm_options(gemm_min_m=512)
    SC.case_nt_rowdot(DEV, 562, 768, 768, 281)


def test_split_gemm_nt_fallback_shapes_are_exact_fp32(gemm_options):
    """M < 512 and N % 256 != 0 run the exact fp32 kernel (gemm_nt256_try returns -1); K % 32 != 0 is no fall-back but an argument error of
    maest_gemm_nt for fp32 operands of either kind."""
    gemm_options(gemm_min_m=512)
    SC.case_nt_fallback(DEV, 300, 256, 64)
    SC.case_nt_fallback(DEV, 549, 200, 64)
    with pytest.raises(_lib.MaestHipError, match="multiple of 32"):
        ops.gemm_nt(torch.zeros(549, 48, device=DEV), torch.zeros(256, 48, device=DEV), None, out_dtype=torch.float32, x3=True)


# ------------------------------------------------------------------------------------------------ one bf16 GEMM over 3 K
@pytest.mark.parametrize("shape,epi", [((843, 2304, 768), "none"), ((843, 768, 768), "residual"), ((843, 3072, 768), "gelu"), ((843, 768, 3072), "residual")],
                         ids=["qkv", "proj", "fc1", "fc2"])
def test_split_gemm_over_3k(shape, epi, gemm_options):
    """[hi | hi | lo] activation rows x cast_weights_multi(.., SPLIT3) weights through the bf16 kernels: the four GEMMs of a block at 3 clips of 281
    tokens; fc1 writes its GELU as fp32 and as split rows."""
    gemm_options(gemm_min_m=512)
    SC.case_nt_over_3k(DEV, *shape, epi=epi, split_out=epi == "gelu")


def test_split_gemm_over_3k_128_tile_kernel():
    """150 rows: the 128 x 128 kernel (the last block's head-token rows)."""
    SC.case_nt_over_3k(DEV, 150, 768, 768)


# ------------------------------------------------------------------------------------------------ TN GEMM
@pytest.mark.parametrize("shape", [(128, 768, 768), (144, 768, 768), (304, 768, 768), (1120, 2304, 768), (4496, 768, 3072)], ids=lambda s: "x".join(map(str, s)))
def test_split_gemm_tn(shape):
    """Shapes gemm_tn256_kernel<float, true> takes by default (M N >= 8 x 65536): its minimum depth (8 slices), a ragged slice count, the token
    counts of 2 x 560 and 16 x 281; split_k 1, 3 and automatic, with colsum."""
    SC.case_tn(DEV, *shape)


def test_split_gemm_tn_padded_leading_dimension():
    SC.case_tn(DEV, 304, 768, 768, lda_pad=64)


def test_split_gemm_tn_workspace_combine(gemm_options):
    gemm_options(tn_reduce=1)
    assert ops.gemm_tn_workspace_bytes(torch.float32, 768, 768, 304, 0, x3=True) > 0
    SC.case_tn(DEV, 304, 768, 768, splits=(3, 0), workspace=True, what="TN (304, 768, 768), tn_reduce = 1")


def test_split_gemm_tn_deterministic(gemm_options):
    """deterministic = 1: the split kernel with its partials of C and of colsum ordered through the workspace; a single split has no workspace
    form in the 256-tile kernel and leaves for the exact fp32 one-writer kernel (gemm_tn256_try: `if (!use_ws) return -1`)."""
    gemm_options(deterministic=1)
    assert ops.gemm_tn_workspace_bytes(torch.float32, 768, 768, 304, 0, x3=True) > 0
    SC.case_tn(DEV, 304, 768, 768, splits=(3, 0), workspace=True, what="TN (304, 768, 768), deterministic = 1")
    SC.case_tn_fallback(DEV, 304, 768, 768, split_k=1)


def test_split_gemm_tn_fallback_shapes_are_exact_fp32():
    """M % 256 != 0, K % 16 != 0, K < 128, and M N < 8 x 65536 without gemm_variant = 4: tn256_plan returns false."""
    for K, M, N in ((144, 700, 768), (136, 768, 768), (112, 768, 768), (144, 768, 512)):
        assert not SC.tn_takes_split(M, N, K)
        SC.case_tn_fallback(DEV, K, M, N)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("BN", [(1, 64), (1, 128), (2, 129), (3, 281), (2, 320), (2, 321), (1, 875), (1, 1685)], ids=lambda s: "x".join(map(str, s)))
def test_split_attention_forward(BN):
    """N = 64 (the one length at which attn_fwd_x3s_kernel skips its key mask on a single tile), 128 and 320 (multiples of 64 with several
    tiles), one key past a tile (129, 321), the training length and the 30 s rows."""
    SC.case_attn_fwd(DEV, *BN)


@pytest.mark.parametrize("BN", [(1, 290), (2, 560)], ids=lambda s: "x".join(map(str, s)))
def test_split_attention_forward_rescale_branch(BN):
    SC.case_attn_fwd(DEV, *BN, spike=True)


@pytest.mark.parametrize("BN", [(3, 281), (2, 321)], ids=lambda s: "x".join(map(str, s)))
def test_split_attention_head_rows(BN):
    SC.case_attn_fwd(DEV, *BN, head_rows=True)


@pytest.mark.parametrize("BN", [(1, 64), (2, 129), (3, 281), (2, 321), (1, 875)], ids=lambda s: "x".join(map(str, s)))
def test_split_attention_backward(BN):
    SC.case_attn_bwd(DEV, *BN)


def test_split_attention_backward_rescale_branch():
    SC.case_attn_bwd(DEV, 1, 290, spike=True)


# ------------------------------------------------------------------------------------------------ inside guarded arenas
@covers("maest_gemm_nt")
def test_guard_split_gemm_nt_ragged_rows(gemm_options):
    gemm_options(gemm_min_m=512)
    SC.case_nt(DEV, 549, 256, 96)
    SC.case_nt(DEV, 843, 768, 768)


@covers("maest_gemm_tn_ws")
def test_guard_split_gemm_tn():
    SC.case_tn(DEV, 304, 768, 768, lda_pad=64)


@covers("maest_attn_fwd_rows", "maest_attn_bwd_rows")
def test_guard_split_attention_one_past_a_tile():
    SC.case_attn_fwd(DEV, 2, 321)
    SC.case_attn_bwd(DEV, 2, 321)
