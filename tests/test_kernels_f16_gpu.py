"""GPU (`-m gpu`): the half-precision build (libmaest_hip_f16.so, precision="fp16") kernel by kernel on a real MI355X, at the shapes
test_kernels_gpu.py runs the bf16 build at.  Every kernel form is forced through ops.options so that each asm path of the half build --
v_mfma_*_f16, v_cvt_pk_f16_f32, v_dot2c_f32_f16 in gemm_nt_ow.h, gemm_tn_ow.hip and attn_fwd_pw.hip -- runs at least once.  The cases
run through kernel_cases' flavour-aware helpers and kernel_cases.controlled: the same inputs through the bf16 build must come out at
least 4x further from the reference wherever it is above fp32 noise."""
import pytest
import torch

from maest_amd import _lib
from tests import attention_cases as AC
from tests import epilogue_cases as EC
from tests import kernel_cases as KC
from tests import norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16     # the 16-bit container tag of both builds


def test_f16_build_has_the_same_kernel_forms():
    """A half build whose register audit left an owned kernel out would make the forced forms below test the fallback unnoticed."""
    bf = _lib.kernel_forms()
    with _lib.flavour("f16"):
        f16 = _lib.kernel_forms()
    print(f"kernel forms: bf16 build {bf:#x}, half build {f16:#x}")
    assert f16 == bf


@pytest.mark.parametrize("shape", [(1120, 2304, 768), (562, 768, 3072), (300, 400, 768), (300, 519, 768)])
def test_f16_gemm(shape):
    KC.controlled(KC.case_gemm, DEV, BF, *shape)


@pytest.mark.parametrize("variant", [0, 3])
def test_f16_gemm_256_row_tiles(variant, gemm_options):
    """gemm_variant 0: the owned-register one-wave-per-SIMD kernel (asm MFMA / conversions), 3: the eight-wave kernel."""
    gemm_options(gemm_min_m=512, gemm_variant=variant)
    KC.controlled(KC.case_gemm, DEV, BF, 1120, 2304, 768)


def test_f16_gemm_128_row_tiles_forced(gemm_options):
    gemm_options(gemm_min_m=512, gemm_tail=2)
    KC.controlled(KC.case_gemm, DEV, BF, 2560, 768, 3072)


def test_f16_gemm_last_partial_round():
    KC.controlled(KC.case_gemm, DEV, BF, 66000, 768, 768, identity=False)


@pytest.mark.parametrize("shape,opts", [((777, 512, 192), {}), ((2560 + 77, 768, 768), {"gemm_wgs": 8}),
                                        ((2560 + 77, 2304, 768), {"gemm_panel": 2, "gemm_wgs": 24})])
def test_f16_gemm_one_wave_per_simd_kernel(shape, opts, gemm_options):
    """the owned kernel against the eight-wave kernel (both half) in every epilogue form: persistent tile walk, column panels"""
    gemm_options(gemm_min_m=512, gemm_tail=0, **opts)
    KC.controlled(KC.case_gemm_one_wave_per_simd, DEV, *shape)


def test_f16_gemm_rowdot(gemm_options):
    KC.controlled(KC.case_gemm_rowdot, DEV, BF, 74240, 768, 768, 290)
    gemm_options(gemm_min_m=512)
    KC.controlled(KC.case_gemm_rowdot, DEV, BF, 1120, 768, 768, 560)


@pytest.mark.parametrize("shape", [(1121, 768, 3072), (2300, 2304, 768), (64, 400, 768), (7, 519 + 57, 768)])
def test_f16_gemm_tn(shape):
    """small and 256-tile wgrad kernels with colsum, split-K and the workspace combine (tn_reduce = 1, inside case_gemm_tn)"""
    K, M, N = shape
    if M == 519 + 57:
        KC.controlled(KC.case_gemm_tn, DEV, BF, K, 519, N, lda_pad=57)
    else:
        KC.controlled(KC.case_gemm_tn, DEV, BF, K, M, N)


@pytest.mark.parametrize("variant", [0, 3])
def test_f16_gemm_tn_256_tiles(variant, gemm_options):
    """gemm_variant 0: gemm_tn256o_kernel (asm MFMA, v_dot2c colsum against MAEST_ONE16X2), 3: the eight-wave kernel"""
    gemm_options(gemm_variant=variant)
    KC.controlled(KC.case_gemm_tn, DEV, BF, 9280, 2304, 768, splits=(0, 1, 5))


def test_f16_transpose_and_casts():
    with _lib.flavour("f16"):      # (exact against the half-rounded reference)
        KC.case_transpose(DEV, BF, 1121, 768)
        KC.case_transpose(DEV, BF, 562, 3072)


def test_f16_layernorm_and_colsum():
    KC.controlled(KC.case_layernorm, DEV, BF, 1123)
    KC.controlled(KC.case_loss, DEV, 64, 400)


# tests/norm_cases.py in the half build: the bounds are those of the fp32 arithmetic, the 16-bit outputs are held to
# the half rounding bracket
def test_f16_layernorm_fwd_on_hard_rows():
    with _lib.flavour("f16"):
        NC.case_layernorm_fwd(DEV, BF, 64)


def test_f16_add_layernorm_fwd_on_hard_rows():
    with _lib.flavour("f16"):
        NC.case_add_layernorm_fwd(DEV, BF, 64)


def test_f16_drop_add_layernorm_fwd_on_hard_rows():
    with _lib.flavour("f16"):
        NC.case_drop_add_layernorm_fwd(DEV, BF, 64, n_tok=43)


def test_f16_layernorm_bwd_on_hard_rows():
    with _lib.flavour("f16"):
        NC.case_layernorm_bwd(DEV, BF, 64, deterministic=(0,))


def test_f16_head_pool_and_loss_on_hard_rows():
    """fp32 kernels: the half build compiles the same sources"""
    with _lib.flavour("f16"):
        NC.case_head_pool(DEV)
        NC.case_loss(DEV)


@pytest.mark.parametrize("BN", [(2, 560), (3, 281), (1, 875), (1, 64), (1, 129)])
def test_f16_attention(BN):
    """every forward form (the persistent attn_fwd_pw kernel above 320 tokens by default, 1, 2, 3) and backward form (fused at N <= 320,
    two-kernel), each against the oracle"""
    KC.controlled(KC.case_attention, DEV, BF, *BN)


@pytest.mark.parametrize("BN", [(2, 560), (24, 290), (13, 875)])
def test_f16_attention_prescaled_q(BN):
    """q_prescaled; (24, 290): the persistent fused backward crossing item boundaries; (13, 875): the persistent forward walking items"""
    KC.controlled(KC.case_attention, DEV, BF, *BN, qs=True)


@pytest.mark.parametrize("BN", [(3, 290), (2, 560)])
def test_f16_attention_restricted_to_the_head_tokens(BN):
    KC.controlled(KC.case_attention_head_rows, DEV, BF, *BN)


@pytest.mark.parametrize("B,N,kw", [(1, 64, {}), (1, 129, {}), (3, 281, {}), (24, 290, {}), (24, 290, {"qs": True}), (2, 321, {}), (2, 560, {}),
                                    (13, 875, {}), (3, 290, {"q_rows": 2})])
def test_f16_attention_calibrated(B, N, kw):
    """Every forward and backward form of the half build inside 1.25 x (rms) / 2 x (max) of the error its own half roundings make (the
    shapes of test_kernels_gpu.py: test_attention_calibrated)."""
    with _lib.flavour("f16"):
        AC.case_attention_calibrated(DEV, B, N, **kw)


@pytest.mark.parametrize("qs", [False, True])
@pytest.mark.parametrize("BN", [(2, 321), (13, 875), (24, 290)])
def test_f16_attention_exact(BN, qs):
    """A forward whose every softmax term is a power of two: each form within one half ulp of the exactly known answer."""
    with _lib.flavour("f16"):
        AC.case_attention_exact(DEV, *BN, qs=qs)


@pytest.mark.parametrize("BN", [(2, 321), (13, 875)])
def test_f16_attention_exact_rescale_paths(BN):
    """The exact forward with the levels that send the persistent kernel down pw_softmax_slow (test_kernels_gpu.py), in the half build."""
    with _lib.flavour("f16"):
        AC.case_attention_exact(DEV, *BN, hot=True)


def test_f16_patch_embed():
    KC.controlled(KC.case_patch_embed, DEV, BF, 3, 626, patchout=30, mix=True, masked=True)


def test_f16_conversions_round_like_torch():
    """cast_weights(_multi), cast_rows and the 16-bit GEMM output of each kernel (128 x 128, owned 256-row, eight-wave, 128-row tiles)
    bit for bit against torch's .half(): also checks the f16 denormal mode the kernels were compiled with."""
    forms = ({"gemm_min_m": 1 << 30}, {"gemm_min_m": 512}, {"gemm_min_m": 512, "gemm_variant": 3}, {"gemm_min_m": 512, "gemm_tail": 2})
    with _lib.flavour("f16"):
        KC.case_half_conversions(DEV, M=1024, N=512, K=64, forms=forms)


def test_f16_gelu_on_the_exact_argument_grid():
    """Every GELU output form (fp32, half, value + gelu' pair) of each kernel on exactly known arguments: inside the error the erf fit's
    documented bound, v_exp / v_rcp and the roundings allow (tests/epilogue_cases.py)."""
    with _lib.flavour("f16"):
        worst = EC.case_gelu_grid(DEV, BF, EC.FORMS_ALL, M=1024, N=512, K=64)
    print("".join(f"\n  {k}: worst err / delta {v:.3f}" for k, v in worst.items()))


def test_f16_mul_and_residual_epilogues_are_exact():
    """mul -> half: one fp32 multiply of acc + bias, one rounding; residual -> fp32: (acc + bias) + res -- bit for bit, each kernel."""
    with _lib.flavour("f16"):
        EC.case_epilogue_exact(DEV, BF, EC.FORMS_ALL, M=1024, N=512, K=64)


def test_f16_gemm_gelu_arguments_where_the_function_bends(gemm_options):
    """Weights scaled by 1 / sqrt(K): nearly every GELU argument inside |x| < 3."""
    with _lib.flavour("f16"):
        KC.case_gemm(DEV, BF, 1120, 2304, 768, wscale=768 ** -0.5)
        gemm_options(gemm_min_m=512)
        KC.case_gemm(DEV, BF, 777, 512, 192, wscale=192 ** -0.5)


@pytest.mark.parametrize("flavour", ["f16", "bf16"])
def test_f16_nonfinite_values_propagate(flavour):
    """inf / NaN reach exactly the outputs they feed, in every kernel form: NT dgrad (128 x 128, owned, eight-wave), TN wgrad + colsum
    (small, owned with v_dot2c, eight-wave, workspace combine), attention backward (fused, two-kernel), layernorm_bwd."""
    gemm = ({}, {"gemm_min_m": 512}, {"gemm_min_m": 512, "gemm_variant": 3})
    tn = ({}, {"gemm_variant": 4}, {"gemm_variant": 3}, {"tn_reduce": 1})
    with _lib.flavour(flavour):
        KC.case_nonfinite(DEV, M=512, N=256, K=512, B=2, Ntok=290, rows=1123, gemm_forms=gemm, tn_forms=tn,
                          attn_forms=({"attn_bwd": 0}, {"attn_bwd": 1}))
