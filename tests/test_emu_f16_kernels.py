"""CPU (`-m "not gpu"`): the half-precision build of the kernel sources (-DMAEST_16BIT_F16, libmaest_hip_f16.so: precision="fp16")
under the SIMT lockstep emulator (tests/emu), at the shapes of test_emu_kernels.py.  Every case runs through the flavour-aware helpers of
kernel_cases (16-bit containers holding IEEE half bits) against references on half-rounded operands, then -- kernel_cases.controlled --
on the same inputs in the bf16 build, whose errors above fp32 noise must be at least 4x the half build's.  The emulator runs the C++
twins of the owned-register asm kernels: this covers the flavour's C++ paths and its dispatch; the asm is tests/test_kernels_f16_gpu.py's."""
import pytest
import torch

from maest_amd import _lib, ops
from tests import attention_cases as AC
from tests import epilogue_cases as EC
from tests import kernel_cases as KC
from tests import norm_cases as NC
from tests.test_emu_grad_kernels import _case, _im2col_ref, _stripes

BF = torch.bfloat16     # the 16-bit container tag of both builds


@pytest.fixture
def emu16():
    """Both emulator builds bound: the bf16 one, and the half one that `with _lib.flavour("f16")` calls go to."""
    from tests.emu import build_emu
    if not build_emu.available():
        pytest.skip("host clang for the emulator build is not available")
    _lib._testing_override(build_emu.build(), build_emu.build(f16=True))
    yield "cpu"
    _lib._testing_restore()


def test_emu_f16_call_without_a_half_build_raises(emu):
    """Only the bf16 emulator build bound (the conftest fixture): a flavour("f16") call must fail, never run the bf16 kernels on half bits."""
    with _lib.flavour("f16"):
        with pytest.raises(_lib.MaestHipError, match="half-precision emulator build"):
            ops.gemm_nt(KC.rnd((64, 64), 0).bfloat16(), KC.rnd((64, 64), 1).bfloat16(), None, out_dtype=torch.float32)


def test_emu_f16_builds_report_the_same_kernel_forms(emu16):
    bf = _lib.kernel_forms()
    with _lib.flavour("f16"):
        assert _lib.kernel_forms() == bf


def test_emu_f16_gemm(emu16):
    """NT GEMM of the 128 x 128 kernel: NONE / GELU with aux / RESIDUAL / MUL / split-K, fp32 and 16-bit outputs, ragged N."""
    KC.controlled(KC.case_gemm, emu16, BF, 150, 200, 128)
    KC.controlled(KC.case_gemm, emu16, BF, 70, 51, 64)


def test_emu_f16_gemm_gelu_arguments_where_the_function_bends(emu16, gemm_options):
    """Weights scaled by 1 / sqrt(K): nearly every GELU argument inside |x| < 3 -- the 128 x 128 kernel, then the 256-row-tile kernels (against the
    rounding brackets of kernel_cases.gate_gelu, eight times narrower in half: no control run)."""
    with _lib.flavour("f16"):
        KC.case_gemm(emu16, BF, 150, 200, 128, wscale=128 ** -0.5)
        gemm_options(gemm_min_m=512)
        KC.case_gemm(emu16, BF, 512, 256, 192, identity=False, wscale=192 ** -0.5)


def test_emu_f16_gemm_256_tile_kernels(emu16, gemm_options):
    """The one-wave-per-SIMD kernel's C++ twin against the 8-wave kernel in every epilogue form (bit for bit under the emulator), the
    8-wave kernel itself, and the 128-row tiles of the last partial round (576 rows: ragged)."""
    gemm_options(gemm_min_m=512, gemm_tail=0)
    KC.controlled(KC.case_gemm_one_wave_per_simd, emu16, 520, 256, 128)
    gemm_options(gemm_variant=3)
    KC.controlled(KC.case_gemm, emu16, BF, 512, 256, 128, identity=False)
    gemm_options(gemm_variant=0, gemm_tail=2)
    KC.controlled(KC.case_gemm, emu16, BF, 576, 256, 128, identity=False)


def test_emu_f16_gemm_rowdot(emu16, gemm_options):
    KC.controlled(KC.case_gemm_rowdot, emu16, BF, 150, 128, 128, 75)
    gemm_options(gemm_min_m=512, gemm_tail=2)
    KC.controlled(KC.case_gemm_rowdot, emu16, BF, 576, 256, 128, 96)


def test_emu_f16_gemm_tn(emu16, gemm_options):
    """TN GEMM + colsum (the MAEST_ONE16X2 operand of the column sums) through the small kernel, the 256-tile kernels and the workspace
    combine (tn_reduce = 1, inside case_gemm_tn)."""
    KC.controlled(KC.case_gemm_tn, emu16, BF, 150, 136, 200)
    KC.controlled(KC.case_gemm_tn, emu16, BF, 40, 24, 72, lda_pad=8)
    gemm_options(gemm_variant=4)
    KC.controlled(KC.case_gemm_tn, emu16, BF, 288, 256, 512, splits=(2,))


def test_emu_f16_transpose_and_casts(emu16):
    with _lib.flavour("f16"):      # (exact against the half-rounded reference: a bf16 result could not pass; nothing for a control to compare)
        KC.case_transpose(emu16, BF, 70, 130)


def test_emu_f16_colsum(emu16):
    KC.controlled(KC.case_loss, emu16, 6, 50)


def test_emu_f16_layernorm(emu16):
    """layernorm_fwd / add_layernorm_fwd / layernorm_bwd (16-bit dy in, 16-bit dx out), with the compact head-token form."""
    KC.controlled(KC.case_layernorm, emu16, BF, 11)


def test_emu_f16_layernorm_on_hard_rows(emu16):
    """tests/norm_cases.py in the half build: every LayerNorm entry point with a half y / delta / dy / dx_lp."""
    with _lib.flavour("f16"):
        NC.case_layernorm_fwd(emu16, BF, 4)
        NC.case_add_layernorm_fwd(emu16, BF, 4)
        NC.case_drop_add_layernorm_fwd(emu16, BF, 4, n_tok=9)
        NC.case_layernorm_bwd(emu16, BF, 4, blocks=(None,), deterministic=(0,))


def test_emu_f16_attention(emu16):
    """Forward (every form, persistent included) and backward (fused; two-kernel) on two key tiles."""
    KC.controlled(KC.case_attention, emu16, BF, 1, 75)


def test_emu_f16_attention_prescaled_q(emu16):
    KC.controlled(KC.case_attention, emu16, BF, 1, 40, qs=True)


@pytest.mark.parametrize("B,N", [(2, 40), (1, 20)])
def test_emu_f16_attention_restricted_to_the_head_tokens(emu16, B, N):
    """q_rows = 2 forward / backward and gather_head_rows / scatter_head_rows."""
    KC.controlled(KC.case_attention_head_rows, emu16, BF, B, N)


@pytest.mark.parametrize("B,N,kw", [(1, 75, {}), (2, 40, {}), (1, 40, {"qs": True}), (2, 40, {"q_rows": 2})])
def test_emu_f16_attention_calibrated(emu16, B, N, kw):
    """Every forward and backward form of the half build inside 1.25 x (rms) / 2 x (max) of the error its own half roundings make (the forms
    left to the device: test_emu_kernels.py, test_emu_attention_calibrated)."""
    with _lib.flavour("f16"):
        AC.case_attention_calibrated(emu16, B, N, **kw)


@pytest.mark.parametrize("B,N,qs", [(1, 75, False), (2, 40, False), (1, 40, True)])
def test_emu_f16_attention_exact(emu16, B, N, qs):
    """A forward whose every softmax term is a power of two: each form within one half ulp of the exactly known answer."""
    with _lib.flavour("f16"):
        AC.case_attention_exact(emu16, B, N, qs=qs)


def test_emu_f16_attention_exact_rescale_paths(emu16):
    """The exact forward with the levels that send the persistent kernel's twin down pw_softmax_slow, in the half build."""
    with _lib.flavour("f16"):
        AC.case_attention_exact(emu16, 1, 75, hot=True)


@pytest.mark.parametrize("mix", [False, True])
def test_emu_f16_patch_embed(emu16, mix):
    """patch_im2col(_strided) from fp32 and from half mel input (MAEST_F16, inside the case), token assembly and its backward."""
    KC.controlled(KC.case_patch_embed, emu16, BF, 2, 66, patchout=2, mix=mix, masked=mix)


@pytest.mark.parametrize("mix", [False, True])
def test_emu_f16_input_gradients(emu16, mix):
    """patch_im2col_bwd on 16-bit dcols (to fp32 and to half mel gradients) and embed_pool_bwd with a 16-bit output, in the half build."""
    B, Fdim, T, stride = 3, 42, 46, (10, 10)
    tok, _, _ = _case(B, Fdim, T, stride, seed=7)
    P = tok.shape[0]
    perm = torch.tensor([2, 0, 1], dtype=torch.int32) if mix else None
    lam = torch.tensor([0.7, 0.35, 0.9]) if mix else None
    t_str, f_str = _stripes(B, Fdim, T, 9) if mix else (None, None)
    with _lib.flavour("f16"):
        dcols = KC.lp(KC.rnd((B * P, 256), 11))
        x = torch.zeros((B, Fdim, T), requires_grad=True)
        (_im2col_ref(x, tok, stride, perm, lam, t_str, f_str) * KC.f32(dcols)).sum().backward()
        for x_dtype in (torch.float32, torch.float16):
            got = ops.patch_im2col_bwd(dcols, (B, Fdim, T), x_dtype, tok, perm=perm, lam=lam, t_stripes=t_str, f_stripes=f_str, stride=stride)
            KC.close(got, x.grad.to(x_dtype), 1e-5 if x_dtype == torch.float32 else 1e-3, 1e-5, f"col2im half dcols -> {x_dtype}")
        d = KC.rnd((2, 3 * 768), 21)
        dx, dlp = ops.embed_pool_bwd(d, 7, lp_dtype=BF)
        KC._half_bits_equal(dlp, dx, "embed_pool_bwd 16-bit output")
        # (a bf16 reading of the half dcols is 2^3 .. 2^-3 off: far outside the 1e-5 above)


def test_emu_f16_conversions_round_like_torch(emu16, gemm_options):
    """cast_weights(_multi), cast_rows and a GEMM's 16-bit output (the 128 x 128 kernel, and the one-wave-per-SIMD kernel's twin) against
    torch's .half() bit for bit: round to nearest even, +-inf past 65504, subnormals kept."""
    with _lib.flavour("f16"):
        KC.case_half_conversions(emu16, M=512, N=256, K=64, forms=({"gemm_min_m": 1 << 30}, {"gemm_min_m": 512}))


def test_emu_f16_gelu_on_the_exact_argument_grid(emu16):
    """Every GELU output form of the half build (fp32, half, value + gelu' pair) on the exact-argument grid, inside the error the erf fit's
    documented bound and the roundings allow (tests/epilogue_cases.py)."""
    with _lib.flavour("f16"):
        worst = EC.case_gelu_grid(emu16, BF, ({"gemm_min_m": 1 << 30}, {"gemm_min_m": 512}))
    print("".join(f"\n  {k}: worst err / delta {v:.3f}" for k, v in worst.items()))


def test_emu_f16_mul_and_residual_epilogues_are_exact(emu16):
    """mul -> half: one fp32 multiply of acc + bias, one rounding; residual -> fp32: (acc + bias) + res -- bit for bit on exact accumulators."""
    with _lib.flavour("f16"):
        EC.case_epilogue_exact(emu16, BF, ({"gemm_min_m": 1 << 30}, {"gemm_min_m": 512}))


def test_emu_f16_nonfinite_values_propagate(emu16):
    """inf / NaN in one operand row reach exactly the outputs they feed (NT dgrad, TN wgrad + colsum incl. the workspace combine,
    attention backward fused and two-kernel, layernorm_bwd) -- in the half build and in the bf16 build."""
    kw = dict(tn_forms=({}, {"tn_reduce": 1}), attn_forms=({"attn_bwd": 0}, {"attn_bwd": 1}))
    with _lib.flavour("f16"):
        KC.case_nonfinite(emu16, **kw)
    KC.case_nonfinite(emu16, **kw)
