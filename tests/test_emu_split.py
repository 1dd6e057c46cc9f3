"""CPU (`-m "not gpu"`): the split-bf16 kernels under the SIMT lockstep emulator through the gate of tests/split_cases.py -- the kernel's error
against fp64 within 1.25 x (rms) / 2 x (max) of what its roundings allow, the plain fp32 call different, the plain bf16 call 10 x outside.
The emulator takes seconds per launch: the smallest shapes that reach each split kernel; the shapes with tails, long rows and every
epilogue run on the device (tests/test_split_gpu.py)."""
import pytest

from tests import split_cases as SC


def test_emu_split_gemm_nt_ragged_rows(emu, gemm_options):
    """gemm_nt256w_kernel<float, .., true>: 549 rows = two 256-row tiles and 37 rows, K = 64 = two stages (shorter than the prologue)."""
    gemm_options(gemm_min_m=512)
    SC.case_nt(emu, 549, 256, 64, epis=("none + bias", "residual"))


def test_emu_split_gemm_tn(emu, gemm_options):
    """gemm_tn256_kernel<float, true>: one 256 x 256 tile over 144 tokens = 9 slices."""
    gemm_options(gemm_variant=4)
    SC.case_tn(emu, 144, 256, 256, splits=(0,))


@pytest.mark.parametrize("BN", [(1, 64), (2, 70)])
def test_emu_split_attention_forward(emu, BN):
    """attn_fwd_x3s_kernel and attn_fwd_kernel<float, true>: one full key tile (the unmasked path), and 70 = one tile and six keys."""
    SC.case_attn_fwd(emu, *BN)


def test_emu_split_attention_backward(emu):
    SC.case_attn_bwd(emu, 2, 70)
