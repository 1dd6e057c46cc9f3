"""CPU (`-m "not gpu"`): the per-clip form of the patch-embedding operand load (MAEST_IM2COL_CLIP_TOKENS, csrc/embed.hip
patch_im2col_clips_kernel) and ops.token_assemble_clips under the SIMT lockstep emulator, in the bf16 and in the half build, through the
cases of tests/im2col_clips_cases.py; tests/test_im2col_clips_gpu.py runs the same cases on the device."""
import pytest
import torch

from maest_amd import _lib
from tests import guard
from tests import im2col_clips_cases as IC
from tests.test_emu_f16_kernels import emu16  # noqa: F401  (the two-build emulator fixture)

COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_builds(fn):
    fn()
    with _lib.flavour("f16"):
        fn()


@pytest.mark.parametrize("stride", IC.STRIDES)
@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
@pytest.mark.parametrize("x_dtype", IC.X_DTYPES)
@pytest.mark.parametrize("B,P", IC.SHAPES)
def test_emu_im2col_clips_equal_the_shared_form(emu16, B, P, x_dtype, out_dtype, stride):
    _both_builds(lambda: IC.case_equal(emu16, B, P, x_dtype, out_dtype, stride))


@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
def test_emu_im2col_clips_with_mixup_and_stripes(emu16, out_dtype):
    _both_builds(lambda: IC.case_equal(emu16, 3, 7, torch.float16, out_dtype, (8, 12), mix=True, masked=True))


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
def test_emu_im2col_clips_blank_rows_are_zero_bits_over_nan(emu16, out_dtype, mix):
    _both_builds(lambda: IC.case_blank(emu16, out_dtype, torch.float32, mix))
    IC.case_blank(emu16, out_dtype, torch.float16, mix)


@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
def test_emu_im2col_clips_broadcast_table_equals_the_unflagged_call(emu16, out_dtype):
    _both_builds(lambda: IC.case_broadcast(emu16, 3, 7, out_dtype, (10, 10)))
    IC.case_broadcast(emu16, 1, 1, out_dtype, (8, 12))


def test_emu_im2col_clips_argument_errors(emu16):
    _both_builds(lambda: IC.case_argument_errors(emu16))


@pytest.mark.parametrize("B,P", IC.SHAPES)
def test_emu_token_assemble_clips(emu16, B, P):
    _both_builds(lambda: IC.case_token_assemble_clips(emu16, B, P))


@guard.covering(COVERED, "maest_patch_im2col_strided", "maest_token_assemble")
def test_emu_im2col_clips_guarded(emu16):
    """Inside guarded arenas: out is written in exactly [B * P, 256], the inputs are untouched, nothing outside is written."""
    _both_builds(lambda: IC.case_regions(emu16, 3, 7, torch.bfloat16))
    IC.case_regions(emu16, 3, 7, torch.float32)
    IC.case_regions(emu16, 1, 1, torch.float32)
