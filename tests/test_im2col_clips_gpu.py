"""GPU (`-m gpu`): the per-clip form of the patch-embedding operand load (MAEST_IM2COL_CLIP_TOKENS, csrc/embed.hip
patch_im2col_clips_kernel) and ops.token_assemble_clips on the device, in both libraries, through the cases of
tests/im2col_clips_cases.py -- and the one size only the device holds: output offsets past 2^31 elements."""
import pytest
import torch

from maest_amd import _lib
from tests import guard
from tests import im2col_clips_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda"
COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_libraries(fn):
    fn()
    with _lib.flavour("f16"):
        fn()


@pytest.mark.parametrize("stride", IC.STRIDES)
@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
@pytest.mark.parametrize("x_dtype", IC.X_DTYPES)
@pytest.mark.parametrize("B,P", IC.SHAPES)
def test_im2col_clips_equal_the_shared_form(B, P, x_dtype, out_dtype, stride):
    _both_libraries(lambda: IC.case_equal(DEV, B, P, x_dtype, out_dtype, stride))


@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
def test_im2col_clips_with_mixup_and_stripes(out_dtype):
    _both_libraries(lambda: IC.case_equal(DEV, 3, 7, torch.float16, out_dtype, (8, 12), mix=True, masked=True))


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
def test_im2col_clips_blank_rows_are_zero_bits_over_nan(out_dtype, mix):
    _both_libraries(lambda: IC.case_blank(DEV, out_dtype, torch.float32, mix))
    IC.case_blank(DEV, out_dtype, torch.float16, mix)


@pytest.mark.parametrize("out_dtype", IC.OUT_DTYPES)
def test_im2col_clips_broadcast_table_equals_the_unflagged_call(out_dtype):
    _both_libraries(lambda: IC.case_broadcast(DEV, 3, 7, out_dtype, (10, 10)))
    IC.case_broadcast(DEV, 1, 1, out_dtype, (8, 12))


def test_im2col_clips_argument_errors():
    _both_libraries(lambda: IC.case_argument_errors(DEV))


@pytest.mark.parametrize("B,P", IC.SHAPES)
def test_token_assemble_clips(B, P):
    _both_libraries(lambda: IC.case_token_assemble_clips(DEV, B, P))


@guard.covering(COVERED, "maest_patch_im2col_strided", "maest_token_assemble", limit=120)
def test_im2col_clips_guarded():
    """Inside guarded arenas: out is written in exactly [B * P, 256], the inputs are untouched, nothing outside is written."""
    _both_libraries(lambda: IC.case_regions(DEV, 3, 7, torch.bfloat16))
    IC.case_regions(DEV, 3, 7, torch.float32)
    IC.case_regions(DEV, 2, 225, torch.float32)


def test_im2col_clips_offsets_past_2_to_31():
    IC.case_big(DEV)
