"""GPU (`-m gpu`): token counts per clip in the attention forward (MAEST_ATTN_LENS, csrc/attention.hip: the LENS instantiations of
attn_fwd_kernel, attn_fwd_dma_kernel and attn_fwd_x3s_kernel) on the device, in both libraries, through the cases of
tests/attn_lens_cases.py.  Shapes: B = 12, N = 161 with a count on either side of every 32-query wave, 64-key tile and 128-query workgroup
boundary; B = 5, N = 330 with whole-workgroup early exits and N > 320, where the unflagged 16-bit dispatch takes the persistent kernel and
the flagged one must not."""
import pytest

from maest_amd import _lib
from tests import attn_lens_cases as LC
from tests import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_libraries(form, fn):
    """fn() in libmaest_hip.so and, for the forms whose operands are 16-bit, in libmaest_hip_f16.so as well."""
    fn()
    if form in LC.FORMS_16:
        with _lib.flavour("f16"):
            fn()


@pytest.mark.parametrize("form", list(LC.FORMS))
@pytest.mark.parametrize("B,N,counts", LC.GPU_SHAPES)
def test_attn_lens(B, N, counts, form):
    """Complete passes: full counts, every clip against the clip alone and against fp64, NaN padding, written rows, two calls."""
    _both_libraries(form, lambda: LC.case_lens(DEV, form, B, N, counts))


@pytest.mark.parametrize("form", ["f32", "x3", "16", "16r", "qs"])
@pytest.mark.parametrize("B,N,counts", LC.GPU_SHAPES)
@guard.covering(COVERED, "maest_attn_fwd_rows", limit=120)
def test_attn_lens_head_rows_guarded(B, N, counts, form):
    """q_rows = 2 inside guarded arenas: rows >= 32 keep the pre-fill pattern, a clip of one token has one real query."""
    _both_libraries(form, lambda: LC.case_lens(DEV, form, B, N, counts, q_rows=2))


@pytest.mark.parametrize("B,N,counts", LC.GPU_SHAPES)
@guard.covering(COVERED, "maest_attn_fwd_rows", limit=120)
def test_attn_lens_guarded(B, N, counts):
    """Complete passes of every form inside guarded arenas."""
    for form in LC.FORMS:
        _both_libraries(form, lambda: LC.case_lens(DEV, form, B, N, counts))


def test_attn_lens_argument_errors():
    LC.case_argument_errors(DEV)
    with _lib.flavour("f16"):
        LC.case_argument_errors(DEV)
