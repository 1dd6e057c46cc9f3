"""GPU (`-m gpu`): gradient-weighted attention pooling (MAEST_ATTN_APPLY | MAEST_ATTN_APPLY_GRAD, csrc/attention.hip attn_apply_stats_kernel +
attn_apply_kernel<.., GRAD>) on the device, in both libraries, through the cases of tests/attn_relevance_cases.py: every shape in every
operand code against the derived bound, the spike and the scaled operands, a zero gradient, NaN in the unread rows and columns, repeat
calls, the refusals, the neighbouring forms and the guard."""
import pytest

from maest_amd import _lib
from tests import attn_relevance_cases as RC
from tests import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_libraries(code, fn):
    """fn() in libmaest_hip.so and, for the codes whose operands are 16-bit, in libmaest_hip_f16.so as well."""
    fn()
    if code in ("16", "qs"):
        with _lib.flavour("f16"):
            fn()


@pytest.mark.parametrize("code", RC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", RC.SHAPES + [RC.SHAPE_GPU])
def test_attn_relevance(B, N, q_rows, R, code):
    _both_libraries(code, lambda: RC.case_relevance(DEV, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", RC.CODES)
def test_attn_relevance_spike(code):
    _both_libraries(code, lambda: RC.case_relevance(DEV, 2, 161, 161, 3, code, spike=True))


@pytest.mark.parametrize("code", RC.CODES)
def test_attn_relevance_operands_times_three(code):
    _both_libraries(code, lambda: RC.case_relevance(DEV, 2, 161, 161, 3, code, times=3.0))


@pytest.mark.parametrize("code", RC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", [(2, 70, 70, 2), (2, 161, 40, 1), (1, 353, 353, 8)])
def test_attn_relevance_zero_gradient(B, N, q_rows, R, code):
    _both_libraries(code, lambda: RC.case_zero(DEV, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", RC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", [(2, 161, 2, 2), (2, 161, 40, 1)])
def test_attn_relevance_nan_rows(B, N, q_rows, R, code):
    _both_libraries(code, lambda: RC.case_nan_rows(DEV, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", RC.CODES)
def test_attn_relevance_repeat(code):
    _both_libraries(code, lambda: RC.case_repeat(DEV, 2, 161, 161, 3, code))


def test_attn_relevance_argument_errors():
    RC.case_argument_errors(DEV)
    with _lib.flavour("f16"):
        RC.case_argument_errors(DEV)


def test_attn_relevance_leaves_its_neighbours_alone():
    RC.case_neighbours_unchanged(DEV)


@pytest.mark.parametrize("B,N,q_rows,R", [(2, 70, 70, 2), (2, 161, 40, 1), (2, 161, 2, 2)])
@guard.covering(COVERED, "maest_attn_bwd_rows", limit=120)
def test_attn_relevance_guarded(B, N, q_rows, R):
    """Inside guarded arenas: Y has exactly [B, R, N] elements written, dO and W are const, the workspace is written in rows < q_rows only."""
    for code in RC.CODES:
        _both_libraries(code, lambda: RC.case_regions(DEV, B, N, q_rows, R, code))
        _both_libraries(code, lambda: RC.case_relevance(DEV, B, N, q_rows, R, code))
