"""GPU (`-m gpu`): weighted attention pooling (MAEST_ATTN_APPLY, csrc/attention.hip attn_apply_stats_kernel + attn_apply_kernel) on the device,
in both libraries, through the cases of tests/attn_apply_cases.py: every shape in every operand code against the derived bound, the spike and
the scaled operands, one-hot weights against the head-mean maps, NaN in the unread weight columns, repeat calls, the refusals and the guard."""
import pytest

from maest_amd import _lib
from tests import attn_apply_cases as AC
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


@pytest.mark.parametrize("code", AC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", AC.SHAPES + [AC.SHAPE_GPU])
def test_attn_apply(B, N, q_rows, R, code):
    _both_libraries(code, lambda: AC.case_apply(DEV, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", AC.CODES)
def test_attn_apply_spike(code):
    _both_libraries(code, lambda: AC.case_apply(DEV, 2, 161, 161, 3, code, spike=True))


@pytest.mark.parametrize("code", AC.CODES)
def test_attn_apply_operands_times_three(code):
    _both_libraries(code, lambda: AC.case_apply(DEV, 2, 161, 161, 3, code, times=3.0))


@pytest.mark.parametrize("code", AC.CODES)
def test_attn_apply_onehot_against_the_maps(code):
    _both_libraries(code, lambda: AC.case_onehot(DEV, 2, 161, code))


@pytest.mark.parametrize("code", AC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", [(2, 161, 2, 2), (2, 161, 40, 1)])
def test_attn_apply_nan_columns(B, N, q_rows, R, code):
    _both_libraries(code, lambda: AC.case_nan_columns(DEV, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", AC.CODES)
def test_attn_apply_repeat(code):
    _both_libraries(code, lambda: AC.case_repeat(DEV, 2, 161, 161, 3, code))


def test_attn_apply_argument_errors():
    AC.case_argument_errors(DEV)
    with _lib.flavour("f16"):
        AC.case_argument_errors(DEV)


def test_attn_apply_leaves_the_backward_alone():
    AC.case_backward_unchanged(DEV)


@pytest.mark.parametrize("B,N,q_rows,R", [(2, 70, 70, 2), (2, 161, 40, 1), (2, 161, 2, 2)])
@guard.covering(COVERED, "maest_attn_bwd_rows", limit=120)
def test_attn_apply_guarded(B, N, q_rows, R):
    """Inside guarded arenas: Y has exactly [B, R, N] elements, W is const, the workspace is written in rows < q_rows only."""
    for code in AC.CODES:
        _both_libraries(code, lambda: AC.case_regions(DEV, B, N, q_rows, R, code))
        _both_libraries(code, lambda: AC.case_apply(DEV, B, N, q_rows, R, code))
