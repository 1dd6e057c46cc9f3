"""GPU (`-m gpu`): the attention-map kernel (MAEST_ATTN_PROBS, csrc/attention.hip attn_probs_kernel) on the device, in both libraries, through
the cases of tests/attn_probs_cases.py: every shape in every operand code against the derived bound, the mean form bit for bit, repeat
calls, the cross-check with the forward, the refusals and both forms under the guard."""
import pytest
import torch

from maest_amd import _lib
from tests import attn_probs_cases as PC
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


@pytest.mark.parametrize("code", PC.CODES)
@pytest.mark.parametrize("B,N,q_rows", PC.SHAPES + [PC.SHAPE_GPU])
def test_attn_probs(B, N, q_rows, code):
    """The per-head form inside the derived bound, rows summing to 1; the mean form bit-identical to the ascending-head fp32 sum."""
    _both_libraries(code, lambda: PC.case_probs(DEV, B, N, q_rows, code))


@pytest.mark.parametrize("code", PC.CODES)
def test_attn_probs_spike(code):
    _both_libraries(code, lambda: PC.case_probs(DEV, 2, 161, 161, code, spike=True))


@pytest.mark.parametrize("code", PC.CODES)
def test_attn_probs_operands_times_three(code):
    _both_libraries(code, lambda: PC.case_probs(DEV, 2, 161, 161, code, times=3.0))


@pytest.mark.parametrize("code", PC.CODES)
def test_attn_probs_repeat(code):
    _both_libraries(code, lambda: PC.case_repeat(DEV, 2, 161, 161, code))


@pytest.mark.parametrize("B,N", [(2, 70), (2, 161)])
def test_attn_probs_against_the_forward(B, N):
    PC.case_forward_consistency(DEV, B, N)


def test_attn_probs_argument_errors():
    PC.case_argument_errors(DEV)
    with _lib.flavour("f16"):
        PC.case_argument_errors(DEV)


@pytest.mark.parametrize("B,N,q_rows", [(2, 70, 70), (2, 161, 2)])
@guard.covering(COVERED, "maest_attn_fwd_rows", limit=120)
def test_attn_probs_guarded(B, N, q_rows):
    """Both forms inside guarded arenas: `out` has exactly q_rows rows per head, so a kernel that writes the padded rows of its last query block,
    or the padding keys of its last tile, lands in a band."""
    for code in PC.CODES:
        _both_libraries(code, lambda: PC.case_probs(DEV, B, N, q_rows, code))
