"""GPU (`-m gpu`): per-head attention pooling (MAEST_ATTN_APPLY_HEADS, csrc/attention.hip attn_apply_stats_kernel +
attn_apply_kernel<.., HEADS>) on the device, in both libraries, through the cases of tests/attn_heads_cases.py: every shape in every operand
code, plain and gradient-weighted -- the identity with the mean form bit for bit, every head against the derived bound --, repeat calls,
NaN in the unread rows and columns, the refusals and the guard."""
import pytest

from maest_amd import _lib
from tests import attn_heads_cases as HC
from tests import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
COVERED = set()     # entry points this module runs under the guard (guard.covering)
FORMS = [pytest.param(False, id="plain"), pytest.param(True, id="grad")]


def _both_libraries(code, fn):
    """fn() in libmaest_hip.so and, for the codes whose operands are 16-bit, in libmaest_hip_f16.so as well."""
    fn()
    if code in ("16", "qs"):
        with _lib.flavour("f16"):
            fn()


@pytest.mark.parametrize("grad", FORMS)
@pytest.mark.parametrize("code", HC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", HC.SHAPES + [HC.SHAPE_GPU])
def test_attn_heads_identity(B, N, q_rows, R, code, grad):
    _both_libraries(code, lambda: HC.case_identity(DEV, B, N, q_rows, R, code, grad))


@pytest.mark.parametrize("grad", FORMS)
@pytest.mark.parametrize("code", HC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", HC.SHAPES + [HC.SHAPE_GPU])
def test_attn_heads_bound(B, N, q_rows, R, code, grad):
    _both_libraries(code, lambda: HC.case_bound(DEV, B, N, q_rows, R, code, grad))


@pytest.mark.parametrize("grad", FORMS)
@pytest.mark.parametrize("code", HC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", HC.SHAPES + [HC.SHAPE_GPU])
def test_attn_heads_repeat(B, N, q_rows, R, code, grad):
    _both_libraries(code, lambda: HC.case_repeat(DEV, B, N, q_rows, R, code, grad))


@pytest.mark.parametrize("grad", FORMS)
@pytest.mark.parametrize("code", HC.CODES)
@pytest.mark.parametrize("B,N,q_rows,R", [s for s in HC.SHAPES if s[2] < s[1]])      # (every shape that has a tail)
def test_attn_heads_tails(B, N, q_rows, R, code, grad):
    _both_libraries(code, lambda: HC.case_tails(DEV, B, N, q_rows, R, code, grad))


def test_attn_heads_argument_errors():
    HC.case_argument_errors(DEV)
    with _lib.flavour("f16"):
        HC.case_argument_errors(DEV)


@pytest.mark.parametrize("grad", FORMS)
@pytest.mark.parametrize("B,N,q_rows,R", HC.SHAPES + [HC.SHAPE_GPU])
@guard.covering(COVERED, "maest_attn_bwd_rows", limit=120)
def test_attn_heads_guarded(B, N, q_rows, R, grad):
    """Inside guarded arenas: Y has exactly [B, 12, R, N] elements written -- a store for a key >= N or into a thirteenth head would land in
    a band --, dO and W are const, the workspace is written in rows < q_rows only."""
    for code in HC.CODES:
        _both_libraries(code, lambda: HC.case_regions(DEV, B, N, q_rows, R, code, grad))
