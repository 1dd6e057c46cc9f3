"""CPU (`-m "not gpu"`): per-head attention pooling (MAEST_ATTN_APPLY_HEADS, csrc/attention.hip attn_apply_stats_kernel +
attn_apply_kernel<.., HEADS>) under the SIMT lockstep emulator, in the bf16 and in the half build, through the cases of
tests/attn_heads_cases.py -- and, without any kernel, what that module's two conditions pass and refuse.  The emulator takes seconds per
launch: the plain form runs the identity and the bound at every shape, the rest a subset; all of it runs on the device
(tests/test_attn_heads_gpu.py)."""
import pytest

from maest_amd import _lib
from tests import attn_heads_cases as HC
from tests import attn_probs_cases as PC
from tests import attn_relevance_cases as RC
from tests import guard
from tests.test_emu_f16_kernels import emu16  # noqa: F401  (the two-build emulator fixture)

COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_builds(code, fn):
    """fn() in the bf16 build and, for the codes whose operands are 16-bit, in the half build as well."""
    fn()
    if code in ("16", "qs"):
        with _lib.flavour("f16"):
            fn()


# the plain form: every shape once in an fp32 code and once in a 16-bit code, every code at the ragged shape
PLAIN = [(2, 64, 64, 2, "f32"), (2, 64, 64, 2, "qs"),
         (2, 70, 70, 2, "f32"), (2, 70, 70, 2, "x3"), (2, 70, 70, 2, "16"), (2, 70, 70, 2, "qs"),
         (2, 161, 161, 3, "x3"), (2, 161, 161, 3, "16"),
         (2, 161, 2, 2, "f32"), (2, 161, 2, 2, "16"),
         (2, 161, 40, 1, "x3"), (2, 161, 40, 1, "qs")]
# the gradient-weighted form: the ragged shape in every arithmetic, two key blocks with a partial query tile, the head-token rows
GRAD = [(2, 70, 70, 2, "f32"), (2, 70, 70, 2, "x3"), (2, 70, 70, 2, "qs"), (2, 161, 40, 1, "16"), (2, 161, 2, 2, "x3")]


@pytest.mark.parametrize("B,N,q_rows,R,code", PLAIN)
def test_emu_attn_heads_identity(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: HC.case_identity(emu16, B, N, q_rows, R, code, False))


@pytest.mark.parametrize("B,N,q_rows,R,code", PLAIN)
def test_emu_attn_heads_bound(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: HC.case_bound(emu16, B, N, q_rows, R, code, False))


@pytest.mark.parametrize("B,N,q_rows,R,code", GRAD)
def test_emu_attn_heads_grad_identity(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: HC.case_identity(emu16, B, N, q_rows, R, code, True))


@pytest.mark.parametrize("B,N,q_rows,R,code", GRAD)
def test_emu_attn_heads_grad_bound(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: HC.case_bound(emu16, B, N, q_rows, R, code, True))


@pytest.mark.parametrize("grad,code", [(False, "x3"), (True, "16")])
def test_emu_attn_heads_repeat(emu16, grad, code):
    HC.case_repeat(emu16, 2, 70, 70, 2, code, grad)


@pytest.mark.parametrize("B,N,q_rows,R,code,grad", [(2, 161, 2, 2, "x3", False), (2, 161, 40, 1, "16", True)])
def test_emu_attn_heads_tails(emu16, B, N, q_rows, R, code, grad):
    _both_builds(code, lambda: HC.case_tails(emu16, B, N, q_rows, R, code, grad))


def test_emu_attn_heads_argument_errors(emu16):
    HC.case_argument_errors(emu16)
    with _lib.flavour("f16"):
        HC.case_argument_errors(emu16)


@guard.covering(COVERED, "maest_attn_bwd_rows")
def test_emu_attn_heads_guarded(emu16):
    """Inside guarded arenas: Y has exactly [B, 12, R, N] elements written, dO and W are const, the workspace is written in rows < q_rows
    only."""
    HC.case_regions(emu16, 2, 161, 40, 1, "16", True)
    HC.case_regions(emu16, 2, 70, 70, 2, "f32", False)


# ---------------------------------------------------------------------------------------------- the two conditions themselves (no kernel)
def _doctored(defect, grad, B=1, N=70, q_rows=70, R=2, code="f32"):
    _, xs = PC.operands(B, N, code)
    ds = RC.dout(B, N, q_rows, code)[1] if grad else None
    return HC.pipeline64(xs, ds, HC.weights(B, R, N, q_rows), B, N, q_rows, PC.c2_of(code), defect)


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("B,N,q_rows,R", [(1, 70, 70, 2), (2, 161, 40, 1), (2, 161, 2, 2)])
def test_attn_heads_gates_pass_the_sound_pipeline(B, N, q_rows, R, grad):
    """The conditions that must hold before any kernel result is believed: the fp64 pipeline, rounded to fp32 once, uses next to nothing of
    the bound (its one rounding: u of a limit of many u), and its ascending mean satisfies the identity."""
    y, mean = _doctored(None, grad, B, N, q_rows, R)
    assert HC.gate("fp64 pipeline", y, HC.reference_of(B, N, q_rows, R, "f32", grad)) < 0.5
    HC.identity("fp64 pipeline", y, mean)


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("defect", HC.DEFECTS)
def test_attn_heads_gates_reject_defects(defect, grad):
    y, mean = _doctored(defect, grad)
    if defect == "descending head sum":      # every head is where and what it should be: only the identity can see the order of the sum
        HC.gate(f"fp64 pipeline, defect {defect!r}", y, HC.reference_of(1, 70, 70, 2, "f32", grad))
        with pytest.raises(AssertionError, match="elements differ"):
            HC.identity(f"fp64 pipeline, defect {defect!r}", y, mean)
    else:
        with pytest.raises(AssertionError, match="outside the bound"):
            HC.gate(f"fp64 pipeline, defect {defect!r}", y, HC.reference_of(1, 70, 70, 2, "f32", grad))
