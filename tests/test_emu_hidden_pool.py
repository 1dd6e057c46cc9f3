"""CPU (`-m "not gpu"`): the grid pools of the hidden states (MAEST_GATHER_POOLS, csrc/misc.hip gather_pools_kernel) under the SIMT
lockstep emulator, in the bf16 and in the half build, through the cases of tests/hidden_pool_cases.py up to the model test's N = 227 -- and,
without any kernel, what that module's two conditions pass and refuse.  The two long shapes run on the device
(tests/test_hidden_pool_gpu.py)."""
import pytest

from maest_amd import _lib
from tests import guard
from tests import hidden_pool_cases as HP
from tests.test_emu_f16_kernels import emu16  # noqa: F401  (the two-build emulator fixture)

COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_builds(fn):
    fn()
    with _lib.flavour("f16"):
        fn()


@pytest.mark.parametrize("clips,Fk,Tk", HP.SHAPES)
def test_emu_hidden_pool_exact(emu16, clips, Fk, Tk):
    _both_builds(lambda: HP.case_exact(emu16, clips, Fk, Tk))


def test_emu_hidden_pool_repeat(emu16):
    _both_builds(lambda: HP.case_repeat(emu16, 3, 4, 13))


def test_emu_hidden_pool_argument_errors(emu16):
    _both_builds(lambda: HP.case_argument_errors(emu16))


@guard.covering(COVERED, "maest_gather_head_rows")
def test_emu_hidden_pool_guarded(emu16):
    """Inside guarded arenas: dst is written in exactly [clips, 3 + Fk + Tk, 768], src is untouched, nothing outside is written."""
    _both_builds(lambda: HP.case_regions(emu16, 3, 4, 13))
    HP.case_regions(emu16, 1, 1, 1)
    HP.case_regions(emu16, 2, 1, 7)


# ---------------------------------------------------------------------------------------------- the two conditions themselves (no kernel)
@pytest.mark.parametrize("clips,Fk,Tk", HP.SHAPES + HP.SHAPES_GPU)
def test_hidden_pool_conditions_pass_the_sound_pipeline(clips, Fk, Tk):
    """The definition evaluated independently (every operation in fp64, rounded to fp32) has the bits of the ascending fp32 loop and lies
    inside the bound; building the operand asserts the condition on the inputs for every shape, the device's two included."""
    ref, lims = HP.reference_of(clips, Fk, Tk)
    got = HP.pipeline(HP.operand(clips, Fk, Tk), Fk, Tk)
    HP.equal("fp64 pipeline", got, ref)
    assert HP.gate("fp64 pipeline", got, lims) <= 1.0


@pytest.mark.parametrize("defect", HP.DEFECTS)
def test_hidden_pool_conditions_reject_defects(defect):
    clips, Fk, Tk = 2, 9, 25
    ref, lims = HP.reference_of(clips, Fk, Tk)
    got = HP.pipeline(HP.operand(clips, Fk, Tk), Fk, Tk, defect)
    if defect == "descending order":      # every row is where and what it should be: only equality can see the order of a sum
        HP.gate(f"fp64 pipeline, defect {defect!r}", got, lims)
        with pytest.raises(AssertionError, match="elements differ"):
            HP.equal(f"fp64 pipeline, defect {defect!r}", got, ref)
    else:
        with pytest.raises(AssertionError, match="outside the bound"):
            HP.gate(f"fp64 pipeline, defect {defect!r}", got, lims)
