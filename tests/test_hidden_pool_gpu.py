"""GPU (`-m gpu`): the grid pools of the hidden states (MAEST_GATHER_POOLS, csrc/misc.hip gather_pools_kernel) on the device, in both
libraries, through the cases of tests/hidden_pool_cases.py: every shape, the 10 s and 30 s token counts included -- equality with the
ascending fp32 loop, the bound, rows 0 .. 2 against maest_embed_pool --, repeat launches, the refusals and the guard."""
import pytest

from maest_amd import _lib
from tests import guard
from tests import hidden_pool_cases as HP

pytestmark = pytest.mark.gpu
DEV = "cuda"
COVERED = set()     # entry points this module runs under the guard (guard.covering)
SHAPES = HP.SHAPES + HP.SHAPES_GPU


def _both_libraries(fn):
    fn()
    with _lib.flavour("f16"):
        fn()


@pytest.mark.parametrize("clips,Fk,Tk", SHAPES)
def test_hidden_pool_exact(clips, Fk, Tk):
    _both_libraries(lambda: HP.case_exact(DEV, clips, Fk, Tk))


@pytest.mark.parametrize("clips,Fk,Tk", SHAPES)
def test_hidden_pool_repeat(clips, Fk, Tk):
    _both_libraries(lambda: HP.case_repeat(DEV, clips, Fk, Tk))


def test_hidden_pool_argument_errors():
    _both_libraries(lambda: HP.case_argument_errors(DEV))


@pytest.mark.parametrize("clips,Fk,Tk", SHAPES)
@guard.covering(COVERED, "maest_gather_head_rows", limit=120)
def test_hidden_pool_guarded(clips, Fk, Tk):
    """Inside guarded arenas: dst is written in exactly [clips, 3 + Fk + Tk, 768], src is untouched, nothing outside is written."""
    _both_libraries(lambda: HP.case_regions(DEV, clips, Fk, Tk))
