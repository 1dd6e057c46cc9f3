"""CPU (`-m "not gpu"`): token counts per clip in the attention forward (MAEST_ATTN_LENS, csrc/attention.hip: the LENS instantiations of
attn_fwd_kernel, attn_fwd_dma_kernel and attn_fwd_x3s_kernel) under the SIMT lockstep emulator, in the bf16 and in the half build, through
the cases of tests/attn_lens_cases.py.  The emulator takes seconds per launch: the shapes are the smallest that cross a 64-key tile, a
32-query wave and a clip of one token; the 128- and 256-query workgroup boundaries and N > 320 run on the device
(tests/test_attn_lens_gpu.py)."""
import pytest

from maest_amd import _lib
from tests import attn_lens_cases as LC
from tests import guard
from tests.test_emu_f16_kernels import emu16  # noqa: F401  (the two-build emulator fixture)

COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_builds(form, fn):
    """fn() in the bf16 build and, for the forms whose operands are 16-bit, in the half build as well."""
    fn()
    if form in ("16", "qs"):      # (the register-staged 16-bit form in the half build: the device)
        with _lib.flavour("f16"):
            fn()


@pytest.mark.parametrize("form", LC.FORMS_EMU)
def test_emu_attn_lens(emu16, form):
    """Complete passes: full counts, every clip against the clip alone and against fp64, NaN padding, written rows, two calls."""
    B, N, counts = LC.EMU_SHAPES[0]
    _both_builds(form, lambda: LC.case_lens(emu16, form, B, N, counts, full_B=1))


@pytest.mark.parametrize("form", ["f32", "x3", "16", "16r", "qs"])
@guard.covering(COVERED, "maest_attn_fwd_rows")
def test_emu_attn_lens_head_rows_guarded(emu16, form):
    """q_rows = 2 inside guarded arenas: rows >= 32 keep the pre-fill pattern, a clip of one token has one real query."""
    B, N, counts = LC.EMU_SHAPES[0]
    _both_builds(form, lambda: LC.case_lens(emu16, form, B, N, counts, q_rows=2, full_B=1))


@pytest.mark.parametrize("form", ["x3", "16"])
@guard.covering(COVERED, "maest_attn_fwd_rows")
def test_emu_attn_lens_short_guarded(emu16, form):
    """N = 40: one key tile, a clip of three tokens beside a full one, complete passes under the guard."""
    B, N, counts = LC.EMU_SHAPES[1]
    LC.case_lens(emu16, form, B, N, counts)


def test_emu_attn_lens_argument_errors(emu16):
    LC.case_argument_errors(emu16)
    with _lib.flavour("f16"):
        LC.case_argument_errors(emu16)
