"""CPU (`-m "not gpu"`): weighted attention pooling (MAEST_ATTN_APPLY, csrc/attention.hip attn_apply_stats_kernel + attn_apply_kernel) under the
SIMT lockstep emulator, in the bf16 and in the half build, through the cases of tests/attn_apply_cases.py -- and, without any kernel, what
that module's gate passes and refuses.  The emulator takes seconds per launch: a subset of the (shape, code) matrix runs here, all of it on the
device (tests/test_attn_apply_gpu.py)."""
import pytest
import torch

from maest_amd import _lib
from tests import attn_apply_cases as AC
from tests import attn_probs_cases as PC
from tests import guard
from tests.test_emu_f16_kernels import emu16  # noqa: F401  (the two-build emulator fixture)

COVERED = set()     # entry points this module runs under the guard (guard.covering)


def _both_builds(code, fn):
    """fn() in the bf16 build and, for the codes whose operands are 16-bit, in the half build as well."""
    fn()
    if code in ("16", "qs"):
        with _lib.flavour("f16"):
            fn()


# every shape once in fp32 and once in a 16-bit code, every code at the ragged shape
@pytest.mark.parametrize("B,N,q_rows,R,code", [(2, 64, 64, 2, "f32"), (2, 64, 64, 2, "qs"),
                                               (2, 70, 70, 2, "f32"), (2, 70, 70, 2, "x3"), (2, 70, 70, 2, "16"), (2, 70, 70, 2, "qs"),
                                               (2, 161, 161, 3, "x3"), (2, 161, 161, 3, "16"),
                                               (2, 161, 2, 2, "f32"), (2, 161, 2, 2, "16"),
                                               (2, 161, 40, 1, "x3"), (2, 161, 40, 1, "qs")])
def test_emu_attn_apply(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: AC.case_apply(emu16, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", ["f32", "16"])
def test_emu_attn_apply_spike(emu16, code):
    """One probability of 1.000 in a row whose others lie below 2^-126 (flushed by v_exp_f32: the 2^-100 floor)."""
    _both_builds(code, lambda: AC.case_apply(emu16, 2, 161, 161, 3, code, spike=True))


@pytest.mark.parametrize("code", ["x3", "qs"])
def test_emu_attn_apply_operands_times_three(emu16, code):
    """Exponents over +-40."""
    _both_builds(code, lambda: AC.case_apply(emu16, 2, 161, 161, 3, code, times=3.0))


@pytest.mark.parametrize("code", ["f32", "16"])
def test_emu_attn_apply_onehot_against_the_maps(emu16, code):
    AC.case_onehot(emu16, 2, 70, code)


@pytest.mark.parametrize("B,N,q_rows,R,code", [(2, 161, 2, 2, "x3"), (2, 161, 40, 1, "16")])
def test_emu_attn_apply_nan_columns(emu16, B, N, q_rows, R, code):
    AC.case_nan_columns(emu16, B, N, q_rows, R, code)


@pytest.mark.parametrize("code", ["x3", "16"])
def test_emu_attn_apply_repeat(emu16, code):
    AC.case_repeat(emu16, 2, 70, 70, 2, code)


def test_emu_attn_apply_argument_errors(emu16):
    AC.case_argument_errors(emu16)
    with _lib.flavour("f16"):
        AC.case_argument_errors(emu16)


def test_emu_attn_apply_leaves_the_backward_alone(emu16):
    AC.case_backward_unchanged(emu16)


@guard.covering(COVERED, "maest_attn_bwd_rows")
def test_emu_attn_apply_guarded(emu16):
    """Inside guarded arenas: Y has exactly [B, R, N] elements, W is const, the workspace is written in rows < q_rows only."""
    AC.case_regions(emu16, 2, 161, 40, 1, "16")
    AC.case_apply(emu16, 2, 70, 70, 2, "f32")


# ---------------------------------------------------------------------------------------------- the gate itself (no kernel)
def _gated(defect, B=1, N=70, q_rows=70, R=2, code="f32"):
    _, xs = PC.operands(B, N, code)
    y = AC.pipeline64(xs, AC.weights(B, R, N, q_rows), B, N, q_rows, PC.c2_of(code), defect)
    return AC.gate(f"fp64 pipeline, defect {defect!r}", y, AC.reference_of(B, N, q_rows, R, code))


@pytest.mark.parametrize("B,N,q_rows,R", [(1, 70, 70, 2), (2, 161, 40, 1), (2, 161, 2, 2)])
def test_attn_apply_gate_passes_the_sound_pipeline(B, N, q_rows, R):
    """The condition that must hold before any kernel result is believed."""
    ratio, rratio = _gated(None, B, N, q_rows, R)
    assert ratio < 1e-6 and rratio < 1e-6


@pytest.mark.parametrize("defect", AC.DEFECTS)
def test_attn_apply_gate_rejects_defects(defect):
    q_rows = 40 if defect == "all queries" else 70        # (a defect that needs queries past q_rows to exist)
    with pytest.raises(AssertionError, match="outside the bound|a row sums to"):
        _gated(defect, q_rows=q_rows)


def test_attn_apply_weights_are_what_the_cases_say():
    w = AC.weights(2, 3, 161, 161)
    assert bool((w >= 0).all()) and 0 < int((w == 0).sum()) < w.numel() // 4
    assert bool(torch.isnan(AC.weights(2, 3, 161, 40, nan_tail=True)[:, :, 40:]).all()) and not bool(torch.isnan(w).any())
