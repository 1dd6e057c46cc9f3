"""CPU (`-m "not gpu"`): gradient-weighted attention pooling (MAEST_ATTN_APPLY | MAEST_ATTN_APPLY_GRAD, csrc/attention.hip attn_apply_stats_kernel
+ attn_apply_kernel<.., GRAD>) under the SIMT lockstep emulator, in the bf16 and in the half build, through the cases of
tests/attn_relevance_cases.py -- and, without any kernel, what that module's gate passes and refuses.  The emulator takes seconds per launch:
a subset of the (shape, code) matrix runs here, all of it on the device (tests/test_attn_relevance_gpu.py)."""
import pytest

from maest_amd import _lib
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


# every shape once in an fp32 code and once in a 16-bit code, every code at the ragged shape
@pytest.mark.parametrize("B,N,q_rows,R,code", [(2, 64, 64, 2, "f32"), (2, 64, 64, 2, "qs"),
                                               (2, 70, 70, 2, "f32"), (2, 70, 70, 2, "x3"), (2, 70, 70, 2, "16"), (2, 70, 70, 2, "qs"),
                                               (2, 161, 161, 3, "x3"), (2, 161, 161, 3, "16"),
                                               (2, 161, 2, 2, "f32"), (2, 161, 2, 2, "16"),
                                               (2, 161, 40, 1, "x3"), (2, 161, 40, 1, "qs")])
def test_emu_attn_relevance(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: RC.case_relevance(emu16, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", ["f32", "16"])
def test_emu_attn_relevance_spike(emu16, code):
    """One probability of 1.000 in a row whose others lie below 2^-126 (flushed by v_exp_f32: the 2^-100 floor)."""
    _both_builds(code, lambda: RC.case_relevance(emu16, 2, 161, 161, 3, code, spike=True))


@pytest.mark.parametrize("code", ["x3", "qs"])
def test_emu_attn_relevance_operands_times_three(emu16, code):
    """Exponents over +-40, values (and so dP) three times as large."""
    _both_builds(code, lambda: RC.case_relevance(emu16, 2, 161, 161, 3, code, times=3.0))


@pytest.mark.parametrize("B,N,q_rows,R,code", [(2, 70, 70, 2, "x3"), (2, 161, 40, 1, "16")])
def test_emu_attn_relevance_zero_gradient(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: RC.case_zero(emu16, B, N, q_rows, R, code))


@pytest.mark.parametrize("B,N,q_rows,R,code", [(2, 161, 2, 2, "x3"), (2, 161, 40, 1, "16")])
def test_emu_attn_relevance_nan_rows(emu16, B, N, q_rows, R, code):
    _both_builds(code, lambda: RC.case_nan_rows(emu16, B, N, q_rows, R, code))


@pytest.mark.parametrize("code", ["x3", "16"])
def test_emu_attn_relevance_repeat(emu16, code):
    RC.case_repeat(emu16, 2, 70, 70, 2, code)


def test_emu_attn_relevance_argument_errors(emu16):
    RC.case_argument_errors(emu16)
    with _lib.flavour("f16"):
        RC.case_argument_errors(emu16)


def test_emu_attn_relevance_leaves_its_neighbours_alone(emu16):
    RC.case_neighbours_unchanged(emu16)


@guard.covering(COVERED, "maest_attn_bwd_rows")
def test_emu_attn_relevance_guarded(emu16):
    """Inside guarded arenas: Y has exactly [B, R, N] elements written, dO and W are const, the workspace is written in rows < q_rows only."""
    RC.case_regions(emu16, 2, 161, 40, 1, "16")
    RC.case_relevance(emu16, 2, 70, 70, 2, "f32")


# ---------------------------------------------------------------------------------------------- the gate itself (no kernel)
def _gated(defect, B=1, N=70, q_rows=70, R=2, code="f32"):
    _, xs = PC.operands(B, N, code)
    _, ds = RC.dout(B, N, q_rows, code)
    y = RC.pipeline64(xs, ds, RC.weights(B, R, N, q_rows), B, N, q_rows, PC.c2_of(code), defect)
    return RC.gate(f"fp64 pipeline, defect {defect!r}", y, RC.reference_of(B, N, q_rows, R, code))


@pytest.mark.parametrize("B,N,q_rows,R", [(1, 70, 70, 2), (2, 161, 40, 1), (2, 161, 2, 2)])
def test_attn_relevance_gate_passes_the_sound_pipeline(B, N, q_rows, R):
    """The condition that must hold before any kernel result is believed."""
    assert _gated(None, B, N, q_rows, R) < 1e-6


@pytest.mark.parametrize("defect", RC.DEFECTS)
def test_attn_relevance_gate_rejects_defects(defect):
    q_rows = 40 if defect == "all queries" else 70        # (a defect that needs queries past q_rows to exist)
    with pytest.raises(AssertionError, match="outside the bound"):
        _gated(defect, q_rows=q_rows)


def test_attn_relevance_operands_are_what_the_cases_say():
    d, ds = RC.dout(2, 161, 40, "16")
    assert d.shape == (2 * 161, 768) and ds.dtype.is_floating_point and float(ds.abs().max()) > 1
    assert not bool(RC.dout(2, 161, 40, "16", variant="zero")[0].float().any())
    dn = RC.dout(2, 161, 40, "f32", variant="nan")[0].reshape(2, 161, 768)
    assert bool(dn[:, 40:].isnan().all()) and not bool(dn[:, :40].isnan().any())
