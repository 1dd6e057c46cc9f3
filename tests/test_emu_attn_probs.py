"""CPU (`-m "not gpu"`): the attention-map kernel (MAEST_ATTN_PROBS, csrc/attention.hip attn_probs_kernel) under the SIMT lockstep emulator,
in the bf16 and in the half build, through the cases of tests/attn_probs_cases.py -- and, without any kernel, what that module's gate refuses.
The emulator takes seconds per launch: the mean form, the repeat and the guard run at a subset of the shapes here and at every shape on the
device (tests/test_attn_probs_gpu.py)."""
import pytest
import torch

from maest_amd import _lib
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


@pytest.mark.parametrize("code", PC.CODES)
@pytest.mark.parametrize("B,N,q_rows", PC.SHAPES)
def test_emu_attn_probs(emu16, B, N, q_rows, code):
    _both_builds(code, lambda: PC.case_probs(emu16, B, N, q_rows, code, mean=False))


@pytest.mark.parametrize("code", ["f32", "x3", "16"])
def test_emu_attn_probs_spike(emu16, code):
    """One probability of 1.000 in a row whose others lie below 2^-126 (flushed by v_exp_f32: the 2^-100 floor), and a late maximum that
    moves the running statistics of pass 1 by hundreds of binades."""
    _both_builds(code, lambda: PC.case_probs(emu16, 2, 161, 161, code, mean=False, spike=True))


@pytest.mark.parametrize("code", ["x3", "16", "qs"])
def test_emu_attn_probs_operands_times_three(emu16, code):
    """Exponents over +-40."""
    _both_builds(code, lambda: PC.case_probs(emu16, 2, 161, 161, code, mean=False, times=3.0))


@pytest.mark.parametrize("B,N,q_rows,code", [(2, 70, 70, "f32"), (2, 70, 70, "x3"), (2, 70, 70, "16"), (2, 70, 70, "qs"), (2, 161, 40, "16"),
                                             (2, 161, 161, "qs")])
def test_emu_attn_probs_mean_form(emu16, B, N, q_rows, code):
    """Bit-identical to the ascending-head fp32 sum of the per-head output times fp32(1 / 12)."""
    _both_builds(code, lambda: PC.case_mean(emu16, B, N, q_rows, code))


@pytest.mark.parametrize("code", ["x3", "16"])
def test_emu_attn_probs_repeat(emu16, code):
    PC.case_repeat(emu16, 2, 70, 70, code)


def test_emu_attn_probs_against_the_forward(emu16):
    PC.case_forward_consistency(emu16, 2, 70)


def test_emu_attn_probs_argument_errors(emu16):
    PC.case_argument_errors(emu16)
    with _lib.flavour("f16"):
        PC.case_argument_errors(emu16)


@pytest.mark.parametrize("B,N,q_rows", [(2, 70, 70), (2, 161, 2)])
@guard.covering(COVERED, "maest_attn_fwd_rows")
def test_emu_attn_probs_guarded(emu16, B, N, q_rows):
    """Both forms inside guarded arenas: `out` has exactly q_rows rows per head, so a kernel that writes the padded rows of its last query block,
    or the padding keys of its last tile, lands in a band."""
    for code in ("x3", "16"):
        PC.case_probs(emu16, B, N, q_rows, code)


# ---------------------------------------------------------------------------------------------- the gate itself (no kernel)
def _gated(defect, B=1, N=70, code="f32"):
    _, xs = PC.operands(B, N, code)
    p = PC.pipeline64(xs, B, N, N, PC.c2_of(code), defect)
    return PC.gate(f"fp64 pipeline, defect {defect!r}", p, *PC.reference_of(B, N, N, code), N)


def test_attn_probs_gate_passes_the_sound_pipeline():
    ratio, dsum = _gated(None)
    assert ratio < 1e-6 and dsum < 1e-12


@pytest.mark.parametrize("defect", ["scale", "padding", "bf16 sum", "bf16 c2"])
def test_attn_probs_gate_rejects_defects(defect):
    with pytest.raises(AssertionError, match="outside the bound|a row sums to"):
        _gated(defect)


def test_attn_probs_reference_has_the_spike():
    """The spike case is what its docstring says: a largest probability of 1.000 and smallest ones below 2^-126."""
    p_ref, _ = PC.reference_of(2, 161, 161, "f32", spike=True)
    row = p_ref[0, 0, 3]
    assert int(row.argmax()) == 5 and float(row.max()) > 0.9999 and float(row.min()) < 2.0 ** -126
