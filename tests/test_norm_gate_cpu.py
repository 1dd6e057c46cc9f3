"""CPU, no kernel involved: the gates of tests/norm_cases.py can fail.  An fp32 restatement of the LayerNorm, head and
loss arithmetic in the kernels' summation order passes every gate; each defect of it is rejected on a family that the test names; and the four
eps / variance defects PASS the 1e-5 gate of kernel_cases.case_layernorm on the plain family -- the blindness section 7c closes, kept as a fact."""
import pytest
import torch
import torch.nn.functional as F

from tests import kernel_cases as KC
from tests import norm_cases as NC

ROWS = 16          # per family


def _rows_of(family, x, fam):
    m = fam == NC.FAMILIES.index(family)
    return x[m], fam[m]


def _fwd_gates(x, fam, g, b, eps, defect=None, eps_given=None):
    """The restated forward through every forward gate: fp32 y, bf16 y, split rows, mean, rstd."""
    y, mean, rstd = NC.restate_fwd(x, g, b, eps if eps_given is None else eps_given, defect)
    ref = NC.fwd_ref(x, g, b, eps, fam)
    worst = NC.check_fwd(y, mean, rstd, x, g, b, eps, fam, "restated forward", ref)
    NC.check_fwd(KC.lp(y), None, None, x, g, b, eps, fam, "restated forward, 16-bit y", ref)
    hi = KC.lp(y)
    NC.check_fwd(torch.cat([hi, hi, KC.lp(y - KC.f32(hi))], 1), None, None, x, g, b, eps, fam, "restated forward, split rows", ref)
    return worst


def test_the_restatement_passes_every_forward_gate():
    x, fam, g, b = NC.inputs(ROWS)
    worst = {}
    for eps in NC.EPS:
        for k, r in _fwd_gates(x, fam, g, b, eps).items():
            worst[k] = max(worst.get(k, 0.0), r)
    NC.show("restated forward", worst)


def _bwd_inputs(eps):
    x, fam, g, b = NC.inputs(ROWS)
    _, mean, rstd = NC.restate_fwd(x, g, b, eps)
    return x, fam, g, mean, rstd, KC.rnd(tuple(x.shape), 730), KC.rnd(tuple(x.shape), 731)


def test_the_restatement_passes_every_backward_gate():
    worst = {}
    for eps in NC.EPS:
        x, fam, g, mean, rstd, dy, dres = _bwd_inputs(eps)
        for dr in (None, dres):
            dx = NC.restate_bwd(dy, x, g, mean, rstd, dr)
            for k, r in NC.check_bwd(dx, KC.lp(dx), None, None, dy, x, g, mean, rstd, dr, fam, "restated backward").items():
                worst[k] = max(worst.get(k, 0.0), r)
        d16 = KC.lp(dy)             # a 16-bit dy: the reference reads the rounded values
        dx = NC.restate_bwd(KC.f32(d16), x, g, mean, rstd)
        NC.check_bwd(dx, KC.lp(dx), None, None, d16, x, g, mean, rstd, None, fam, "restated backward, 16-bit dy")
    NC.show("restated backward", worst)


@pytest.mark.parametrize("shape", NC.LOSS_SHAPES)
def test_the_restatement_passes_the_loss_gates(shape):
    z, y, perm, lam = NC.loss_inputs(*shape)
    worst = {}
    for p, l in ((None, None), (perm, lam)):
        for weight in (1.0, 0.5):
            for training in (True, False):
                loss, dz = NC.restate_loss(z, y, p, l, weight, training)
                for k, r in NC.check_loss(loss, dz, z, y, p, l, weight, f"restated loss {shape} mixed={p is not None} training={training}").items():
                    worst[k] = max(worst.get(k, 0.0), r)
    print(f"restated loss {shape}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# defect -> the family (rows of the one tensor, or logits) on which the gates must reject it
REJECTED_ON = {
    "one-pass variance": "offset",
    "variance without the mean": "offset",
    "divisor 767": "plain",
    "eps dropped": "near-constant",
    "eps outside the root": "near-constant",
    "the other eps": "near-constant",
    "no s1": "huge",
    "s2 off by 1e-3": "huge",
}


@pytest.mark.parametrize("defect", NC.FWD_DEFECTS)
@pytest.mark.parametrize("eps", NC.EPS)
def test_a_forward_defect_is_rejected(defect, eps):
    x, fam, g, b = NC.inputs(ROWS)
    xs, fs = _rows_of(REJECTED_ON[defect], x, fam)
    _fwd_gates(xs, fs, g, b, eps)                                    # the honest restatement passes on these rows ...
    with pytest.raises(AssertionError, match=REJECTED_ON[defect]):   # ... the defect does not, and the failure names the family
        _fwd_gates(xs, fs, g, b, eps, defect)


@pytest.mark.parametrize("defect", NC.BWD_DEFECTS)
def test_a_backward_defect_is_rejected(defect):
    x, fam, g, mean, rstd, dy, _ = _bwd_inputs(1e-6)
    m = fam == NC.FAMILIES.index(REJECTED_ON[defect])
    args = (dy[m], x[m], g, mean[m], rstd[m])
    NC.check_bwd(NC.restate_bwd(*args), None, None, None, *args, None, fam[m], "restated backward")
    with pytest.raises(AssertionError, match=REJECTED_ON[defect]):
        NC.check_bwd(NC.restate_bwd(*args, defect=defect), None, None, None, *args, None, fam[m], "restated backward")


def test_backward_without_s1_passes_the_old_gate_on_huge_rows():
    """kernel_cases.case_layernorm's 1e-4 relative + 1e-5 absolute is blind to scale: dx of rows of magnitude 1e4 is about 1e-4."""
    x, fam, g, mean, rstd, dy, _ = _bwd_inputs(1e-6)
    m = fam == NC.FAMILIES.index("huge")
    xr = x[m].clone().requires_grad_(True)
    F.layer_norm(xr, (768,), g, None, 1e-6).backward(dy[m])
    KC.close(NC.restate_bwd(dy[m], x[m], g, mean[m], rstd[m], defect="no s1"), xr.grad, 1e-4, 1e-5, "dx without s1 under the old gate")


@pytest.mark.parametrize("training", [True, False])
def test_a_loss_without_the_absolute_value_is_rejected_on_the_logits_below_minus_88(training):
    z, y, perm, lam = NC.loss_inputs(*NC.LOSS_SHAPES[1])
    loss, dz = NC.restate_loss(z, y, None, None, 1.0, training, defect="no abs in log1p(exp(-|z|))")
    with pytest.raises(AssertionError, match="the loss is inf"):
        NC.check_loss(loss, dz, z, y, None, None, 1.0, "loss without |z|")
    # ... and where nothing overflows (|z| <= 20) the value is off by |z| at every negative logit: outside the bound
    zm = z.clamp(-20, 20)
    loss, dz = NC.restate_loss(zm, y, None, None, 1.0, training, defect="no abs in log1p(exp(-|z|))")
    with pytest.raises(AssertionError, match="outside"):
        NC.check_loss(loss, dz, zm, y, None, None, 1.0, "loss without |z|, moderate logits")


@pytest.mark.parametrize("training", [True, False])
def test_unmixed_targets_are_rejected(training):
    z, y, perm, lam = NC.loss_inputs(*NC.LOSS_SHAPES[1])
    loss, dz = NC.restate_loss(z, y, perm, lam, 1.0, training, defect="unmixed targets")
    with pytest.raises(AssertionError, match="loss|dlogits"):
        NC.check_loss(loss, dz, z, y, perm, lam, 1.0, "unmixed targets")
    if training:        # the loss aside, dlogits alone rejects it
        good, _ = NC.restate_loss(z, y, perm, lam, 1.0, True)
        with pytest.raises(AssertionError, match="dlogits"):
            NC.check_loss(good, dz, z, y, perm, lam, 1.0, "unmixed targets")


def _old_gate(y, mean, rstd, x, g, b, eps):
    """What kernel_cases.case_layernorm asserts of a forward."""
    KC.close(y, F.layer_norm(x, (768,), g, b, eps), 1e-5, 1e-5, "layernorm fwd")
    KC.close(mean, x.mean(1), 1e-5, 1e-6, "layernorm mean")
    KC.close(rstd, 1.0 / torch.sqrt(x.var(1, unbiased=False) + eps), 1e-5, 1e-6, "layernorm rstd")


@pytest.mark.parametrize("defect", NC.OLD_GATE_BLIND)
def test_control_the_old_gate_is_blind_on_the_plain_family(defect):
    """The suite's one family, 2 N + 0.3 at eps = 1e-6 (kernel_cases.case_layernorm), under its 1e-5 + 1e-5 |ref| gate: these four defects pass."""
    x, fam, g, b = NC.inputs(ROWS)
    xs, _ = _rows_of("plain", x, fam)
    _old_gate(*NC.restate_fwd(xs, g, b, 1e-6, defect), xs, g, b, 1e-6)


def test_control_the_old_gate_rejects_the_honest_restatement_on_offset_rows():
    """... and it cannot simply be kept for the other families: rows of mean 300, std 0.5 fail it with nothing wrong."""
    x, fam, g, b = NC.inputs(ROWS)
    xs, _ = _rows_of("offset", x, fam)
    with pytest.raises(AssertionError):
        _old_gate(*NC.restate_fwd(xs, g, b, 1e-6), xs, g, b, 1e-6)
