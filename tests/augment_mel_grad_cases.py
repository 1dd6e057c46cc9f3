"""Shared by tests/test_emu_augment_mel_bwd.py (CPU, host emulator) and tests/test_augment_mel_grad_gpu.py: the yardstick of the
AugmentMelSTFT backward (maest_augment_mel_bwd, csrc/mel2.hip).

The gradient is compared with float64 torch autograd of a restatement of the front end (the steps of oracle.maest_oracle.augment_mel,
which casts its constants to fp32 and so cannot run in float64) that uses THE MODULE'S OWN fp32 constants upcast: the 800 window values,
the kaldi bank padded by one zero bin, the pre-emphasis buffer -- a reference with other constants measures the constants, not the kernel.

The function is badly conditioned in fp32 (low kaldi bands hold one or two pre-emphasised low-frequency bins whose power sits near
log_eps, and 1 / (acc + 1e-5) amplifies the FFT's absolute error there), so the gate is calibrated per case by torch's own fp32 autograd
of the same restatement (the reference arithmetic, never the code under test):

    e_max(a) = max|a - want64| / max|want64|        e_l2(a) = ||a - want64|| / ||want64||
    gate_x   = max(1e-4, 4 * e_x(ref32))            assert e_x(kernel) <= gate_x for x in {max, l2}
    condition: e_x(ref32) <= 5e-4                   (no gate above 2e-3; a case that breaks it is a badly chosen input and fails)

Margin 4: the sibling log-mel backward kernel measures at most 1.5 times torch's fp32 error on its inputs; 4 leaves a factor 2.7 for the
different FFT factorisation.  A real defect (a dropped frame, a wrong fold, a missing pre-emphasis tap, doubled mirror bins) shows as 1e-2
or more."""
import torch
import torch.nn.functional as F

from maest_amd.preprocess import kaldi_mel_banks

FLOOR, MARGIN, CONDITION = 1e-4, 4.0, 5e-4


def restate(wave, aug, fmin, fmax, f_stripe=None, t_stripe=None):
    """The front end in wave's dtype from `aug`'s constants; stripes = (start, width) zeroed after the log."""
    dt = wave.dtype
    left = (aug.n_fft - aug.win_length) // 2
    win = aug.window.detach().cpu()[left:left + aug.win_length].to(dt)
    y = F.conv1d(wave.unsqueeze(1), aug.preemphasis_coefficient.detach().cpu().to(dt)).squeeze(1)
    spec = torch.stft(y, aug.n_fft, hop_length=aug.hopsize, win_length=aug.win_length, center=True, normalized=False, window=win,
                      return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2
    fb = torch.from_numpy(kaldi_mel_banks(aug.n_mels, aug.n_fft, aug.sr, fmin, fmax)).to(dt)
    mel = (torch.matmul(F.pad(fb, (0, 1)), power) + 0.00001).log()
    keep = torch.ones(mel.shape[1:], dtype=dt)
    if f_stripe is not None:
        keep[f_stripe[0]:f_stripe[0] + f_stripe[1], :] = 0.0
    if t_stripe is not None:
        keep[:, t_stripe[0]:t_stripe[0] + t_stripe[1]] = 0.0
    return (mel * keep + 4.5) / 5.0


def reference_grads(wave, g, aug, fmin, fmax, **stripes):
    """(want64, ref32): autograd of the restatement in float64 and in fp32, upstream gradient g."""
    out = []
    for dt in (torch.float64, torch.float32):
        w = wave.detach().cpu().to(dt).requires_grad_()
        restate(w, aug, fmin, fmax, **stripes).backward(g.detach().cpu().to(dt))
        out.append(w.grad)
    return out


def errors(a, want64):
    d = a.detach().cpu().double() - want64
    return float(d.abs().max() / want64.abs().max()), float(d.norm() / want64.norm())


def check(got, wave, g, aug, what, fmin=None, fmax=None, **stripes):
    """Print the kernel's and the fp32 reference's errors and the gates, then assert the condition and the gates."""
    want64, ref32 = reference_grads(wave, g, aug, aug.fmin if fmin is None else fmin, aug.fmax if fmax is None else fmax, **stripes)
    assert got.shape == want64.shape
    e_k, e_r = errors(got, want64), errors(ref32, want64)
    gates = tuple(max(FLOOR, MARGIN * e) for e in e_r)
    print(f"{what}: kernel max {e_k[0]:.2e} l2 {e_k[1]:.2e} | ref32 max {e_r[0]:.2e} l2 {e_r[1]:.2e} | gate max {gates[0]:.2e} "
          f"l2 {gates[1]:.2e}")
    assert bool(torch.isfinite(got).all()), what
    assert e_r[0] <= CONDITION and e_r[1] <= CONDITION, (what, "the fp32 reference itself is outside the condition: a badly chosen input", e_r)
    assert e_k[0] <= gates[0] and e_k[1] <= gates[1], (what, e_k, gates)


def module_grad(aug, wave, g, dev="cpu"):
    """wave.grad through the module (a recorded forward, then backward of g); also returns the recorded output."""
    w = wave.to(dev).clone().requires_grad_()
    out = aug(w)
    out.backward(g.to(dev))
    return w.grad, out.detach()
