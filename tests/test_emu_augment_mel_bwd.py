"""CPU (`-m "not gpu"`): the backward of the AugmentMelSTFT front end (maest_augment_mel_bwd, csrc/mel2.hip) runs from the SAME sources
under the host SIMT emulator (tests/emu), against float64 torch autograd of a restatement of the front end with the module's own
constants; the gate of each case is calibrated by torch's fp32 autograd of the same restatement (tests/augment_mel_grad_cases.py)."""
import numpy as np
import pytest
import torch

from maest_amd.preprocess import AugmentMelSTFT
from tests import augment_mel_grad_cases as C
from tests.kernel_cases import rnd


def _frames(S):
    return 1 + (S - 1) // 320


def _eval_case(wave, seed, what, n_mels=128):
    aug = AugmentMelSTFT(n_mels=n_mels).eval()
    g = rnd((wave.shape[0], n_mels, _frames(wave.shape[1])), seed)
    got, _ = C.module_grad(aug, wave, g)
    C.check(got, wave, g, aug, what)
    return aug, g, got


@pytest.mark.parametrize("B, S, what", [
    (1, 700, "S = 700: T = 3, both folds reach the same samples"),
    (1, 3200, "S = 3200: a multiple of the hop"),
    (2, 4001, "B = 2, odd S: clip 1 starts misaligned"),
    (1, 32 * 320 + 77, "T = 33: two blocks, the right fold in the second"),
    (2, 96 * 320 + 101, "T = 97: interior blocks"),
])
def test_emu_augment_mel_bwd_matches_autograd(emu, B, S, what):
    _eval_case(rnd((B, S), 100 + S, 0.3), 200 + S, what)


def test_emu_augment_mel_bwd_dc_and_nyquist(emu):
    """Energy in bins 0 and 512, which have no mirror partner in the inverse transform."""
    S = 4000
    n = torch.arange(S, dtype=torch.float32)
    dc = 0.4 + 0.01 * rnd((S,), 11)
    nyq = 0.5 * torch.cos(np.pi * n) + 0.01 * rnd((S,), 12)
    _eval_case(torch.stack([dc, nyq]), 13, "DC offset and Nyquist tone")


def _train_module():
    return AugmentMelSTFT(fmin_aug_range=10, fmax_aug_range=2000, timem=20).train()      # 29 frames: the time stripe stays in the clip


def _replay_draws(aug, T):
    """The module's draws of one training call, from the seed the caller has just set: fmin, fmax, frequency stripe, time stripe."""
    fmin = aug.fmin + torch.randint(aug.fmin_aug_range, (1,)).item()
    fmax = aug.fmax + aug.fmax_aug_range // 2 - torch.randint(aug.fmax_aug_range, (1,)).item()
    v = torch.rand(1) * aug.freqm
    mv = torch.rand(1) * (aug.n_mels - v)
    fs = (int(mv.long()), int(v.long()))
    v = torch.rand(1) * aug.timem
    mv = torch.rand(1) * (T - v)
    ts = (int(mv.long()), int(v.long()))
    return fmin, fmax, fs, ts


def test_emu_augment_mel_bwd_training_mode(emu):
    """Band-edge jitter and both stripes replayed from the seed: zero inside the stripes, 1 / 5 of the upstream gradient elsewhere; the
    recorded forward is the plain training forward bit for bit; a gradient fed ONLY inside the stripes gives dwave == 0 exactly."""
    aug = _train_module()
    wave = rnd((2, 9000), 5, 0.3)
    T = _frames(9000)
    g = rnd((2, 128, T), 6)
    torch.manual_seed(7)
    got, out = C.module_grad(aug, wave, g)
    torch.manual_seed(7)
    fmin, fmax, fs, ts = _replay_draws(aug, T)
    assert (fmin, fmax, fs) == (5.0, 14108, (63, 31)) and 0 <= ts[0] and ts[0] + ts[1] <= T and ts[1] > 0
    torch.manual_seed(7)
    with torch.no_grad():
        plain = aug(wave)
    assert torch.equal(out, plain)
    assert bool((plain[:, fs[0]:fs[0] + fs[1], :] == 0.9).all()) and bool((plain[:, :, ts[0]:ts[0] + ts[1]] == 0.9).all())
    C.check(got, wave, g, aug, "training mode", fmin=fmin, fmax=fmax, f_stripe=fs, t_stripe=ts)
    inside = torch.zeros_like(g)
    inside[:, fs[0]:fs[0] + fs[1], :] = g[:, fs[0]:fs[0] + fs[1], :]
    inside[:, :, ts[0]:ts[0] + ts[1]] = g[:, :, ts[0]:ts[0] + ts[1]]
    torch.manual_seed(7)
    got0, _ = C.module_grad(aug, wave, inside)
    assert bool((got0 == 0).all()), "a gradient inside the masked stripes reached the waveform"


def test_emu_augment_mel_bwd_deterministic(emu):
    aug = AugmentMelSTFT().eval()
    wave = rnd((2, 5001), 21, 0.3)
    g = rnd((2, 128, _frames(5001)), 22)
    a, _ = C.module_grad(aug, wave, g)
    b, _ = C.module_grad(aug, wave, g)
    assert torch.equal(a, b)


def test_emu_augment_mel_module_waveform_grad(emu):
    """Through the module, one clip: the output requires grad and is the no-grad forward bit for bit; the caller's gradient is left as it was."""
    aug = AugmentMelSTFT().eval()
    wave = rnd((1, 2900), 31, 0.3)
    with torch.no_grad():
        plain = aug(wave)
    w = wave.clone().requires_grad_()
    out = aug(w)
    assert out.requires_grad and out.grad_fn is not None and torch.equal(out.detach(), plain)
    g = rnd(tuple(out.shape), 32)
    g0 = g.clone()
    out.backward(g)
    assert w.grad is not None and w.grad.shape == wave.shape and w.grad.dtype == torch.float32
    assert torch.equal(g, g0)
    C.check(w.grad, wave, g, aug, "AugmentMelSTFT, 1 clip")


def test_emu_augment_mel_fp16_waveform_gets_an_fp16_gradient(emu):
    aug = AugmentMelSTFT().eval()
    wave = rnd((1, 2900), 41, 0.3).half()
    g = rnd((1, 128, _frames(2900)), 42)
    g16, _ = C.module_grad(aug, wave, g)
    assert g16 is not None and g16.dtype == torch.float16 and g16.shape == wave.shape
    g32, _ = C.module_grad(aug, wave.float(), g)
    assert torch.equal(g16, g32.half())


@pytest.mark.parametrize("training", [False, True])
def test_emu_augment_mel_plain_call_records_nothing(emu, training):
    """Grad mode on but a waveform that does not require grad: today's path, no graph."""
    aug = _train_module() if training else AugmentMelSTFT().eval()
    wave = rnd((2, 9000), 51, 0.3)
    torch.manual_seed(3)
    out = aug(wave)
    assert not out.requires_grad and out.grad_fn is None
    torch.manual_seed(3)
    with torch.no_grad():
        assert torch.equal(aug(wave), out)
