"""CPU (`-m "not gpu"`): the backward of the log-mel front end (maest_logmel_bwd, csrc/mel.hip) runs from the SAME sources under the host
SIMT emulator (tests/emu), against float64 torch autograd of the oracle's log-mel (O.logmel's steps: torch.stft power spectrum, the
slaney bank, log10(1 + 1e4 mel), z-norm) with a random upstream gradient."""
import numpy as np
import pytest
import torch

from maest_amd import ops
from maest_amd.melspectrogram import MelConstants, MelSpectrogram
from oracle import maest_oracle as O
from tests.kernel_cases import rnd

GATE = 1e-4


def _logmel64(w):
    """O.logmel in float64 (O.logmel itself casts to float32 first)."""
    spec = O.power_spectrogram(w)
    fb = torch.from_numpy(O.mel_filterbank()).to(w.dtype)
    mel = torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)
    return (torch.log10(1 + mel * 10000) - O.NORM_MEAN) / (O.NORM_STD * 2)


def _want(wave, g):
    w = wave.double().requires_grad_()
    _logmel64(w).backward(g.double())
    return w.grad


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def _consts():
    m = MelSpectrogram()
    return MelConstants("cpu", m.sr, m.win_len, m.n_mel, m.norm_mean, m.norm_std)


def _check(wave, seed, what):
    B, S = wave.shape
    g = rnd((B, 96, 1 + S // 256), seed)
    got = ops.logmel_bwd(wave.contiguous(), g, _consts())
    err = _rel(got, _want(wave, g))
    print(f"{what}: max|got - want| / max|want| = {err:.2e}")
    assert err <= GATE, (what, err)
    return got, g


@pytest.mark.parametrize("B, S, what", [
    (1, 300, "S = 300: T = 2, both reflect folds reach the same samples"),
    (1, 2560, "S = 2560: a multiple of 256"),
    (2, 4001, "B = 2, odd S: the second clip starts misaligned"),
    (1, 64 * 256 + 77, "T = 65: two blocks, the right fold in the second"),
    (2, 192 * 256 + 101, "T = 193, odd S: clip 0's middle block takes the interior fetch, clip 1 (misaligned) never does"),
])
def test_emu_logmel_bwd_matches_autograd(emu, B, S, what):
    _check(rnd((B, S), 100 + S, 0.3), 200 + S, what)


def test_emu_logmel_bwd_dc_and_nyquist(emu):
    """Energy in bins 0 and 256, which have no mirror partner in the inverse transform."""
    S = 2000
    n = torch.arange(S, dtype=torch.float32)
    dc = 0.4 + 0.01 * rnd((S,), 11)
    nyq = 0.5 * torch.cos(np.pi * n) + 0.01 * rnd((S,), 12)
    _check(torch.stack([dc, nyq]), 13, "DC offset and Nyquist tone")


def test_emu_logmel_bwd_deterministic(emu):
    wave = rnd((2, 3001), 21, 0.3)
    g = rnd((2, 96, 1 + 3001 // 256), 22)
    c = _consts()
    a = ops.logmel_bwd(wave, g, c)
    b = ops.logmel_bwd(wave, g, c)
    assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2900,), (2, 2900)])
def test_emu_melspectrogram_waveform_grad(emu, shape):
    """Through the module: a waveform that requires grad gets its gradient, and the forward output is the no-grad one bit for bit."""
    mel = MelSpectrogram()
    wave = rnd(shape, 31, 0.3)
    with torch.no_grad():
        plain = mel(wave)
    w = wave.clone().requires_grad_()
    out = mel(w)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    g = rnd(tuple(out.shape), 32)
    out.backward(g)
    assert w.grad is not None and w.grad.shape == wave.shape
    want = _want(wave.reshape(-1, shape[-1]), g.reshape(-1, 96, out.shape[-1])).reshape(shape)
    err = _rel(w.grad, want)
    print(f"MelSpectrogram {shape}: {err:.2e}")
    assert err <= GATE, err


def test_emu_melspectrogram_plain_call_records_nothing(emu):
    """Grad mode on but a waveform that does not require grad: today's path, no graph."""
    mel = MelSpectrogram()
    wave = rnd((2, 2900), 41, 0.3)
    out = mel(wave)
    assert not out.requires_grad and out.grad_fn is None
    with torch.no_grad():
        assert torch.equal(mel(wave), out)
