"""GPU (`-m gpu`): gradients through the AugmentMelSTFT front end to the waveform (maest_augment_mel_bwd, csrc/mel2.hip): the kernel
against float64 autograd of a restatement of the front end, each gate calibrated by torch's fp32 autograd of the same restatement
(tests/augment_mel_grad_cases.py), and end to end through a PaSST-shaped model."""
import pytest
import torch

from maest_amd import get_maest
from maest_amd.preprocess import AugmentMelSTFT
from oracle import maest_oracle as O
from tests import augment_mel_grad_cases as C
from tests.kernel_cases import rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = "passt_s_swa_p16_128_ap476"
S_E2E = 200001                 # 96 bands x 626 frames: the model's input
S10 = 320077                   # 10 s at 32 kHz with a ragged tail: 1001 frames


def _frames(S):
    return 1 + (S - 1) // 320


def test_augment_mel_bwd_96_bands_matches_float64_autograd():
    aug = AugmentMelSTFT(n_mels=96).eval()
    wave = rnd((2, S_E2E), 62, 0.3)
    g = rnd((2, 96, _frames(S_E2E)), 63)
    got, _ = C.module_grad(aug, wave, g, DEV)
    C.check(got, wave, g, aug, "n_mels = 96, S = 200001")


def test_augment_mel_bwd_10s_batch_matches_float64_autograd_and_repeats_bit_equal():
    aug = AugmentMelSTFT().eval()
    wave = rnd((3, S10), 1, 0.3)
    g = rnd((3, 128, _frames(S10)), 2)
    got, out = C.module_grad(aug, wave, g, DEV)
    with torch.no_grad():
        assert torch.equal(out, aug(wave.to(DEV)))
    C.check(got, wave, g, aug, "10 s batch, S = 320077")
    again, _ = C.module_grad(aug, wave, g, DEV)
    assert torch.equal(got, again), "wave.grad differs between two identical backward passes"


def test_waveform_gradient_through_the_front_end_and_the_model():
    """wave -> AugmentMelSTFT(96 bands) -> model -> sum(logits * w).  Expected: the model's mel-input gradient G (that path is pinned to the
    oracle by tests/test_grad_paths_gpu.py) pushed through the float64 restatement of the front end.  A frozen model gives the same
    wave.grad and no parameter gradient."""
    aug = AugmentMelSTFT(n_mels=96).eval()
    net = get_maest(ARCH, pretrained=False, input_t=625, precision="fp32")
    net.load_state_dict(O.make_state_dict(625, seed=61))
    net = net.to(DEV).eval()
    wave = rnd((2, S_E2E), 62, 0.3)
    w = rnd((2, 400), 63).to(DEV)

    def wave_grad():
        wd = wave.to(DEV).requires_grad_()
        logits = net(aug(wd).unsqueeze(1))[0]
        (logits * w).sum().backward()
        assert wd.grad is not None and wd.grad.shape == wave.shape and wd.grad.dtype == torch.float32
        return wd.grad

    got = wave_grad()
    with torch.no_grad():
        mel = aug(wave.to(DEV))
    mel = mel.requires_grad_()
    (net(mel.unsqueeze(1))[0] * w).sum().backward()
    G = mel.grad.detach().cpu()
    assert G.shape == (2, 96, _frames(S_E2E))
    C.check(got, wave, G, aug, "end to end, G from the model")
    net.requires_grad_(False)
    net.zero_grad(set_to_none=True)
    frozen = wave_grad()
    same = float((frozen - got).abs().max() / got.abs().max())
    print(f"frozen model: max|d wave.grad| / max|wave.grad| = {same:.2e}")
    assert same < 1e-6         # (the bound of tests/test_waveform_grad_gpu.py for the same statement about the log-mel front end)
    assert all(p.grad is None for p in net.parameters())
