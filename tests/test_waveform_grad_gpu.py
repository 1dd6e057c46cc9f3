"""GPU (`-m gpu`): gradients through the log-mel front end to the waveform (saliency on raw audio, a loss behind a waveform generator):
the whole model against the oracle's CPU autograd (O.logmel -> O.forward), and maest_logmel_bwd itself against float64 autograd."""

import numpy as np
import pytest
import torch

from maest_amd import get_maest, ops
from oracle import maest_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = "passt_s_swa_p16_128_ap476"
S10 = 160000                  # 10 s at 16 kHz: 626 frames


def randn(shape, seed, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def rel_err(a, b):
    a = a.detach().float().cpu()
    b = torch.as_tensor(b).detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def make(sd, precision="fp32", **kw):
    net = get_maest(ARCH, pretrained=False, input_t=625, precision=precision, **kw)
    net.load_state_dict(sd)
    return net.to(DEV)


def oracle_params(sd):
    return {k: v.clone().requires_grad_(True) for k, v in sd.items()}


def oracle_wave_grad(wave, sd, w=None, y=None, **tk):
    """wave.grad of the oracle on the CPU for a 2-D batch: O.logmel -> O.forward; loss sum(logits * w) or mean BCE against y."""
    wo = wave.clone().requires_grad_(True)
    logits = O.forward(O.logmel(wo).unsqueeze(1), oracle_params(sd), (96, 625), **tk)[0]
    loss = (logits * w).sum() if y is None else torch.nn.functional.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    return wo.grad


def test_logmel_bwd_kernel_matches_float64_autograd():
    """The kernel alone at a 10 s batch with a ragged tail clip length: against float64 torch autograd of the oracle's log-mel steps."""
    from maest_amd.melspectrogram import MelSpectrogram
    B, S = 3, S10 + 77
    wave = randn((B, S), 1, 0.3)
    g = randn((B, 96, 1 + S // 256), 2)
    mel = MelSpectrogram()
    got = ops.logmel_bwd(wave.to(DEV), g.to(DEV), mel._constants(torch.device(DEV)))
    w = wave.double().requires_grad_()
    spec = O.power_spectrogram(w)
    m = torch.matmul(spec.transpose(-1, -2), torch.from_numpy(O.mel_filterbank()).double()).transpose(-1, -2)
    ((torch.log10(1 + m * 10000) - O.NORM_MEAN) / (O.NORM_STD * 2)).backward(g.double())
    e = rel_err(got, w.grad)
    print(f"logmel_bwd vs float64 autograd: {e:.2e}")
    assert e < 1e-4


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_waveform_gradient_fp32_matches_the_oracle(mode):
    sd = O.make_state_dict(625, seed=61)
    net = make(sd, s_patchout_t=20)
    net.train(mode == "train")
    B = 2
    wave = randn((B, S10), 62, 0.3)
    w = randn((B, 400), 63)
    keep = sorted(np.random.Generator(np.random.PCG64(64)).permutation(62)[:42].tolist())
    po = dict(_patchout=(0, torch.tensor(keep))) if mode == "train" else {}
    wd = wave.to(DEV).requires_grad_(True)
    logits, _ = net(wd, **po)
    (logits * w.to(DEV)).sum().backward()
    assert wd.grad is not None and wd.grad.shape == wave.shape and wd.grad.dtype == torch.float32
    want = oracle_wave_grad(wave, sd, w, **(dict(toffset=0, t_keep=keep) if mode == "train" else {}))
    e = rel_err(wd.grad, want)
    print(f"wave.grad fp32 {mode}: {e:.2e}")
    assert e < 1e-3
    # a frozen model: the same wave.grad, no parameter gradient at all
    g_full = wd.grad.clone()
    net.requires_grad_(False)
    net.zero_grad(set_to_none=True)
    wd2 = wave.to(DEV).requires_grad_(True)
    logits, _ = net(wd2, **po)
    (logits * w.to(DEV)).sum().backward()
    assert rel_err(wd2.grad, g_full) < 1e-6
    assert all(p.grad is None for p in net.parameters())


def test_waveform_gradient_1d_chunked_30s():
    """A 1-D 30 s waveform: mel [96, 1876] -> trimmed to 1875 -> reshape + swapaxes into three 625-frame chunks."""
    sd = O.make_state_dict(625, seed=71)
    net = make(sd).eval()
    wave = randn((3 * S10,), 72, 0.3)
    w = randn((3, 400), 73)
    wd = wave.to(DEV).requires_grad_(True)
    logits, _ = net(wd)
    assert logits.shape[0] == 3
    (logits * w.to(DEV)).sum().backward()
    wo = wave.clone().requires_grad_(True)
    m = O.logmel(wo)
    m = m[:, : m.shape[1] - m.shape[1] % 625].reshape(96, 1, -1, 625).swapaxes(0, 2)
    (O.forward(m, oracle_params(sd), (96, 625))[0] * w).sum().backward()
    e = rel_err(wd.grad, wo.grad)
    print(f"wave.grad 1-D 30 s: {e:.2e}")
    assert e < 1e-3


@pytest.mark.parametrize("precision,mode,tol", [("auto", "eval", 1e-3), ("bf16", "train", 1e-2)])
def test_waveform_gradient_other_precisions(precision, mode, tol):
    """The tolerances of test_grad_paths_gpu.py::test_input_gradient_other_precisions: bf16x3 eval at the fp32 gate, bf16 training in
    the G5 band (norm within 3 tol, every element within 10 tol of the largest)."""
    sd = O.make_state_dict(625, seed=81)
    net = make(sd, precision=precision, s_patchout_t=20)
    net.train(mode == "train")
    B = 2
    wave = randn((B, S10), 82, 0.3)
    y = (torch.from_numpy(np.random.Generator(np.random.PCG64(83)).random((B, 400))) < 0.02).float()
    keep = sorted(np.random.Generator(np.random.PCG64(84)).permutation(62)[:42].tolist())
    po = dict(_patchout=(0, torch.tensor(keep))) if mode == "train" else {}
    wd = wave.to(DEV).requires_grad_(True)
    logits, _ = net(wd, **po)
    torch.nn.functional.binary_cross_entropy_with_logits(logits.float(), y.to(DEV)).backward()
    want = oracle_wave_grad(wave, sd, y=y, **(dict(toffset=0, t_keep=keep) if mode == "train" else {}))
    g = wd.grad.float().cpu()
    assert bool(torch.isfinite(g).all())
    e_max = rel_err(g, want)
    e_norm = abs(float(g.norm()) - float(want.norm())) / float(want.norm())
    print(f"wave.grad {precision} {mode}: worst element {e_max:.2e} of the largest, norm {e_norm:.2e}")
    if precision == "auto":
        assert e_max < tol
    else:
        assert e_norm < 3 * tol and e_max < 10 * tol


def test_fp16_waveform_gets_an_fp16_gradient():
    sd = O.make_state_dict(625, seed=91)
    net = make(sd).eval()
    wave = randn((2, S10), 92, 0.3).half()
    w = randn((2, 400), 93).to(DEV)
    w16 = wave.to(DEV).requires_grad_(True)
    (net(w16)[0] * w).sum().backward()
    assert w16.grad is not None and w16.grad.dtype == torch.float16
    w32 = wave.float().to(DEV).requires_grad_(True)
    (net(w32)[0] * w).sum().backward()
    assert rel_err(w16.grad, w32.grad.half().float()) < 1e-3


def test_repeated_backward_is_bit_identical_and_plain_logits_unchanged():
    sd = O.make_state_dict(625, seed=101)
    net = make(sd).eval().requires_grad_(False)
    wave = randn((2, S10), 102, 0.3).to(DEV)
    grads = []
    for _ in range(2):
        wd = wave.clone().requires_grad_(True)
        logits, _ = net(wd)
        logits.sum().backward()
        grads.append(wd.grad)
    assert torch.equal(grads[0], grads[1]), "wave.grad differs between two identical backward passes"
    # a waveform that does not require grad: the plain inference path, logits bit for bit those of the recording forward's inputs
    with torch.no_grad():
        plain = net(wave)[0]
    assert torch.equal(net(wave)[0], plain)
    with torch.no_grad():
        mel_plain = net.melspectrogram(wave)
    mel_grad = net.melspectrogram(wave.clone().requires_grad_(True))
    assert mel_grad.requires_grad and torch.equal(mel_grad.detach(), mel_plain)
