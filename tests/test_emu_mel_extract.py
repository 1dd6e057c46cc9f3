"""CPU (`-m "not gpu"`): the extractor's device path (maest_logmel_rows_f16 and maest_resample, csrc/mel.hip) from the SAME sources under
the host SIMT emulator (tests/emu): the fp16 rows against maest_logmel's own frames bit for bit, against the oracle's float64 log-mel
within one fp16 ulp, and the resampler against a float64 restatement of torchaudio's functional.resample (sinc_interp_hann, width 6,
rolloff 0.99) written out here."""
import math

import numpy as np
import pytest
import torch

from maest_amd import mel_extractor as X
from maest_amd import ops
from maest_amd.melspectrogram import MelConstants
from oracle import maest_oracle as O
from tests.kernel_cases import rnd


def _consts():
    return MelConstants("cpu", 16000, 512, 96, norm_mean=0.0, norm_std=0.5)      # log10(1 + 1e4 mel), 2 std = 1: no z-norm


def _bits(h):
    return h.contiguous().view(torch.int16)


def _plain_rows(wave):
    """float16(maest_logmel(wave, norm_mean=0, norm_2std=1)) as rows [T, 96]."""
    return ops.logmel(wave[None].contiguous(), _consts())[0].t().to(torch.float16)


def _rows(waves, offsets, trims):
    """maest_logmel_rows_f16 on `waves` packed at `offsets` with (f0, n) per track -> the per-track rows."""
    total = max(o + w.numel() for o, w in zip(offsets, waves))
    buf = torch.zeros(total, dtype=torch.float32)
    for o, w in zip(offsets, waves):
        buf[o: o + w.numel()] = w
    counts = [n for _, n in trims]
    r0 = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    tab = torch.tensor([[o, w.numel(), f, n, r] for o, w, (f, n), r in zip(offsets, waves, trims, r0)], dtype=torch.int64)
    bs = torch.from_numpy(X._blocks(counts, 64))
    rows = ops.logmel_rows_f16(buf, tab, bs, int(bs[-1]), int(sum(counts)), _consts())
    return [rows[r: r + n] for r, n in zip(r0.tolist(), counts)]


@pytest.mark.parametrize("S", [257, 2560, 64 * 256 + 77])
def test_emu_rows_equal_logmel_bitwise(emu, S):
    w = rnd((S,), 500 + S, 0.3)
    got = X.extract([w], 16000, "cpu")[0]
    want = _plain_rows(w)
    assert got.shape == (1 + S // 256, 96)
    assert torch.equal(_bits(got), _bits(want))


def test_emu_trimmed_rows_are_a_slice(emu):
    """f0 > 0, both reflect edges, counts that are not multiples of 64."""
    S = 150 * 256 + 131
    T = 1 + S // 256
    w = rnd((S,), 71, 0.3)
    full = _plain_rows(w)
    trims = [(0, 70), (T - 75, 75), (37, 100), (64, 64), (T - 1, 1)]
    got = _rows([w] * len(trims), [0] * len(trims), trims)
    for (f0, n), g in zip(trims, got):
        assert torch.equal(_bits(g), _bits(full[f0: f0 + n])), (f0, n)


def test_emu_rows_ragged_batch_equals_alone(emu):
    """Lengths 257, 300, 16 000 and 160 001 and one track that starts on an odd sample (no aligned fetch), in one launch."""
    lens = [257, 300, 16000, 160001, 20000]
    waves = [rnd((n,), 900 + i, 0.3) for i, n in enumerate(lens)]
    offsets, o = [], 0
    for n in lens[:-1]:
        offsets.append(o)
        o += -(-n // 64) * 64
    offsets.append(o + 3)                                   # 12 bytes past a 64-sample boundary
    trims = [(0, 1 + n // 256) for n in lens]
    got = _rows(waves, offsets, trims)
    for w, g in zip(waves, got):
        assert torch.equal(_bits(g), _bits(_plain_rows(w))), w.numel()
    # and through the public API (64-sample aligned packing)
    for w, g in zip(waves, X.extract(waves, 16000, "cpu")):
        assert torch.equal(_bits(g), _bits(_plain_rows(w)))


def test_emu_rows_within_one_fp16_ulp_of_float64(emu):
    S = 40 * 256 + 9
    w = rnd((S,), 33, 0.3)
    spec = O.power_spectrogram(w.double())
    mel = torch.matmul(spec.transpose(-1, -2), torch.from_numpy(O.mel_filterbank()).double())
    want = torch.log10(1 + 1e4 * mel).numpy()                     # [T, 96]
    got = X.extract([w], 16000, "cpu")[0].float().numpy()
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    err = np.abs(got - want) / ulp
    print(f"rows vs float64 log-mel: worst {err.max():.3f} fp16 ulp")
    assert err.max() <= 1.0


def _resample64(x, orig, new, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio.functional.resample (sinc_interp_hann) in float64, written out: the gcd, the [new, 2 width + orig] kernel, the padded
    strided convolution, the target length."""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    kern = np.zeros((new, 2 * width + orig))
    for p in range(new):
        for k in range(2 * width + orig):
            t = (-p / new + (k - width) / orig) * base
            t = max(-lowpass_filter_width, min(lowpass_filter_width, t))
            win = math.cos(t * math.pi / lowpass_filter_width / 2) ** 2
            s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
            kern[p, k] = s * win * base / orig
    xp = np.concatenate([np.zeros(width), np.asarray(x, np.float64), np.zeros(width + orig)])
    n_frames = (xp.size - kern.shape[1]) // orig + 1
    frames = np.lib.stride_tricks.as_strided(xp, (n_frames, kern.shape[1]), (8 * orig, 8))
    y = (frames @ kern.T).reshape(-1)
    return y[: math.ceil(new * len(x) / orig)]


@pytest.mark.parametrize("rate", [44100, 48000, 22050, 32000, 8000])
def test_emu_resample_matches_float64_torchaudio(emu, rate):
    """A ragged batch of three lengths at one rate; output lengths exact, relative max error <= 1e-5."""
    lens = [rate // 10 + 7, 1000, 37]
    waves = [rnd((n,), rate + n, 0.3) for n in lens]
    got = X.resample_batch(waves, rate, "cpu")
    for w, g in zip(waves, got):
        want = _resample64(w.numpy(), rate, 16000)
        assert g.numel() == want.size == math.ceil(16000 * w.numel() / rate)
        err = float(np.abs(g.double().numpy() - want).max() / np.abs(want).max())
        print(f"{rate} Hz, {w.numel()} samples: rel max error {err:.2e}")
        assert err <= 1e-5, (rate, w.numel(), err)


def test_emu_extract_mixed_rates_one_batch(emu):
    """Five rates into 16 kHz in one extract() call: each track's rows equal those of its float64-resampled wave within one fp16
    ulp-equivalent of the fp32 path, and the frame counts follow the exact resampled lengths."""
    rates = [44100, 48000, 22050, 32000, 8000]
    waves = [rnd((r // 8 + 11 * i,), 40 + i, 0.3) for i, r in enumerate(rates)]
    got = X.extract(waves, rates, "cpu")
    for w, r, g in zip(waves, rates, got):
        n16 = math.ceil(16000 * w.numel() / r)
        assert X.resampled_length(w.numel(), r) == n16
        assert g.shape == (1 + n16 // 256, 96)
        res = X.resample_batch([w], r, "cpu")[0]
        assert torch.equal(_bits(g), _bits(_plain_rows(res)))
