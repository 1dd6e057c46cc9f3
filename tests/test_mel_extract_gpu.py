"""GPU: the extractor on an MI355X (maest_logmel_rows_f16 + maest_resample).  Device rows and resampled audio against the host
emulator's (same sources), the on-disk round trip through MelFileReader against the model's own z-normed log-mel, and the centre trim
of a 301 s track.  Audio is generated here from fixed seeds."""
import numpy as np
import pytest
import torch
from scipy.io import wavfile

from maest_amd import _lib, ops
from maest_amd import mel_extractor as X
from maest_amd.melfile import MelFileReader
from maest_amd.melspectrogram import MelConstants, MelSpectrogram

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _seeded(n, seed, scale=0.3):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 44100.0
    tone = 0.2 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * np.sin(2 * np.pi * 3100.0 * t)
    return (tone + scale * rng.standard_normal(n)).astype(np.float32)


def _bits(h):
    return h.contiguous().view(torch.int16)


def _plain_rows(wave):
    c = MelConstants(wave.device, 16000, 512, 96, norm_mean=0.0, norm_std=0.5)
    return ops.logmel(wave[None].contiguous(), c)[0].t().to(torch.float16)


def test_device_matches_emulator():
    from tests.emu import build_emu
    if not build_emu.available():
        pytest.skip("host clang for the emulator build is not available")
    rates = [44100, 48000, 16000]
    waves = [_seeded(r * 3 + 17 * i, 60 + i) for i, r in enumerate(rates)]
    dev_rows = [r.cpu() for r in X.extract(waves, rates, DEV)]
    dev_res = X.resample_batch(waves[:1], 44100, DEV)[0].cpu()
    _lib._testing_override(build_emu.build())
    try:
        emu_rows = X.extract(waves, rates, "cpu")
        emu_res = X.resample_batch(waves[:1], 44100, "cpu")[0]
    finally:
        _lib._testing_restore()
    assert torch.equal(dev_res, emu_res), float((dev_res - emu_res).abs().max())
    differ = 0
    for d, e in zip(dev_rows, emu_rows):
        assert d.shape == e.shape
        diff = (_bits(d).int() - _bits(e).int()).abs()
        assert int(diff.max()) <= 1, "more than one fp16 ulp apart"
        differ += int((diff != 0).any(dim=1).sum())
    print(f"resampled audio bitwise equal; rows differing from the emulator's (<= 1 fp16 ulp): {differ} of "
          f"{sum(d.shape[0] for d in dev_rows)}")


def test_rows_equal_logmel_on_device():
    w = torch.from_numpy(_seeded(160001, 3)).to(DEV)
    got = X.extract([w], 16000, DEV)[0]
    assert torch.equal(_bits(got), _bits(_plain_rows(w)))


def test_round_trip_through_melfile_reader(tmp_path):
    """44.1 kHz stereo WAV -> extract_files -> MelFileReader.load_batch(offset k) vs MelSpectrogram(resampled wave)[..., k:k+625]."""
    n = 44100 * 12
    left, right = _seeded(n, 11), _seeded(n, 12)
    pcm = np.round(np.stack([left, right], 1).clip(-1, 1) * 32767).astype(np.int16)
    wav = tmp_path / "track.wav"
    wavfile.write(wav, 44100, pcm)
    dst = tmp_path / "mel" / "track.mmap"
    assert X.extract_files([wav], [dst], device=DEV) == []
    k = 50
    reader = MelFileReader(base_dir=tmp_path)
    got = reader.load_batch(["mel/track.mmap"], DEV, offsets=[k])[0, 0]          # [96, 625]
    mono, rate = X.decode_wav(wav)
    res = X.resample_batch([mono], rate, DEV)[0]
    want = MelSpectrogram().to(DEV)(res)[:, k: k + 625]
    err = float((got - want).abs().max())
    print(f"round trip vs MelSpectrogram: worst {err:.2e} (z-normed units)")
    assert got.shape == want.shape == (96, 625)
    assert err <= 4e-3


def test_301s_track_is_centre_trimmed():
    S = 301 * 16000
    w = torch.from_numpy(_seeded(S, 21)).to(DEV)
    got = X.extract([w], 16000, DEV)[0]
    T = 1 + S // 256
    assert got.shape == (18750, 96)
    f0 = T // 2 - 18750 // 2
    full = _plain_rows(w)
    assert torch.equal(_bits(got), _bits(full[f0: f0 + 18750]))
