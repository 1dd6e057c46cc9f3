"""CPU: the extractor's host layer (maest_amd/mel_extractor.py) -- trim arithmetic, the file format, WAV decoding, skip / force and the
error path of extract_files (device work under the host SIMT emulator) -- and the argument checks of the two new C-ABI entries."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from maest_amd import _lib
from maest_amd import mel_extractor as X
from tests.kernel_cases import rnd

P1 = 256                 # a non-null "pointer": never dereferenced, every call below fails its checks first


@pytest.mark.parametrize("frames, max_duration, want", [
    (18750, 300, (0, 18750)),              # exactly max_ts: kept whole
    (18751, 300, (9375 - 9375, 18750)),    # T // 2 = 9375, max_ts = 18750 (even)
    (18813, 300, (9406 - 9375, 18750)),    # a 301 s track
    (1000, 10.0, (500 - 312, 624)),        # max_ts = int(10 * 16000 / 256) = 625 (odd): an even count of 624
    (1001, 10.0, (500 - 312, 624)),
    (625, 10.0, (0, 625)),
    (626, 10.0, (313 - 312, 624)),
])
def test_trim_range(frames, max_duration, want):
    assert X.trim_range(frames, max_duration) == want
    f0, n = want
    if frames > int(max_duration * 16000 / 256):           # the reference's slice, literally
        a = np.arange(frames)
        mid, m = frames // 2, int(max_duration * 16000 / 256)
        assert list(a[mid - m // 2: mid + m // 2]) == list(range(f0, f0 + n))


def test_resampled_length():
    assert X.resampled_length(44100, 44100) == 44100 * 16000 // 44100 == 16000
    assert X.resampled_length(44101, 44100) == 16001           # ceil(160 * 44101 / 441)
    assert X.resampled_length(1000, 16000) == 1000
    assert X.resampled_length(3, 8000) == 6


def test_filter_bands():
    """44.1 kHz: 475 taps per phase in torchaudio's kernel, about 35 of them non-zero in fp32; the band covers every non-zero tap."""
    f = X.ResampleFilter(44100, 16000, "cpu")
    assert (f.orig, f.new, f.width) == (441, 160, 17)
    assert 30 <= f.n_taps <= 40
    k64, width = X.sinc_taps64(441, 160)
    assert k64.shape == (160, 2 * 17 + 441) and width == 17
    taps, first = f.taps.numpy(), f.first.numpy()
    for p in range(160):
        full = np.zeros(k64.shape[1], np.float32)
        full[first[p]: first[p] + f.n_taps] = taps[:, p][: k64.shape[1] - first[p]]
        assert np.array_equal(full, k64[p].astype(np.float32)), p


def test_write_melfile(tmp_path):
    rows = (rnd((123, 96), 5) * 3).to(torch.float16)
    p = tmp_path / "a" / "b" / "x.mmap"
    X.write_melfile(p, rows)
    assert p.stat().st_size == 123 * 192
    ref = tmp_path / "ref.mmap"                                  # the reference writer's bytes
    fp = np.memmap(ref, dtype="float16", mode="w+", shape=(123, 96))
    fp[:] = rows.numpy()[:]
    del fp
    assert p.read_bytes() == ref.read_bytes()


@pytest.mark.parametrize("dtype", ["int16", "int32", "uint8", "float32", "float64"])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_decode_wav(tmp_path, dtype, channels):
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.9, 0.9, (1000, channels))
    if dtype == "int16":
        d, scale, shift = np.round(x * 32767).astype(np.int16), 32768.0, 0.0
    elif dtype == "int32":
        d, scale, shift = np.round(x * 2147483000).astype(np.int32), 2147483648.0, 0.0
    elif dtype == "uint8":
        d, scale, shift = np.round(x * 127 + 128).astype(np.uint8), 128.0, 128.0
    else:
        d, scale, shift = x.astype(dtype), 1.0, 0.0
    if channels == 1:
        d = d[:, 0]
    p = tmp_path / "a.wav"
    wavfile.write(p, 22050, d)
    wave, rate = X.decode_wav(p)
    assert rate == 22050 and wave.dtype == np.float32 and wave.shape == (1000,)
    want = ((d.astype(np.float64) - shift) / scale).reshape(1000, -1).mean(axis=1)
    assert np.abs(wave - want).max() <= 1e-6


def _wav(path, n, rate=16000, seed=0):
    x = (rnd((n,), seed, 0.2).numpy() * 32767).astype(np.int16)
    wavfile.write(path, rate, x)


def test_extract_files_skip_force_and_errors(emu, tmp_path, capsys):
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    _wav(a, 5000, 16000, 1)
    _wav(b, 6000, 44100, 2)
    short = tmp_path / "short.wav"
    _wav(short, 700, 44100, 3)                                   # 254 samples at 16 kHz
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"RIFF....not a wave file")
    srcs = [a, short, bad, b]
    dsts = [tmp_path / "out" / (p.stem + ".mmap") for p in srcs]
    failed = X.extract_files(srcs, dsts, device="cpu", batch_samples=4000)     # a budget below one track: one batch per track
    assert failed == [str(short), str(bad)]
    out = capsys.readouterr().out
    assert f"Error while processing {short}" in out and f"Error while processing {bad}" in out
    assert not dsts[1].exists() and not dsts[2].exists()
    ra = np.fromfile(dsts[0], dtype=np.float16).reshape(-1, 96)
    assert ra.shape == (1 + 5000 // 256, 96)
    assert dsts[3].stat().st_size == (1 + X.resampled_length(6000, 44100) // 256) * 192
    want = X.extract([X.decode_wav(a)[0]], 16000, "cpu")[0].numpy()
    assert np.array_equal(ra.view(np.int16), want.view(np.int16))
    # existing outputs are skipped ...
    dsts[0].write_bytes(b"keep")
    assert X.extract_files([a], [dsts[0]], device="cpu") == []
    assert dsts[0].read_bytes() == b"keep"
    # ... unless forced
    assert X.extract_files([a], [dsts[0]], force=True, device="cpu") == []
    assert dsts[0].stat().st_size == (1 + 5000 // 256) * 192


def test_cli_list(emu, tmp_path, monkeypatch):
    a = tmp_path / "a.wav"
    _wav(a, 3000, 48000, 4)
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text(f"{a}\t{tmp_path / 'm' / 'a.mmap'}\n")
    monkeypatch.setattr(X, "_default_device", lambda: torch.device("cpu"))
    assert X.main(["--list", str(pairs)]) == 0
    assert (tmp_path / "m" / "a.mmap").stat().st_size == (1 + 1000 // 256) * 192
    assert X.main([str(tmp_path / "missing.wav"), str(tmp_path / "m" / "b.mmap")]) == 1


def test_extract_rejects_short_track(emu):
    with pytest.raises(ValueError, match="256"):
        X.extract([np.zeros(256, np.float32)], 16000, "cpu")


# ---- C-ABI argument checks (the gfx950 build when present and the emulator build)

def _libs():
    out = []
    if os.path.exists(_lib.LIB_PATH):
        out.append("gfx950")
    from tests.emu import build_emu
    if build_emu.available():
        out.append("emu")
    return out


@pytest.fixture(params=_libs())
def lib(request):
    if request.param == "emu":
        from tests.emu import build_emu
        _lib._testing_override(build_emu.build())
        yield _lib.load()
        _lib._testing_restore()
    else:
        yield _lib.load()


def _rows(lib, **kw):
    a = dict(wave=P1, total_in=160000, tracks=P1, bs=P1, n=2, nb=20, window=P1, twiddle=P1, fb_start=P1, fb_len=P1, fb_w=P1,
             fb_stride=16, rows=P1, total_rows=1000)
    a.update(kw)
    return lib.maest_logmel_rows_f16(a["wave"], a["total_in"], a["tracks"], a["bs"], a["n"], a["nb"], a["window"], a["twiddle"],
                                     a["fb_start"], a["fb_len"], a["fb_w"], a["fb_stride"], 1e4, a["rows"], a["total_rows"], None)


@pytest.mark.parametrize("kw, msg", [
    (dict(wave=None), b"null pointer"),
    (dict(tracks=None), b"null pointer"),
    (dict(bs=None), b"null pointer"),
    (dict(window=None), b"null pointer"),
    (dict(fb_w=None), b"null pointer"),
    (dict(rows=None), b"null pointer"),
    (dict(n=0), b"bad shape"),
    (dict(nb=0), b"bad shape"),
    (dict(total_in=256), b"S > 256"),
    (dict(total_rows=0), b"bad shape"),
    (dict(fb_stride=0), b"bad fb_stride"),
    (dict(rows=P1 + 2), b"16-byte aligned"),
])
def test_logmel_rows_rejects(lib, kw, msg):
    assert _rows(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def _rs(lib, **kw):
    a = dict(x=P1, total_in=44100, tracks=P1, bs=P1, n=1, nb=63, orig=441, new=160, width=17, taps=P1, first=P1, n_taps=35, out=P1,
             total_out=16000)
    a.update(kw)
    return lib.maest_resample(a["x"], a["total_in"], a["tracks"], a["bs"], a["n"], a["nb"], a["orig"], a["new"], a["width"], a["taps"],
                              a["first"], a["n_taps"], a["out"], a["total_out"], None)


@pytest.mark.parametrize("kw, msg", [
    (dict(x=None), b"null pointer"),
    (dict(tracks=None), b"null pointer"),
    (dict(taps=None), b"null pointer"),
    (dict(first=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
    (dict(n=0), b"bad shape"),
    (dict(total_out=0), b"bad shape"),
    (dict(orig=0), b"bad filter"),
    (dict(n_taps=0), b"bad filter"),
    (dict(n_taps=2 * 17 + 441 + 1), b"bad filter"),
])
def test_resample_rejects(lib, kw, msg):
    assert _rs(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def test_abi_version_unchanged():
    names = list(_lib.SIGNATURES)
    assert "maest_logmel_rows_f16" in names and "maest_resample" in names
    assert _lib.ABI_VERSION == 9
