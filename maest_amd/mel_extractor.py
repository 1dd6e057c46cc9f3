"""Audio -> the on-disk mel format the training pipeline reads (``melfile.MelFileReader``, ``csrc/embed.hip:
melfile_assemble_kernel``): raw float16 rows ``[frames, 96]``, no header.

Replaces the reference's ``helpers/melspectrogram_extractor.py`` (same arguments, same trim, same bytes on disk) without its
essentia dependency.  The arithmetic is this project's log-mel (``csrc/mel.hip``: the forward of ``MelSpectrogram``, the reference's
torchaudio restatement of essentia's ``shift_scale_log`` mel) without the z-norm: ``log10(1 + 1e4 mel)``.  A batch of tracks runs as
one ragged batch on the device:

* audio at another rate is resampled to 16 kHz by ``maest_resample`` -- torchaudio ``functional.resample`` with its defaults
  (``sinc_interp_hann``, ``lowpass_filter_width=6``, ``rolloff=0.99``), taps built here in float64 and stored as fp32;
* ``maest_logmel_rows_f16`` computes only the frames the centre trim keeps and writes them as IEEE half rows.

Decoding (WAV only, ``scipy.io.wavfile``), the channel mean and integer PCM scaling happen on the host.  Not pinned: parity with
essentia (absent; its framing differs) and with torchaudio's resampler (absent; the restatement is tested against its own float64
form).  ``MelFileReader.exhaustive_plan`` tiles a track only when its files carry the ``.mmap`` suffix.

CLI: ``python -m maest_amd.mel_extractor audio_file melbands_file [--force] [--max-duration S]`` or ``--list PAIRS.tsv`` (one
``audio<TAB>melbands`` pair per line).
"""
from __future__ import annotations

import argparse
import math
import pathlib
import sys
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

SR = 16000
HOP_SIZE = 256
N_MELS = 96
FRAME_SIZE = 512
MAX_DURATION = 300
LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
ALIGN = 64                     # samples: each track starts here in the packed 16 kHz buffer (the rows kernel's aligned fetch)
BATCH_SAMPLES = 1 << 28        # extract_files: 16 kHz samples per device batch (1 GiB of fp32)


def sinc_taps64(orig: int, new: int, lowpass_filter_width: int = LOWPASS_FILTER_WIDTH, rolloff: float = ROLLOFF):
    """torchaudio's ``_get_sinc_resample_kernel`` (sinc_interp_hann) in float64 for rates already reduced by their gcd:
    -> (taps [new, 2 width + orig], width)."""
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (-np.arange(new, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    safe = np.where(t == 0, 1.0, t)
    kern = np.where(t == 0, 1.0, np.sin(safe) / safe)
    return kern * window * (base / orig), width


class ResampleFilter:
    """Device tables of maest_resample for orig_rate -> new_rate: each phase's non-zero fp32 band (outside |t| < 6 a tap is below
    fp32's smallest subnormal), tap-major and zero-padded to the longest band, with the band's first index into the padded input."""

    def __init__(self, orig_rate: int, new_rate: int, device):
        g = math.gcd(int(orig_rate), int(new_rate))
        self.orig, self.new = int(orig_rate) // g, int(new_rate) // g
        k64, self.width = sinc_taps64(self.orig, self.new)
        k32 = k64.astype(np.float32)
        first, last = np.zeros(self.new, np.int64), np.zeros(self.new, np.int64)
        for p in range(self.new):
            nz = np.nonzero(k32[p])[0]
            first[p], last[p] = (nz[0], nz[-1]) if len(nz) else (0, 0)
        self.n_taps = int((last - first).max()) + 1
        taps = np.zeros((self.n_taps, self.new), np.float32)
        for p in range(self.new):
            band = k32[p, first[p]: first[p] + self.n_taps]
            taps[: len(band), p] = band
        self.taps = torch.from_numpy(taps).to(device)
        self.first = torch.from_numpy(first.astype(np.int32)).to(device)

    def out_length(self, n: int) -> int:
        """ceil(new n / orig): torchaudio's target length."""
        return -(-self.new * int(n) // self.orig)


_FILTERS = {}
_MEL = {}


def _filter(orig_rate, device) -> ResampleFilter:
    key = (int(orig_rate), str(device))
    if key not in _FILTERS:
        _FILTERS[key] = ResampleFilter(orig_rate, SR, device)
    return _FILTERS[key]


def _mel_constants(device):
    from .melspectrogram import MelConstants
    key = str(device)
    if key not in _MEL:
        _MEL[key] = MelConstants(device, SR, FRAME_SIZE, N_MELS)
    return _MEL[key]


def resampled_length(n: int, sample_rate: int) -> int:
    """Samples at 16 kHz of `n` samples at `sample_rate`."""
    if int(sample_rate) == SR:
        return int(n)
    g = math.gcd(int(sample_rate), SR)
    return -(-(SR // g) * int(n) // (int(sample_rate) // g))


def trim_range(frames: int, max_duration: float = MAX_DURATION) -> Tuple[int, int]:
    """(first frame, frame count) the reference keeps of `frames`: all of them up to int(max_duration 16000 / 256), else the centre
    [T // 2 - m // 2, T // 2 + m // 2) -- an even count."""
    max_ts = int(max_duration * SR / HOP_SIZE)
    if frames > max_ts:
        mid = frames // 2
        return mid - max_ts // 2, 2 * (max_ts // 2)
    return 0, frames


def _blocks(counts, per_block):
    """int32 [n + 1]: the first block of each track, ceil(count / per_block) blocks each."""
    b = np.zeros(len(counts) + 1, np.int64)
    b[1:] = np.cumsum([-(-int(c) // per_block) for c in counts])
    if b[-1] >= 2 ** 31:
        raise ValueError("batch too large for one launch")
    return b.astype(np.int32)


def _as_1d(w) -> torch.Tensor:
    t = torch.as_tensor(w)
    if t.dim() != 1:
        raise ValueError(f"extract takes 1-D waveforms, got shape {tuple(t.shape)}")
    return t.float()


def resample_batch(waves: Sequence, sample_rate: int, device, out: Optional[torch.Tensor] = None,
                   out_offsets: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
    """Resample 1-D waveforms at `sample_rate` to 16 kHz in one launch -> the resampled tracks (views of `out` at `out_offsets` when
    given, else of one packed buffer)."""
    dev = torch.device(device)
    filt = _filter(sample_rate, dev)
    ts = [_as_1d(w) for w in waves]
    lens = [int(t.numel()) for t in ts]
    outs = [filt.out_length(n) for n in lens]
    if out is None:
        out_offsets = np.concatenate([[0], np.cumsum(outs)[:-1]]).astype(np.int64).tolist()
        out = torch.empty(int(sum(outs)), dtype=torch.float32, device=dev)
    x = torch.cat([t.to(dev) for t in ts])
    in_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    tab = np.stack([in_off, np.asarray(lens, np.int64), np.asarray(out_offsets, np.int64), np.asarray(outs, np.int64)], 1)
    bs = _blocks(outs, 256)
    ops.resample(x.contiguous(), torch.from_numpy(tab).to(dev), torch.from_numpy(bs).to(dev), int(bs[-1]), filt, out)
    return [out[o: o + n] for o, n in zip(out_offsets, outs)]


def extract(waves: Sequence, sample_rate: Union[int, Sequence[int]], device, max_duration: float = MAX_DURATION) -> List[torch.Tensor]:
    """1-D waveforms (arrays or tensors; `sample_rate` one rate or one per waveform) -> fp16 ``[frames, 96]`` per track on `device`, the
    reference extractor's rows: log10(1 + 1e4 mel) at 16 kHz, hop 256, centre-trimmed to `max_duration`.  One ragged batch: upload,
    one resampling launch per rate other than 16 kHz, one rows launch.  Raises ValueError for a track of <= 256 samples at 16 kHz."""
    dev = torch.device(device)
    rates = [int(sample_rate)] * len(waves) if np.ndim(sample_rate) == 0 else [int(r) for r in sample_rate]
    if len(rates) != len(waves):
        raise ValueError("one sample rate per waveform")
    if not waves:
        return []
    ts = [_as_1d(w) for w in waves]
    S = [resampled_length(t.numel(), r) for t, r in zip(ts, rates)]
    for i, s in enumerate(S):
        if s <= FRAME_SIZE // 2:
            raise ValueError(f"track {i}: {s} samples at 16 kHz; the log-mel's reflect padding needs more than 256")
    off = np.zeros(len(S), np.int64)
    o = 0
    for i, s in enumerate(S):
        off[i] = o
        o += -(-s // ALIGN) * ALIGN
    buf = torch.zeros(max(o, FRAME_SIZE), dtype=torch.float32, device=dev)
    for r in sorted(set(rates)):
        idx = [i for i, q in enumerate(rates) if q == r]
        if r == SR:
            for i in idx:
                buf[off[i]: off[i] + S[i]].copy_(ts[i])
        else:
            resample_batch([ts[i] for i in idx], r, dev, out=buf, out_offsets=[int(off[i]) for i in idx])
    trims = [trim_range(1 + s // HOP_SIZE, max_duration) for s in S]
    counts = [n for _, n in trims]
    row_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    tab = np.stack([off, np.asarray(S, np.int64), np.asarray([f for f, _ in trims], np.int64), np.asarray(counts, np.int64), row_off], 1)
    bs = _blocks(counts, 64)
    rows = ops.logmel_rows_f16(buf, torch.from_numpy(tab).to(dev), torch.from_numpy(bs).to(dev), int(bs[-1]), int(sum(counts)),
                               _mel_constants(dev))
    return [rows[r: r + n] for r, n in zip(row_off.tolist(), counts)]


def write_melfile(path, rows) -> None:
    """Raw float16 bytes of `rows` [frames, 96], no header (the bytes of the reference's ``np.memmap(path, 'float16', 'w+')``);
    creates the parent directories."""
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a, dtype="<f2")
    path = pathlib.Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    a.tofile(path)


def decode_wav(path) -> Tuple[np.ndarray, int]:
    """WAV -> (mono float32 in [-1, 1), rate): integer PCM scaled by its full range (uint8 around 128), float kept, channels averaged."""
    from scipy.io import wavfile
    rate, data = wavfile.read(str(path))
    d = np.asarray(data)
    if d.dtype == np.uint8:
        x = (d.astype(np.float32) - 128.0) / 128.0
    elif d.dtype == np.int16:
        x = d.astype(np.float32) / 32768.0
    elif d.dtype == np.int32:
        x = (d.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif d.dtype.kind == "f":
        x = d.astype(np.float32)
    else:
        raise ValueError(f"unsupported WAV sample type {d.dtype}")
    if x.ndim == 2:
        x = x.mean(axis=1, dtype=np.float64).astype(np.float32)
    if x.ndim != 1 or x.size == 0:
        raise ValueError("empty or malformed WAV data")
    return np.ascontiguousarray(x), int(rate)


def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def extract_files(audio_files: Sequence, melbands_files: Sequence, force: bool = False, max_duration: float = MAX_DURATION,
                  batch_samples: int = BATCH_SAMPLES, device=None) -> List[str]:
    """The reference extractor over many files: decode each WAV, batch tracks up to `batch_samples` samples at 16 kHz, extract, write
    each ``melbands_file``.  Existing outputs are skipped unless `force`.  A file that fails to decode or is too short (<= 256 samples at
    16 kHz) is reported as ``Error while processing <file>`` and skipped; returns those files."""
    if len(audio_files) != len(melbands_files):
        raise ValueError("one melbands file per audio file")
    dev = torch.device(device) if device is not None else _default_device()
    failed: List[str] = []
    pending: List[Tuple[np.ndarray, int, str]] = []
    budget = 0

    def fail(f):
        print(f"Error while processing {f}")
        failed.append(str(f))

    def flush():
        nonlocal pending, budget
        if pending:
            out = extract([w for w, _, _ in pending], [r for _, r, _ in pending], dev, max_duration)
            for (_, _, dst), rows in zip(pending, out):
                write_melfile(dst, rows)
        pending, budget = [], 0

    for src, dst in zip(audio_files, melbands_files):
        if pathlib.Path(dst).exists() and not force:
            continue
        try:
            wave, rate = decode_wav(src)
        except Exception:          # noqa: BLE001 -- any decoder failure is reported per file, as the reference does
            fail(src)
            continue
        n16 = resampled_length(wave.size, rate)
        if n16 <= FRAME_SIZE // 2:
            fail(src)
            continue
        if pending and budget + n16 > batch_samples:
            flush()
        pending.append((wave, rate, str(dst)))
        budget += n16
    flush()
    return failed


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Computes the mel spectrogram of a given audio file.")
    ap.add_argument("audio_file", nargs="?", help="the name of the file from which to read")
    ap.add_argument("melbands_file", nargs="?", help="the name of the output file")
    ap.add_argument("--force", "-f", action="store_true", help="force")
    ap.add_argument("--max-duration", type=float, default=MAX_DURATION, help="max duration in seconds")
    ap.add_argument("--list", metavar="PAIRS.tsv", help="extract many files: one 'audio<TAB>melbands' pair per line")
    a = ap.parse_args(argv)
    if a.list:
        src, dst = [], []
        for ln in pathlib.Path(a.list).read_text().splitlines():
            if ln.strip():
                s, d = ln.split("\t")[:2]
                src.append(s)
                dst.append(d)
    elif a.audio_file and a.melbands_file:
        src, dst = [a.audio_file], [a.melbands_file]
    else:
        ap.error("give audio_file and melbands_file, or --list")
    failed = extract_files(src, dst, force=a.force, max_duration=a.max_duration)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
