# The extractor (maest_amd/mel_extractor.py) on the GPU: 64 synthetic 300 s tracks at 44.1 kHz in one ragged batch, per-kernel HIP-event
# times against their HBM floors (8 TB/s), the rows kernel's us per 10 s of audio beside logmel_kernel's at the same length, and
# end-to-end files/s of extract_files on WAV files (with the host's decode time alone beside it).
#   python scratch/mel_extract_bench.py [--tracks 64] [--files 32] [--out DIR]      (--files 0: the device batch only, for rocprofv3)
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maest_amd import mel_extractor as X, ops  # noqa: E402
from maest_amd.melspectrogram import MelConstants  # noqa: E402

HBM = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--tracks", type=int, default=64)
ap.add_argument("--seconds", type=float, default=300.0)
ap.add_argument("--files", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(1234)
n_in = int(a.seconds * 44100)
waves = [0.3 * torch.randn(n_in, generator=g, device=dev) for _ in range(a.tracks)]
res = {"tracks": a.tracks, "seconds": a.seconds, "rate_in": 44100}

X.extract(waves[:2], 44100, dev)                                   # warm-up: code objects, tables
torch.cuda.synchronize()
kinds = {"maest_resample", "maest_logmel_rows_f16", "maest_logmel"}
runs = []
for _ in range(a.reps):
    t0 = time.perf_counter()
    with ops.KernelTimer(kinds=kinds) as kt:
        rows = X.extract(waves, 44100, dev)
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    runs.append((wall, kt.summary()))
wall, summ = min(runs, key=lambda r: r[0])
n16 = X.resampled_length(n_in, 44100)
frames = sum(r.shape[0] for r in rows)
rs_bytes = 4.0 * a.tracks * (n_in + n16)
rows_bytes = 4.0 * a.tracks * n16 + 192.0 * frames
rs_ms, rows_ms = summ["maest_resample"]["ms"], summ["maest_logmel_rows_f16"]["ms"]
res["extract_wall_ms"] = wall * 1e3
res["resample"] = {"ms": rs_ms, "floor_ms": rs_bytes / HBM * 1e3, "frac_of_hbm": rs_bytes / HBM * 1e3 / rs_ms, "bytes": rs_bytes}
res["rows"] = {"ms": rows_ms, "floor_ms": rows_bytes / HBM * 1e3, "frac_of_hbm": rows_bytes / HBM * 1e3 / rows_ms, "bytes": rows_bytes,
               "frames": frames}
res["runs_wall_ms"] = [r[0] * 1e3 for r in runs]

# us per 10 s of audio: the rows kernel on 64 x 10 s tracks at 16 kHz vs logmel_kernel on [64, 160000]
ten = [0.3 * torch.randn(160000, generator=g, device=dev) for _ in range(64)]
batch = torch.stack(ten)
c = MelConstants(dev, 16000, 512, 96, norm_mean=0.0, norm_std=0.5)
for _ in range(2):
    X.extract(ten, 16000, dev)
    ops.logmel(batch, c)
torch.cuda.synchronize()
per = {}
for _ in range(5):
    with ops.KernelTimer(kinds=kinds) as kt:
        X.extract(ten, 16000, dev)
        ops.logmel(batch, c)
    for k, v in kt.summary().items():
        per.setdefault(k, []).append(v["ms"])
res["us_per_10s_audio"] = {"rows_kernel": min(per["maest_logmel_rows_f16"]) * 1e3 / 64, "logmel_kernel": min(per["maest_logmel"]) * 1e3 / 64}

if a.files:
    with tempfile.TemporaryDirectory() as td:
        from scipy.io import wavfile
        rng = np.random.default_rng(5)
        srcs, dsts = [], []
        for i in range(a.files):
            pcm = (rng.standard_normal((44100 * 30, 2)) * 6000).astype(np.int16)
            p = os.path.join(td, f"t{i}.wav")
            wavfile.write(p, 44100, pcm)
            srcs.append(p)
            dsts.append(os.path.join(td, "mel", f"t{i}.mmap"))
        X.extract_files(srcs[:2], dsts[:2], force=True, device=dev)
        t0 = time.perf_counter()
        for s in srcs:
            X.decode_wav(s)
        dec = time.perf_counter() - t0
        t0 = time.perf_counter()
        failed = X.extract_files(srcs, dsts, force=True, device=dev)
        torch.cuda.synchronize()
        e2e = time.perf_counter() - t0
        assert not failed
        res["files"] = {"n": a.files, "seconds_each": 30, "format": "44.1 kHz stereo int16 WAV", "files_per_s": a.files / e2e,
                        "wall_s": e2e, "decode_only_s": dec, "host_share": dec / e2e}
print(json.dumps(res, indent=1))
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "mel_extract_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
