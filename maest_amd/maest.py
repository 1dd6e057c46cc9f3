"""MAEST (patchout audio-spectrogram transformer) with the reference's Python surface and an
MI355X-native execution engine underneath.

Drop-in surface (reference file:line, paths relative to palonso/MAEST):
  * ``get_maest(arch, ...)``                      models/maest.py:1467-1569
  * ``MAEST.forward(x, transformer_block=-1, return_self_attention=False,
                    melspectrogram_input=False)``  models/maest.py:831-933
  * ``MAEST.predict_labels(x)``                   models/maest.py:935-939
  * state_dict names / shapes                     models/maest.py:516-530, 537-553, 570-582
  * exception contract                            models/maest.py:855-861, 664-668, 1530

What is different: no tensor op of the hot path is dispatched to torch.  ``forward`` drives the
hand-written gfx950 kernels of libmaest_hip.so (C ABI: include/maest_hip.h) through ctypes;
PyTorch only owns the device memory, the stream and -- in training -- the autograd edge
(one ``torch.autograd.Function`` spanning the whole network, whose backward runs the hand-written
backward kernels and hands fp32 parameter gradients to the optimizer).

Numeric modes (``model.precision``):
  "fp32"  parity mode: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere; matches the reference's
          fp32 CPU path to ~1e-5 (gate: 1e-3 relative, identical top-k labels);
  "bf16"  perf mode: bf16 MFMA operands, fp32 accumulation, fp32 residual stream / LayerNorm /
          softmax / GELU (the reference trains under fp16 autocast, ex_maest.py:51);
  "bf16x3" fast parity mode: fp32 tensors everywhere, the linear layers and the attention forward as three bf16
          MFMAs on hi/lo splits of the fp32 operands (SURVEY H1 "split-bf16"): meets the same 1e-3 gate as "fp32"
          at 2-2.5x its speed (forward and backward; small / ragged GEMMs stay exact fp32);
  "fp16"  fast parity mode (round 6): the "bf16" kernels' schedules with IEEE-half operands (v_mfma_*_f16; the library's second
          build, libmaest_hip_f16.so) -- the reference's own GPU arithmetic (16-mixed autocast) --: logits 6e-4 .. 8e-4 from fp32, inside the
          1e-3 gate, at the bf16 mode's speed.  A train() forward records and differentiates in half too (gradients 8 x closer to fp32 than
          bf16's) and, as under autocast, wants a SCALED loss (torch.amp.GradScaler); eval() forwards never record;
  "auto"  (default) bf16 for a training forward that records a graph; every other forward -- eval(), no_grad,
          predict_labels -- runs "bf16x3" (the reference computes inference in fp32; the split products meet the
          same 1e-3 / identical-ranking gates at twice the speed of the exact ones; precision="fp32" selects those).
"""
from __future__ import annotations

import logging
import collections
import contextlib
import math
import os
import warnings
import weakref
from functools import partial
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .labels import discogs_400labels, discogs_519labels
from .melspectrogram import MelSpectrogram

LOG2E = 1.4426950408889634      # softmax exponent base change (csrc/attn_common.h)

_logger = logging.getLogger("MAEST")

EMBED_DIM = 768
HEAD_TOKENS = 2          # cls, dist: the tokens the final norm + head read (models/maest.py:819-826)
DEPTH = 12
NUM_HEADS = 12
PATCH = 16


# --------------------------------------------------------------------------------------
# parameter containers (same module tree / state_dict keys as the reference; these modules
# only HOLD parameters -- their torch forward() is never called on the hot path)
# --------------------------------------------------------------------------------------
class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=12, qkv_bias=True):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, eps=1e-6):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class PatchEmbed(nn.Module):
    """Parameter holder + geometry of the 16x16 / stride-10 patch embedding (maest.py:214-256)."""

    def __init__(self, img_size, patch_size=16, stride=10, in_chans=1, embed_dim=768):
        super().__init__()
        self.img_size = tuple(img_size)
        self.patch_size = (patch_size, patch_size)
        self.stride = tuple(stride) if isinstance(stride, (tuple, list)) else (stride, stride)
        self.grid_size = (img_size[0] // self.stride[0], img_size[1] // self.stride[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.flatten = False
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.stride)


def _init_vit_weights(module: nn.Module):
    """maest.py:942-976 as reached through ``self.apply`` (name == ""): trunc-normal(.02) Linear
    weights (the head included), zero biases, LayerNorm ones/zeros, Conv2d left at torch default."""
    if isinstance(module, nn.Linear):
        nn.init.trunc_normal_(module.weight, std=0.02, a=-2.0, b=2.0)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.LayerNorm):
        nn.init.zeros_(module.bias)
        nn.init.ones_(module.weight)


# --------------------------------------------------------------------------------------
# the execution engine
# --------------------------------------------------------------------------------------
class _Weights:
    """Operand-dtype copies of the fp32 master parameters (and their transposes for dgrad),
    rebuilt only when a parameter's version counter moves (i.e. after an optimizer step)."""

    def __init__(self):
        self._cache = {}
        self.seen_train = 0     # _Engine._train_forwards when an EVALUATION forward last filled the cache; -1: a training forward did (stale)
        self.epoch = 0          # bumped whenever every copy is dropped (part of the hipGraph cache key)
        self.builds = 0         # copies (re)built so far: a forward during which it moves found the cache cold (MAEST._eval_forward)
        # {id(parameter): rows}: parameters whose PLAIN low-precision copy carries `row_scale` on its first `rows` rows (the q rows of
        # the qkv projections in bf16 mode: include/maest_hip.h MAEST_BF16_QS); the transposed copies (dgrad) stay unscaled
        self.scaled_rows = {}
        self.row_scale = 1.0

    def _srows(self, p, dtype):
        return self.scaled_rows.get(id(p), 0) if dtype != torch.float32 else 0

    def _key(self, p, dtype, transposed, pad_cols_to=0):
        # a row-scaled plain copy is keyed by its scaling, so that it coexists with the unscaled copy of the same parameter (alternating
        # bf16 and fp32 / bf16x3 forwards on one model then drop nothing, and captured evaluation graphs stay valid: ADVICE r5)
        rows = 0 if transposed else self._srows(p, dtype)
        return (id(p), dtype, transposed, pad_cols_to) if rows == 0 else (id(p), dtype, transposed, pad_cols_to, rows, self.row_scale)

    def get(self, p: torch.Tensor, dtype, transposed=False, pad_cols_to: int = 0):
        key = self._key(p, dtype, transposed, pad_cols_to)
        hit = self._fresh(key, p)
        if hit is not None:
            return hit
        src = p.detach()
        w2 = src.reshape(src.shape[0], -1)
        self.builds += 1
        if not transposed:
            if dtype == torch.float32:
                out = w2
            elif self._srows(p, dtype):
                out = ops.cast_weights_multi([w2], dtype, want=True, want_t=False, scaled_rows=[self._srows(p, dtype)],
                                             row_scale=self.row_scale)[0][0]
            else:
                out, _ = ops.cast_weights(w2, dtype, want=True, want_t=False)
        else:
            if pad_cols_to:
                lp = w2 if dtype == torch.float32 else ops.cast_weights(w2, dtype)[0]
                out = ops.transpose(lp, ops.round_up(w2.shape[0], pad_cols_to))
            else:
                _, out = ops.cast_weights(w2, dtype, want=False, want_t=True)
        self._store(key, p, out)
        return out

    def _fresh(self, key, p):
        """The cached copy under `key` if it was made from THIS parameter object (id() of a freed parameter can be
        reused by a new one) at its current version and device; None otherwise."""
        hit = self._cache.get(key)
        if hit is not None and hit[0] == p._version and hit[2]() is p and hit[1].device == p.device:
            return hit[1]
        return None

    def _store(self, key, p, out):
        self._cache[key] = (p._version, out, weakref.ref(p))

    def _build(self, params, key, dtype, *, want=True, want_t=False, rows=None, src=lambda p: p.detach(), view=lambda o: o):
        """The one way copies made by ops.cast_weights_multi enter the cache.  key(p, transposed) names a copy of parameter p; the
        parameters one of whose wanted copies is not fresh are rebuilt together, in ONE launch (`src`: the fp32 matrix handed to it,
        `rows`: the row-scaled rows of p's plain copy, `view`: the shape a copy is cached in).  Returns the plain copies in order."""
        stale = [p for p in params if any(self._fresh(key(p, tr), p) is None for tr in ((False, True) if want_t else (False,)))]
        if stale:
            self.builds += 1
            scaled = {} if rows is None else dict(scaled_rows=[rows(p) for p in stale], row_scale=self.row_scale)
            outs = ops.cast_weights_multi([src(p) for p in stale], dtype, want=want, want_t=want_t, **scaled)
            for p, copies in zip(stale, outs):
                for tr, o in zip((False, True), copies):
                    if o is not None:
                        self._store(key(p, tr), p, view(o))
        return [self._cache[key(p, False)][1] for p in params] if want else None

    def refresh(self, params, dtype, with_t: bool):
        """Bring the plain (and, for training, transposed) operand copies of `params` up to date in one launch."""
        if dtype == torch.float32 and not with_t:
            return
        self._build(params, lambda p, tr: self._key(p, dtype, tr), dtype, want=dtype != torch.float32, want_t=with_t,
                    rows=lambda p: self._srows(p, dtype))

    def split3(self, params):
        """MAEST_SPLIT3_B copies (bf16 [out, 3 * in]: hi | lo | hi) of fp32 weight matrices, stale ones rebuilt in one launch; cached
        like the other operand copies.  Returns them in order."""
        return self._build(params, lambda p, tr: (id(p), "split3b", False, 0), ops.SPLIT3)

    def scaled_biases(self, biases, rows: int):
        """fp32 copies of `biases` with the first `rows` entries multiplied by row_scale (the q part of the qkv biases beside the
        row-scaled weight copies), all in one launch; cached like the weight copies."""
        return self._build(biases, lambda b, tr: (id(b), "scaled-bias", False, rows, self.row_scale), torch.float32, rows=lambda b: rows,
                           src=lambda b: b.detach().reshape(-1, 1), view=lambda o: o.reshape(-1))

    def clear(self):
        self._cache.clear()
        self.epoch += 1
        self.builds += 1


def _block_sites(reg, i: int):
    """Block i's regularised sites (include/maest_hip.h: site 8 * i + k), (site, rate) or None each; None for a block with none, which
    keeps the launches of an unregularised forward.  reg: the forward's drop rate `p` and per-block drop-path rates `dpr`, or None."""
    if reg is None or not (reg["p"] > 0 or reg["dpr"][i] > 0):
        return None
    elem = lambda k: (8 * i + k, reg["p"]) if reg["p"] > 0 else None
    path = lambda k: (8 * i + k, reg["dpr"][i]) if reg["dpr"][i] > 0 else None
    return dict(elem_a=elem(0), path_a=path(1), elem_h=elem(2), elem_m=elem(3), path_m=path(4))


def _split_k(n_out: int, k_out: int, tokens: int) -> int:
    """K splits of a wgrad so that ~1024 workgroups are in flight (4 per CU) whatever the weight shape."""
    tiles = math.ceil(n_out / 128) * math.ceil(k_out / 128)
    return max(1, min(1024 // tiles, math.ceil(tokens / 64)))


def _wgrad(dy: torch.Tensor, x: torch.Tensor, n_out: int, k_out: int, out=None, bias_out=None, x3=False, wgs: int = 0) -> torch.Tensor:
    """dW[n_out, k_out] = dy[M, n_out]^T @ x[M, k_out] (fp32) and, fused in the same kernel,
    db[n_out] = dy.sum(0): token-major operands are consumed in place (csrc/gemm.hip: gemm_tn_kernel).
    `out` / `bias_out` (pre-zeroed fp32) receive the results if given.  wgs > 0: about that many workgroups (K splits = wgs // tiles)
    instead of the kernel's own plan, which fills the 256 CUs in one round."""
    dw = (torch.zeros((n_out, k_out), dtype=torch.float32, device=dy.device) if out is None
          else out.view(n_out, k_out))
    split = 0                                                                     # 0 = kernel-chosen split
    if wgs > 0 and n_out % 256 == 0 and k_out % 256 == 0:
        split = max(1, wgs // ((n_out // 256) * (k_out // 256)))
    ops.gemm_tn(dy, x, dw, colsum=bias_out, split_k=split, M=n_out, N=k_out, x3=x3)
    return dw


# The engines' extra streams, ONE set per device and process (every engine of a device shares them).  torch hands out the 32 streams of
# its pool round robin and the runtime multiplexes them onto a few hardware queues: which pool entry an engine's weight-gradient stream is
# decides whether it has a queue of its own or sits behind the caller's stream -- where the narrow (108 - 126 workgroups) wgrad launches run
# one after the other INSTEAD of beside the dgrad chain.  With a stream per engine, the fifth model of a process lost 12 % of its training
# step to exactly that (bench.py's 30 s training case behind three evaluation cases that had each taken a stream: 89.2 ms against 79.6,
# profiles/r06_stream_identity.txt).  All three roles are created together, on first use, in a fixed order.
# Measured per pool entry (scratch/r06_stream_identity.py: a 108-workgroup wgrad on pool stream k beside an NT GEMM on the default stream,
# 503 + 281 us alone).  With the runtime's default of four hardware queues: 575 - 600 us together on entries 0 - 5, 7 - 9, 11; 755 - 786 us --
# nearly serial -- on entries 6 and 10, which land on the default stream's queue.  With eight hardware queues (a job's own setting):
# 585 - 600 us, and 662 - 677 us on entries 3 and 10.  Those entries are passed over (the index is the pool stream's id >> 5); with any other
# queue count nothing is skipped, and a runtime that maps differently loses nothing.
_ENGINE_STREAMS = {}
_RUNTIME_DEFAULT_QUEUES = "4"          # the HIP runtime's count when the environment sets none


def _on_default_queue(k: int, queues=None) -> bool:
    """Whether pool entry k shares the default stream's hardware queue at `queues` queues (default: the process's count)."""
    q = str(queues) if queues is not None else os.environ.get("GPU_MAX_HW_QUEUES") or _RUNTIME_DEFAULT_QUEUES
    return (k >= 4 and k % 4 == 2) if q == "4" else (k % 7 == 3) if q == "8" else False


def _pool_stream(dev):
    for _ in range(8):
        s = torch.cuda.Stream(device=dev)
        if not _on_default_queue(int(s.stream_id) >> 5):
            break
    return s


def _engine_stream(dev, role):
    key = str(dev)
    if key not in _ENGINE_STREAMS:
        _ENGINE_STREAMS[key] = {r: _pool_stream(dev) for r in ("side", "comm", "eval")}
    return _ENGINE_STREAMS[key][role]


class _Engine:
    """Forward / backward of the whole network as a fixed sequence of C-ABI kernel launches."""

    def __init__(self, model: "MAEST"):
        self.m = model
        self.w = _Weights()
        self.w_f16 = _Weights()          # operand copies of precision="fp16" forwards (made by the half-precision build of the kernels)
        self.overlap_wgrad = True
        # The head reads two tokens (cls, dist) of the last block's output (models/maest.py:819-826), and everything in a
        # block after the attention's key / value side is per token: the last block therefore evaluates its attention
        # queries, proj, norm2 and MLP -- forward and backward -- only on those two rows of every clip.  Outputs and
        # gradients are the ones of the full evaluation (the skipped rows feed nothing and receive no gradient).
        self.head_tail = True
        # the attention backward's delta = rowsum(dO * O) comes out of the epilogue of the proj dgrad GEMM (which produces
        # dO) instead of a separate pass over dO and O (ops.gemm_nt_rowdot)
        self.fold_delta = True
        # bf16 mode: scale * log2(e) of the softmax rides in the q rows of the qkv projections' forward operand copies (and in the q part
        # of a copy of their biases), so the attention kernels read q' = scale * log2(e) * q rounded ONCE (MAEST_BF16_QS: the forward
        # takes its fragments straight from the rows, forward and backward exponentiate the same operand product)
        self.fold_qscale = os.environ.get("MAEST_FOLD_QSCALE", "1") != "0"
        self.persistent_gemm = os.environ.get("MAEST_PERSISTENT_GEMM", "1") != "0"      # see _gemm_form
        # "bf16x3" forwards that record no graph (the default evaluation mode): the three-term split product of the qkv / proj / fc1
        # linears runs as ONE bf16 GEMM over 3 K on the fast bf16 kernel -- LayerNorm and the attention forward write their fp32
        # results as [ hi | hi | lo ] bf16 rows (MAEST_SPLIT3_A), the weights are kept as [ hi | lo | hi ] rows (MAEST_SPLIT3_B):
        # the same three products per k as MAEST_F32X3, accumulated in fp32; the fc1 GEMM writes gelu(.) in that row form from its
        # epilogue (large M: the one-wave-per-SIMD kernel), so fc2 follows suit.  The last block's head-token rows (and small M) stay
        # on the per-chunk split kernels.  Same-box at configs[1]: profiles/r05_ab_x3_fast.txt
        self.x3_fast = os.environ.get("MAEST_X3_FAST", "1") != "0"
        # (A/B switches of the three engine-level choices above: MAEST_FOLD_QSCALE / MAEST_PERSISTENT_GEMM / MAEST_X3_FAST = 0 turn one off)
        # bf16 mode: residual adds ride in the LayerNorm that follows (True, see forward) or in the proj / fc2 GEMMs' fp32 RESIDUAL epilogue (False)
        # 1: both adds of a block in the LayerNorms; 0: both in GEMM epilogues; 2: proj's in norm2, fc2's in its epilogue.  Training forwards
        # (a graph is recorded) and evaluation forwards choose separately
        self.split_add = int(os.environ.get("MAEST_SPLIT_ADD", "1"))
        self.split_add_eval = int(os.environ.get("MAEST_SPLIT_ADD_EVAL", os.environ.get("MAEST_SPLIT_ADD", "1")))
        self._weights_dirty = False
        self._train_forwards = 0         # training-mode forwards so far: an operand-copy cache made before the latest one is stale (see _forward)
        # Training steps in flight: the host enqueues a step in ~10 ms, the GPU runs it in ~47, and nothing in a bare training loop makes
        # the host wait -- so it runs ahead, and blocks the caching allocator is asked for while their previous use (recorded on the side
        # stream) is still queued cannot be recycled: 60 unsynchronised steps took the reserved pool from 90 to 247 GB in 545 hipMallocs,
        # and a longer loop ends in an allocator retry (a multi-second stall).  The recording forward of step k therefore waits, on the
        # host, for the backward of step k - run_ahead to have finished on the device (MAEST_RUN_AHEAD, 0: unbounded).  Four steps
        # (~190 ms of queued work at batch 256) ride out a full Python garbage collection on the host (120 - 170 ms measured) without
        # a bubble on the device; the pool stays at ~1/4 of the unbounded loop's.
        self.run_ahead = int(os.environ.get("MAEST_RUN_AHEAD", "4"))
        # Weight gradients on the side stream run BESIDE the dgrad chain: launched half as wide as the kernel's own one-round plan (108 - 126
        # workgroups: 3 K splits for fc1 / fc2, 4 for qkv, 14 for proj) they leave the other CUs to the main stream's kernel, add a third
        # of the split-K atomics and run three times the K range per workgroup: -1.0 ... -2.1 % on the training step on three boxes; 64 / 96
        # make the wgrad the critical path (+40 % / +4 %), 160 / 192 equal the full width (profiles/r05e_step_level_ab.txt).
        # MAEST_WGRAD_WGS = 0: the kernel's plan.  Without the side stream (serialized passes) the plan is the kernel's.
        self.wgrad_wgs = int(os.environ.get("MAEST_WGRAD_WGS", "128"))
        self.bwd_gemm_wgs = int(os.environ.get("MAEST_BWD_GEMM_WGS", "256"))     # persistent workgroups of the dgrad GEMMs (A/B)
        # Data-parallel backward (a gradient sink is attached and exchanges buckets): RCCL's kernels hold a CU per channel while a bucket
        # is in flight, and a wgrad workgroup needs a WHOLE CU (512 registers per lane, 160 KiB of LDS) -- a plan wider than 256 - c
        # workgroups would run a second round for the c that found no CU.  The wgrad launches of such a pass are therefore at most
        # 256 - MAEST_WGRAD_RESERVE_CUS wide (default: NCCL_MAX_NCHANNELS if the job sets it, else 32); with the default 128-wide
        # side-stream launches this only binds serialized passes and MAEST_WGRAD_WGS = 0 / > 224.  Never measured on a multi-GPU box:
        # the knob exists so that the first one can tune it.
        self.wgrad_reserve_cus = max(0, min(192, int(os.environ.get("MAEST_WGRAD_RESERVE_CUS", os.environ.get("NCCL_MAX_NCHANNELS", "32")))))
        self._inflight = collections.deque()

    def throttle(self):
        """Host-side wait that bounds the number of training steps queued on the device (see run_ahead)."""
        if self.run_ahead > 0:
            while len(self._inflight) >= self.run_ahead:
                self._inflight.popleft().synchronize()

    def _step_done(self, dev):
        if self.run_ahead > 0 and dev.type == "cuda" and not torch.cuda.is_current_stream_capturing():
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            self._inflight.append(ev)
            while len(self._inflight) > 8:        # (backwards without forwards in between: keep the queue short)
                self._inflight.popleft()

    def _grad_layout(self):
        """{parameter name: (offset, numel)} into a flat fp32 gradient buffer, 256-byte aligned."""
        if getattr(self, "_layout", None) is None:
            off, lay = 0, {}
            for n, p in self.m.named_parameters():
                lay[n] = (off, p.numel())
                off += (p.numel() + 63) // 64 * 64
            self._layout = (lay, off)
        return self._layout

    def _side_stream(self, dev):
        return _engine_stream(dev, "side")

    def _eval_stream(self, dev):
        return _engine_stream(dev, "eval")

    def _comm_stream(self, dev):
        return _engine_stream(dev, "comm")

    def _gemm_form(self, shared: bool, wgs: int = 256):
        """The bf16 NT GEMM's launch form for a pass (csrc/gemm_nt_ow.hip): persistent -- one workgroup per CU walking its tiles, the next
        tile's first operand units requested from inside the epilogue -- and WITHOUT the second launch that runs the last partial round in
        128-row tiles, when nothing else wants CUs during the pass: +0.5 % (training step) ... +0.8 % (inference) for the persistent form,
        another +1.6 % / +0.4 % for dropping the 69 tail launches of a step (same-box, profiles/r05_ab_gemm_persistent.txt); one workgroup
        per tile and the tail tiles when the gradient all-reduce's kernels run beside it (`shared`: a fixed tile list per workgroup cannot
        be re-dealt around them).  Explicit MAEST_GEMM_WGS / MAEST_GEMM_TAIL settings (set_option) are left alone."""
        if not self.persistent_gemm or shared or ops.get_option("gemm_wgs") != 0:
            return contextlib.nullcontext()
        # (per-thread overrides: the forward thread and the autograd thread of ANOTHER model in this process keep their own form)
        return ops.thread_options(gemm_wgs=wgs, gemm_tail=0) if ops.get_option("gemm_tail") == 1 else ops.thread_options(gemm_wgs=wgs)

    @contextlib.contextmanager
    def _pass(self, f16, shared: bool = False, wgs: int = 256, deterministic: bool = False):
        """The settings of one pass as one context.  f16 (precision="fp16"): the same sequence of C-ABI calls, served by libmaest_hip_f16.so
        for this thread (maest_amd/_lib.py: flavour); then _gemm_form(shared, wgs); then, for a backward, _deterministic_form."""
        none = contextlib.nullcontext()
        with (ops._lib.flavour("f16") if f16 else none), self._gemm_form(shared, wgs), (self._deterministic_form() if deterministic else none):
            yield

    # ---- forward ----------------------------------------------------------------------------
    def forward(self, *args, f16: bool = False, **kw):
        with self._pass(f16):
            return self._forward(*args, f16=f16, **kw)

    def _forward(self, x3: torch.Tensor, dt, *, toffset: int, tok_ft: torch.Tensor, perm, lam, stripes=None,
                 stop_block: int = -1, return_self_attention: bool = False, save: bool = False, x3m=None, f16: bool = False, tap=None,
                 explain: bool = False, tap_x=None, full_last: bool = False, n_tok=None):
        """x3: fp32 [B, F, T] on the device; tok_ft: int32 [P, 2] kept patch tokens.  Returns (outputs, ctx).
        n_tok (ragged batches; only with a table per clip): int32 [B] on the device, clip b's real rows 2 + its kept tokens, the rest of
        its table MAEST_TOK_BLANK pads at the end -- handed to every block's attention (MAEST_ATTN_LENS), nothing else changes.
        x3m: split-bf16 products on the fp32 tensors (the model's resolved mode; None: model.precision == "bf16x3").
        tap (maest_amd/explain.py: the attention maps and the rollout): called as tap(i, qkv, (B, N, scale, x3m, qs)) right behind block
        i's qkv GEMM, with what an attention kernel needs to read that tensor; None: exactly the launches below.
        tap_x (maest_amd/hidden.py: the hidden states): called as tap_x(i, x) with block i's output stream -- fp32 [B * N, 768], which no later
        launch writes -- as soon as that tensor exists: behind the next block's first LayerNorm pass where that pass carries the fc2 add
        (`carry`), else behind block i's fc2 GEMM, for the last block of the pass behind the loop (there [B * 2, 768] when that block ran
        on the head rows); None: exactly the launches below.  full_last: the last block runs complete whatever head_tail says.
        explain (MAEST.attention_relevance, with save): the activations are kept for a backward that updates no weight -- the
        operand copies are cached as an evaluation forward caches them, and no dropout / drop-path is drawn (the step counter stays)."""
        recording = save and not explain      # a forward behind which an optimizer may step
        m, W = self.m, (self.w_f16 if f16 else self.w)
        if x3m is None:
            x3m = m.precision == "bf16x3"
        x3m = bool(x3m) and dt == torch.float32      # an explicit argument of every product
        gemm_nt = partial(ops.gemm_nt, x3=x3m)
        B, F, T = x3.shape
        clip_tokens = tok_ft.dim() == 3      # int32 [B, P, 2]: a table per clip (MAEST.forward_tokens; include/maest_hip.h: MAEST_IM2COL_CLIP_TOKENS)
        if clip_tokens:
            if save or tap is not None or tap_x is not None or stop_block >= 0:
                raise ValueError("a table of kept tokens per clip serves forwards that save nothing: no gradients, maps, pools or "
                                 "intermediate-block outputs (save, tap, tap_x, stop_block)")
            if tuple(tok_ft.shape[::2]) != (B, 2):
                raise ValueError(f"tok_ft of shape {tuple(tok_ft.shape)} for a batch of {B} clips: [B, P, 2] wanted")
        if n_tok is not None:
            if not clip_tokens:
                raise ValueError("token counts per clip (n_tok) go with a table of kept tokens per clip: tok_ft [B, P, 2]")
            if n_tok.dtype != torch.int32 or tuple(n_tok.shape) != (B,) or n_tok.device != x3.device:
                raise ValueError(f"n_tok must be an int32 tensor [{B}] on {x3.device}, got {n_tok.dtype} {tuple(n_tok.shape)} on {n_tok.device}")
        P = int(tok_ft.shape[-2])
        N = 2 + P
        M = B * N
        ctx = {"B": B, "N": N, "toffset": toffset, "tok_ft": tok_ft, "dt": dt, "x3m": x3m, "f16": bool(f16)} if save else None
        # Operand copies are keyed on the parameters' version counters, but FUSED optimizers (torch.optim.AdamW(...,
        # fused=True), multi-tensor kernels in general) update parameters in place WITHOUT bumping them -- a stale
        # bf16 copy then keeps training on the initial weights.  So every training-mode forward recasts everything
        # (one 0.24 ms launch for the 48 block matrices), and the first eval forward after one does too.
        if recording:
            self._train_forwards += 1
        if recording or W.seen_train != self._train_forwards:
            W.clear()
            # a cache a TRAINING forward fills is stale for every later forward (the optimizer steps behind it): -1 matches no count, so the
            # first forward after it -- evaluation or training -- recasts; a cache an evaluation forward fills serves until the next training one.
            # (Round 6 first stored the count here in both cases: an evaluation forward behind a fused-optimizer step then ran on the weights of
            # one step earlier -- bench.py's training cases showed it as deviation_vs_fp32 1e-2 instead of 2e-3.)
            W.seen_train = -1 if recording else self._train_forwards
        self._weights_dirty = bool(recording)
        mats = [lin.weight for blk in m.blocks for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)]
        mats += [m.patch_embed.proj.weight, m.head[1].weight]
        if m.distilled_type == "separated":
            mats.append(m.head_dist.weight)
        scale = m.blocks[0].attn.scale
        qs = bool(self.fold_qscale) and dt == torch.bfloat16
        want_rows = {id(blk.attn.qkv.weight): EMBED_DIM for blk in m.blocks} if qs else {}
        W.scaled_rows, W.row_scale = want_rows, scale * LOG2E      # (scaled and unscaled copies are cached under different keys)
        W.refresh(mats, dt, with_t=save)
        qkv_bias = [blk.attn.qkv.bias for blk in m.blocks]
        if qs and any(b is not None for b in qkv_bias):      # (qkv_bias=False models have no bias to scale)
            have = [b for b in qkv_bias if b is not None]
            scaled = iter(W.scaled_biases(have, EMBED_DIM))
            qkv_bias = [next(scaled) if b is not None else None for b in qkv_bias]
        fast3 = bool(self.x3_fast) and x3m and not save
        # dropout / stochastic depth (recording train() forwards with a rate > 0; None otherwise: exactly the launches below)
        plan = m._regulariser_plan() if recording else None
        reg = None
        if plan is not None:
            # (seed, step) of THIS forward, written on its stream; the state's step moves on in the same launch (csrc/regularise.hip)
            reg = dict(snap=ops.rng_advance(m._regulariser_state(x3.device)), p=plan[0], dpr=plan[1], pos_site=8 * len(m.blocks))
        if fast3:
            w3 = W.split3([lin.weight for blk in m.blocks for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)])
            w3 = {(i, n): w3[4 * i + j] for i in range(len(m.blocks)) for j, n in enumerate(("qkv", "proj", "fc1", "fc2"))}

        t_str, f_str = stripes if stripes is not None else (None, None)
        cols = ops.patch_im2col(x3, tok_ft, dt, perm=perm, lam=lam, t_stripes=t_str, f_stripes=f_str, stride=m.patch_embed.stride)
        patches = gemm_nt(cols, W.get(m.patch_embed.proj.weight, dt), m.patch_embed.proj.bias,
                              out_dtype=torch.float32)
        Tt = m.time_new_pos_embed.shape[-1]
        x = (ops.token_assemble_clips if clip_tokens else ops.token_assemble)(
            patches, m.cls_token.reshape(-1), m.dist_token.reshape(-1), m.new_pos_embed.reshape(2, EMBED_DIM),
            m.freq_new_pos_embed.reshape(EMBED_DIM, -1), m.time_new_pos_embed.reshape(EMBED_DIM, Tt), toffset, tok_ft, B)
        x = x.reshape(M, EMBED_DIM)
        if reg is not None and reg["p"] > 0:       # pos_drop (models/maest.py:800)
            ops.dropout_(x, None, B, N, N, reg["pos_site"], reg["p"], reg["snap"])
        if save:
            ctx["reg"] = reg
            ctx["cols"] = cols
            ctx["blocks"] = []
            ctx["qs"] = qs
            # what the input gradient (patch_im2col_bwd) needs: the forward's own operand-load options
            ctx.update(stop_block=stop_block, self_attention=bool(return_self_attention), x_shape=tuple(x3.shape), x_dtype=x3.dtype,
                       perm=perm, lam=lam, stripes=stripes, stride=tuple(m.patch_embed.stride))
        nblocks = len(m.blocks) if stop_block < 0 else stop_block + 1
        # bf16 perf mode: the proj / fc2 GEMMs emit their output (bias included) in bf16 and the residual add rides in
        # the LayerNorm that follows (ops.add_layernorm_fwd) -- the fp32 stream is read and rewritten by a streaming
        # kernel instead of a GEMM epilogue (proj: 196 -> ~100 us).  The reference rounds these Linear outputs to 16 bits
        # before the add as well (autocast, ex_maest.py:51).  fp32 modes keep the fused fp32 residual epilogue.
        # split_add_fc2: the same choice for the add behind the MLP (fc2 GEMM -> next block's norm1), separately: K = 3072 amortises an fp32
        # RESIDUAL epilogue better than proj's K = 768 does (profiles/r05_ab_split_add.txt)
        mode = self.split_add if save else self.split_add_eval
        split_add = dt != torch.float32 and mode in (1, 2)
        split_add_fc2 = dt != torch.float32 and mode == 1

        def norm(ln, x, add=None, out_dtype=dt, rows=N):
            """LayerNorm `ln` of the stream x -> (x, y, mean, rstd), the statistics None when nothing is saved.  add = (delta, sites): the
            delta of a residual branch joins the stream in the same pass -- x comes back as the new stream --, times the branch multiplier
            of sites = (elem, path) where the branch is regularised (rows: the rows of a clip in x)."""
            if add is None:
                r = ops.layernorm_fwd(x, ln.weight, ln.bias, ln.eps, out_dtype, save_stats=save)
                return (x, *r) if save else (x, r, None, None)
            delta, sites = add
            if sites is None:
                r = ops.add_layernorm_fwd(x, delta, ln.weight, ln.bias, ln.eps, dt, save_stats=save)
            else:
                r = ops.drop_add_layernorm_fwd(x, delta, ln.weight, ln.bias, ln.eps, dt, B, N, rows, *sites, reg["snap"], save_stats=save)
            return r if save else (*r, None, None)

        def linear(i, name, a, fast, **kw):
            """The GEMM of block i's linear `name` on a: fast -- the split path of "bf16x3" evaluation, a in MAEST_SPLIT3_A rows -- against the
            MAEST_SPLIT3_B copy of the weight as one bf16 GEMM over 3 K; else against the mode's operand copy, in the mode's product."""
            lin = getattr(m.blocks[i].attn if name in ("qkv", "proj") else m.blocks[i].mlp, name)
            bias = qkv_bias[i] if name == "qkv" else lin.bias
            if fast:
                return ops.gemm_nt(a, w3[(i, name)], bias, split3=True, **kw)
            return gemm_nt(a, W.get(lin.weight, dt), bias, **kw)

        carry = None              # what the previous block left for this block's norm1 to add: (delta of its fc2, its sites or None)
        for i in range(nblocks):
            blk = m.blocks[i]
            # The block's three choices, made here and carried out below.  (1) Is a branch regularised: br, its sites (a block with none
            # keeps the launches of an unregularised forward).  (2) Which operand copy the GEMMs take: `fast3` for norm1 -> qkv, which
            # always run on every row, `fast` for the rest of the block.  (3) Where the two residual adds ride: in the LayerNorm pass that
            # follows -- a regularised branch in every numeric mode: the GEMM emits its output with the bias-only epilogue and the add
            # rides there with the branch multiplier -- or in the GEMM's fp32 RESIDUAL epilogue.
            br = _block_sites(reg, i)
            tail = self.head_tail and not full_last and stop_block < 0 and i == nblocks - 1
            # (training needs the backward kernel that honours the restriction; otherwise the attention stays complete
            # and only the per-token part of the block is restricted)
            q_rows = HEAD_TOKENS if tail and (not save or ops.attn_bwd_rows_supported(dt, N)) else None
            attn_exit = i == stop_block and return_self_attention
            fast = fast3 and not tail and not attn_exit
            proj_add_in_norm2 = br is not None or split_add
            fc2_add_in_next_norm1 = i + 1 < nblocks and (br is not None or split_add_fc2)
            rpc = HEAD_TOKENS if tail else N      # rows of a clip in this block's per-token buffers

            # norm1 (this pass completes the previous block's output stream where it carries that block's fc2 add) -> qkv -> attention
            x, ln1, mean1, rstd1 = norm(blk.norm1, x, carry, out_dtype=ops.SPLIT3 if fast3 else dt)
            if tap_x is not None and carry is not None:
                tap_x(i - 1, x)
            carry = None
            qkv = linear(i, "qkv", ln1, fast3, out_dtype=torch.float32 if fast3 else dt)
            if tap is not None:      # (the qkv of the last block is complete even when the rest of it runs on the head rows)
                tap(i, qkv, (B, N, scale, x3m, qs))
            r = ops.attn_fwd(qkv, B, N, scale, save_lse=save, q_rows=q_rows, x3=x3m, q_prescaled=qs, out_split3=fast, n_tok=n_tok)
            ao, lse = r if save else (r, None)
            ao_full, x_full, Mb = ao, x, M
            if tail:      # from here on the block lives on [B * 2, 768]
                ao = ops.gather_head_rows(ao, B, N, HEAD_TOKENS)
                x = ops.gather_head_rows(x, B, N, HEAD_TOKENS)
                Mb = B * HEAD_TOKENS
            if save:      # (the rest of the block adds what it makes; the return_self_attention exit keeps this subset)
                s = dict(x=x_full, mean1=mean1, rstd1=rstd1, ln1=ln1, qkv=qkv, ao=ao, lse=lse, tail=tail, ao_full=ao_full, q_rows=q_rows,
                         reg=br, rpc=rpc)
                ctx["blocks"].append(s)
            if attn_exit:
                # Block.forward(..., return_self_attention=True) returns attn(norm1(x)) (maest.py:414-416); the backward of this block
                # starts at the proj GEMM: norm2 / MLP are not part of the output
                a = linear(i, "proj", ao, False, out_dtype=torch.float32)
                if br is not None and br["elem_a"] is not None:      # proj_drop is part of Attention.forward; drop-path is not
                    ops.dropout_(a, None, B, N, N, *br["elem_a"], reg["snap"])
                return ops.embed_pool(a.reshape(B, N, EMBED_DIM)), ctx

            # proj -> norm2
            if proj_add_in_norm2:
                d1 = linear(i, "proj", ao, False, out_dtype=dt)
                x1, ln2, mean2, rstd2 = norm(blk.norm2, x, (d1, None if br is None else (br["elem_a"], br["path_a"])), rows=rpc)
            else:
                x1 = linear(i, "proj", ao, fast, out_dtype=torch.float32, epi=ops.EPI_RESIDUAL, aux_in=x)
                x1, ln2, mean2, rstd2 = norm(blk.norm2, x1, out_dtype=ops.SPLIT3 if fast else dt)

            # fc1: on the fast path gelu(fc1) leaves the GEMM epilogue as [ hi | hi | lo ] rows where that epilogue is the fast one, and fc2
            # takes the 3 K bf16 GEMM as well (small M: an fp32 output and the per-chunk split kernel for fc2)
            H = blk.mlp.fc1.out_features
            h = torch.empty((Mb, H), dtype=dt, device=x.device) if save else None
            fast_fc2 = fast and ops.gemm_split3_out_fast(Mb, H, 3 * EMBED_DIM)
            g = linear(i, "fc1", ln2, fast, out_dtype=(ops.SPLIT3 if fast_fc2 else torch.float32) if fast else dt, epi=ops.EPI_GELU, aux_out=h)
            if br is not None and br["elem_h"] is not None:
                # Mlp.drop behind fc1 (models/maest.py:205), on gelu(.) and on the saved gelu'(.): the EPI_MUL dgrad then carries the mask
                ops.dropout_(g, h, B, N, rpc, *br["elem_h"], reg["snap"])
            if save:
                s.update(x1=x1, mean2=mean2, rstd2=rstd2, ln2=ln2, h=h, g=g)

            # fc2: its add rides in the next block's norm1, in the GEMM's epilogue, or -- a regularised last block of the pass, which
            # nothing follows that could carry it -- in a pass of its own
            if fc2_add_in_next_norm1:
                x, carry = x1, (linear(i, "fc2", g, False, out_dtype=dt), None if br is None else (br["elem_m"], br["path_m"]))
            elif br is not None:
                x = ops.drop_add(x1, linear(i, "fc2", g, False, out_dtype=dt), B, N, rpc, br["elem_m"], br["path_m"], reg["snap"])
            else:
                x = linear(i, "fc2", g, fast_fc2, out_dtype=torch.float32, epi=ops.EPI_RESIDUAL, aux_in=x1)
                if tap_x is not None and i + 1 < nblocks:
                    tap_x(i, x)
        if tap_x is not None:
            tap_x(nblocks - 1, x)
        xb = x.reshape(B, -1, EMBED_DIM)          # [B, N, 768], or [B, 2, 768] behind a restricted last block
        if stop_block >= 0:
            return ops.embed_pool(xb), ctx
        r = ops.head_pool_fwd(xb, m.norm.weight, m.norm.bias, m.norm.eps, save_stats=save)
        cls, dist, feat = r[:3]
        hn, hw = m.head[0], m.head[1]
        if m.distilled_type not in ("mean", "separated"):
            raise NotImplementedError(f"distilled_type={m.distilled_type!r}")
        # the head reads the features ("mean") or the cls token ("separated": the dist token goes through head_dist, a bare Linear)
        _, hl, hmean, hrstd = norm(hn, feat if m.distilled_type == "mean" else cls)
        logits = gemm_nt(hl, W.get(hw.weight, dt), hw.bias, out_dtype=torch.float32)
        if m.distilled_type == "mean":
            outs = (logits, feat)
        else:
            dlp = dist if dt == torch.float32 else ops.cast_weights(dist, dt)[0]
            logits_d = gemm_nt(dlp, W.get(m.head_dist.weight, dt), m.head_dist.bias, out_dtype=torch.float32)
            outs = (logits, logits_d, feat)
            if save:
                ctx["dist_lp"] = dlp
        if save:
            ctx.update(x_final=xb, fmean=r[3], frstd=r[4], cls=cls, dist=dist, feat=feat, hl=hl, hmean=hmean,
                       hrstd=hrstd)
        return outs, ctx

    # ---- backward ---------------------------------------------------------------------------
    def _deterministic_form(self):
        """The ordered gradient reductions for a pass, as a per-thread override like _gemm_form: two models in one process, one of them
        deterministic, never change each other's launches.  None (follow the library switch): nothing is set."""
        mode = self.m.deterministic_mode()
        return contextlib.nullcontext() if mode is None else ops.thread_options(deterministic=mode)

    def backward(self, ctx, grads_out, sink=None, *, weights: bool = True, first=None, tap=None):
        # (a forward recorded by libmaest_hip_f16.so holds IEEE half in its 16-bit tensors: its backward is that build's too)
        with self._pass(ctx.get("f16"), shared=sink is not None, wgs=self.bwd_gemm_wgs, deterministic=True):
            G = self._backward(ctx, grads_out, sink, weights, first, tap)
        if weights:
            self._step_done(ctx["cols"].device)
        return G

    def _backward(self, ctx, grads_out, sink=None, weights: bool = True, first=None, tap=None):
        """grads_out: gradients w.r.t. the forward outputs (same tuple structure, entries may be None).
        Returns {parameter name: fp32 gradient}, plus "_input": the gradient w.r.t. the forward's input x3 when
        ctx["want_dx"] asks for it.  With a `sink` (maest_amd.dist.GradReducer) every
        gradient is written straight into the sink's flat bucket view and reported as soon as it is
        complete, so the RCCL all-reduce of a bucket overlaps with the rest of the backward.
        A forward truncated at block k (ctx["stop_block"] = k: model(x, transformer_block=k)) starts from the backward of its
        embedding pool and runs the blocks k .. 0 and the embeddings only; parameters it does not reach get no gradient (with a
        sink: they are reported complete with their zeroed buffers, like DDP's find_unused_parameters=True).  Parameters that do
        not require grad get none either, and their weight-gradient GEMMs are not run.
        weights=False: the input-gradient chain alone, as if every parameter were frozen -- and no flat gradient buffer, no side stream;
        the LayerNorm kernels' gamma / beta sums land in one scratch buffer that is dropped.
        first: the chain returns right behind block `first`'s `dao`, before that block's attention backward; the activations of the
        blocks below are released unread and nothing of the embeddings runs.
        tap (maest_amd/explain.py: the relevance step): called as tap(i, saved activations of block i, dao) as soon as `dao` exists."""
        m, W = self.m, (self.w_f16 if ctx.get("f16") else self.w)
        x3m = ctx["x3m"]
        qs = ctx["qs"]
        gemm_nt = partial(ops.gemm_nt, x3=x3m)
        dt, B, N = ctx["dt"], ctx["B"], ctx["N"]
        Fp = m.freq_new_pos_embed.shape[2]
        M = B * N
        dev = ctx["cols"].device
        G = {}
        req = {n: weights and p.requires_grad for n, p in m.named_parameters()}
        stop = ctx.get("stop_block", -1)
        top = len(m.blocks) - 1 if stop < 0 else stop     # the last block the forward ran: where the chain starts
        attn_only = stop >= 0 and ctx.get("self_attention", False)      # ... of which only the attention branch

        # without a sink, all parameter gradients of this pass are views of ONE zero-filled flat buffer (one fill
        # kernel instead of ~160; the wgrad kernels accumulate into it with split-K atomics)
        flat, layout = None, None
        if sink is None and weights:
            layout, total = self._grad_layout()
            flat = torch.zeros(total, dtype=torch.float32, device=dev)
        assert first is None or not weights, "an early stop is served for the input-gradient chain alone (nothing waits for a side stream)"
        junk = None if weights else torch.zeros((2, EMBED_DIM), dtype=torch.float32, device=dev)      # gamma / beta sums nobody reads

        def buf(name, *shape):
            v = sink.grad_buffer(name) if sink is not None else None
            if v is not None:
                return v.view(*shape)          # zeroed by sink.reset()
            if layout is not None and name in layout:
                off, n = layout[name]
                return flat[off:off + n].view(*shape)
            return torch.zeros(*shape, dtype=torch.float32, device=dev)

        def norm_bufs(prefix):      # where a LayerNorm backward adds its gamma / beta gradients
            return (junk[0], junk[1]) if junk is not None else (buf(prefix + ".weight", EMBED_DIM), buf(prefix + ".bias", EMBED_DIM))

        # Weight / bias gradients are off the critical path (nothing in backward consumes them), so they run on
        # a SIDE HIP stream and overlap with the dgrad -> LayerNorm -> attention chain on the main stream: the
        # NT dgrad GEMMs are bound by their C-tile writes, the TN wgrad GEMMs by the MFMA pipe.
        side = self._side_stream(dev) if (weights and self.overlap_wgrad and dev.type == "cuda") else None
        main = torch.cuda.current_stream(dev) if side is not None else None

        def done(name, g):
            if not req.get(name, True):
                return               # frozen: its buffer may hold partial sums of a fused kernel, never reported as a gradient
            G[name] = g
            if sink is not None:
                b = sink.note_grad(name)          # host-side count; a bucket index when its last gradient has landed
                if b is None:
                    return
                if side is not None:
                    # The bucket's all-reduce must be ordered after BOTH streams (LayerNorm / embedding gradients come from
                    # the dgrad stream, weight gradients from the side stream).  A third stream waits for the two and
                    # issues it, ONCE PER BUCKET: neither producer stream is held up.  (Round 2 made the side stream wait
                    # for the main stream at every one of the 157 gradients, which locked the two streams together: the
                    # one-rank forced collective showed +3 ms per step with no RCCL kernel in the trace.)
                    comm = self._comm_stream(dev)
                    comm.wait_stream(main)
                    comm.wait_stream(side)
                    with torch.cuda.stream(comm):
                        sink.reduce_bucket(b, dedicated_stream=True)
                else:
                    sink.reduce_bucket(b)

        # launch width of this pass's wgrads (0 = the kernel's one-round plan of <= 256 workgroups)
        wg_w = self.wgrad_wgs if side is not None else 0
        if sink is not None and getattr(sink, "collective", False):
            wg_w = min(wg_w if wg_w > 0 else 256, 256 - self.wgrad_reserve_cus)

        def wgrad(name_w, name_b, dy, x, n_out, k_out, w_shape=None):
            if not (req.get(name_w, True) or req.get(name_b, True)):
                return
            gw, gb = buf(name_w, n_out, k_out), buf(name_b, n_out)
            if side is not None:
                ev = torch.cuda.Event()
                ev.record(main)            # dy, x and the zeroed destinations are ready at this point
                side.wait_event(ev)
                with torch.cuda.stream(side):
                    _wgrad(dy, x, n_out, k_out, gw, gb, x3m, wgs=wg_w)
                for t in (dy, x, gw, gb):
                    t.record_stream(side)  # keep the caching allocator from recycling them under the side stream
            else:
                _wgrad(dy, x, n_out, k_out, gw, gb, x3m, wgs=wg_w)
            done(name_w, gw if w_shape is None else gw.view(w_shape))
            done(name_b, gb)

        def norm_done(prefix, bufs):
            done(prefix + ".weight", bufs[0])
            done(prefix + ".bias", bufs[1])

        def ln_bwd(prefix, norm, dy, x, mean, rstd, dres, *, lp=True, head_tokens=None, bufs=None):
            """The backward of LayerNorm `prefix` -> (dx fp32, dx in the operand dtype: the same tensor in the fp32 modes, None without `lp`).
            Its gamma / beta sums land where norm_bufs says and are reported at once -- or in `bufs`, which the caller reports."""
            gw, gb = bufs or norm_bufs(prefix)
            dx, dx_lp = ops.layernorm_bwd(dy, x, norm.weight, mean, rstd, dres, gw, gb, lp_dtype=dt if lp and dt != torch.float32 else None,
                                          head_tokens=head_tokens)
            if bufs is None:
                norm_done(prefix, (gw, gb))
            return dx, (dx if lp and dt == torch.float32 else dx_lp)

        if stop >= 0:
            # truncated forward: the head, the final norm and the blocks above `stop` never ran -- nothing of theirs runs here
            if sink is not None:
                reached = {"cls_token", "dist_token", "new_pos_embed", "freq_new_pos_embed", "time_new_pos_embed",
                           "patch_embed.proj.weight", "patch_embed.proj.bias"}
                for n in req:
                    if n.startswith("blocks."):
                        i, rest = n.split(".", 2)[1:]
                        if int(i) < stop or (int(i) == stop and (not attn_only or rest.startswith(("norm1.", "attn.")))):
                            reached.add(n)
                for n, p in m.named_parameters():
                    if n not in reached:
                        done(n, buf(n, *p.shape))       # its zeroed bucket view: the bucket still completes and is reduced
            d_emb = grads_out[0] if isinstance(grads_out, (tuple, list)) else grads_out
            if d_emb is None:
                d_emb = torch.zeros((B, 3 * EMBED_DIM), dtype=torch.float32, device=dev)
            dx, dx_lp = ops.embed_pool_bwd(d_emb.float().contiguous(), N, lp_dtype=dt)
            if dx_lp is None:      # (the fp32 modes)
                dx_lp = dx
        else:
            C = m.head[1].out_features
            cpad = ops.round_up(C, 64)
            hn, hw = m.head[0], m.head[1]

            def head_linear_bwd(dlogits, inp_lp, lin, prefix, out_dtype):
                dl = ops.cast_rows(dlogits, dt, cpad)     # fp32 [B, C] -> operand dtype [B, cpad], zero padded (K of the dgrad GEMM)
                wgrad(prefix + ".weight", prefix + ".bias", dl, inp_lp, C, EMBED_DIM)
                wt = W.get(lin.weight, dt, transposed=True, pad_cols_to=64)          # [768, cpad]
                return gemm_nt(dl, wt, None, out_dtype=out_dtype, M=B, N=EMBED_DIM, K=cpad)

            # "mean": the head reads the features, whose own output gradient rides in its LayerNorm backward as the residual;
            # "separated": it reads the cls token, and head_dist the dist token
            sep = m.distilled_type != "mean"
            dlogits, dlogits_d, dfeat_out = grads_out if sep else (grads_out[0], None, grads_out[1])
            dfeat = None if dfeat_out is None else dfeat_out.contiguous()
            d_cls = d_dist = None
            h0 = norm_bufs("head.0")
            if dlogits is not None:
                dhl = head_linear_bwd(dlogits.contiguous(), ctx["hl"], hw, "head.1", dt)
                d, _ = ln_bwd("head.0", hn, dhl, ctx["cls" if sep else "feat"], ctx["hmean"], ctx["hrstd"], None if sep else dfeat,
                              lp=False, bufs=h0)
                d_cls, dfeat = (d, dfeat) if sep else (None, d)
            if dlogits_d is not None:
                # head_dist is a bare Linear: its input gradient feeds head_pool_bwd directly, in fp32
                d_dist = head_linear_bwd(dlogits_d.contiguous(), ctx["dist_lp"], m.head_dist, "head_dist", torch.float32)
            norm_done("head.0", h0)
            nb = norm_bufs("norm")
            dx = ops.head_pool_bwd(d_cls, d_dist, dfeat, ctx["x_final"], m.norm.weight, ctx["fmean"], ctx["frstd"], *nb).reshape(-1, EMBED_DIM)
            norm_done("norm", nb)
            dx_lp = dx if dt == torch.float32 else ops.cast_weights(dx, dt)[0]

        reg = ctx.get("reg")

        def enter(d32, d_lp, elem, path, rpc):
            """The gradient entering a residual branch: `d_lp` as it is, or -- the branch was regularised in the forward -- the stream's
            fp32 gradient times the forward's multiplier, in a buffer of its own (the stream's gradient passes on unmodified)."""
            if elem is None and path is None:
                return d_lp
            return ops.drop_cast(d32, dt, B, N, rpc, elem, path, reg["snap"])

        for i in reversed(range(top + 1)):
            blk, s = m.blocks[i], ctx["blocks"][i]
            p = f"blocks.{i}."
            H = blk.mlp.fc1.out_features
            br, rpc = s.get("reg"), s.get("rpc", N)
            if attn_only and i == top:
                # Block.forward(..., return_self_attention=True) = proj(attn(norm1 x)): no residual, no norm2 / MLP
                dx1, dx1_lp, dres1 = dx, dx_lp, None
                if br is not None:
                    dx1_lp = enter(dx, dx_lp, br["elem_a"], None, rpc)
            else:
                if br is not None:      # (before the wgrad's event: the side stream must see the masked operand)
                    dx_lp = enter(dx, dx_lp, br["elem_m"], br["path_m"], rpc)
                # fc2 (+ residual):  x2 = x1 + g W2^T + b2
                wgrad(p + "mlp.fc2.weight", p + "mlp.fc2.bias", dx_lp, s["g"], EMBED_DIM, H)
                dh = gemm_nt(dx_lp, W.get(blk.mlp.fc2.weight, dt, transposed=True), None, out_dtype=dt,
                                 epi=ops.EPI_MUL, aux_in=s["h"])
                # fc1
                wgrad(p + "mlp.fc1.weight", p + "mlp.fc1.bias", dh, s["ln2"], H, EMBED_DIM)
                dln2 = gemm_nt(dh, W.get(blk.mlp.fc1.weight, dt, transposed=True), None, out_dtype=dt)
                dx1, dx1_lp = ln_bwd(p + "norm2", blk.norm2, dln2, s["x1"], s["mean2"], s["rstd2"], dx)
                dres1 = dx1
                if br is not None:
                    dx1_lp = enter(dx1, dx1_lp, br["elem_a"], br["path_a"], rpc)
            # proj (+ residual)
            wgrad(p + "attn.proj.weight", p + "attn.proj.bias", dx1_lp, s["ao"], EMBED_DIM, EMBED_DIM)
            wt_proj = W.get(blk.attn.proj.weight, dt, transposed=True)
            below = first is None or i > first      # the chain goes on below this block's dao: its attention backward runs
            delta = None
            if s["tail"]:
                dao = gemm_nt(dx1_lp, wt_proj, None, out_dtype=dt)
                # back to the token-major layout: the head tokens' rows, zeros for the queries the kernel still visits
                # (its first 32-row tile when it honours q_rows, every row otherwise)
                dao = ops.scatter_head_rows(dao, B, N, HEAD_TOKENS, min(32, N) if s["q_rows"] else N)
            elif below and self.fold_delta:
                # delta = rowsum(dO * O) per (clip, head, query) out of the C-tile pass of the GEMM that produces dO
                dao, delta = ops.gemm_nt_rowdot(dx1_lp, wt_proj, s["ao_full"], N, out_dtype=dt, x3=x3m)
            else:
                dao = gemm_nt(dx1_lp, wt_proj, None, out_dtype=dt)
            if tap is not None:
                tap(i, s, dao)
            if not below:
                break
            # (delta given: the kernel does not read O; q_rows is set behind a head-rows block only)
            dqkv = ops.attn_bwd(s["qkv"], None if delta is not None else s["ao_full"], dao, s["lse"], B, N, blk.attn.scale, q_rows=s["q_rows"],
                                x3=x3m, delta=delta, q_prescaled=qs)
            wgrad(p + "attn.qkv.weight", p + "attn.qkv.bias", dqkv, s["ln1"], 3 * EMBED_DIM, EMBED_DIM)
            dln1 = gemm_nt(dqkv, W.get(blk.attn.qkv.weight, dt, transposed=True), None, out_dtype=dt)
            dx, dx_lp = ln_bwd(p + "norm1", blk.norm1, dln1, s["x"], s["mean1"], s["rstd1"], dres1,
                               head_tokens=(N, HEAD_TOKENS) if s["tail"] else None)
            s.clear()  # release this block's activations

        if first is not None:
            for s in ctx["blocks"]:
                s.clear()
            return G
        if reg is not None and reg["p"] > 0:      # pos_drop, on the gradient of the assembled tokens
            ops.dropout_(dx, None, B, N, N, reg["pos_site"], reg["p"], reg["snap"])
        Tt = m.time_new_pos_embed.shape[-1]
        d_cls_t, d_dist_t = buf("cls_token", EMBED_DIM), buf("dist_token", EMBED_DIM)
        d_np = buf("new_pos_embed", 2, EMBED_DIM)
        d_fp, d_tp = buf("freq_new_pos_embed", EMBED_DIM, Fp), buf("time_new_pos_embed", EMBED_DIM, Tt)
        dpatch = ops.token_assemble_bwd(dx, B, Fp, Tt, ctx["toffset"], ctx["tok_ft"], dt, d_cls_t, d_dist_t, d_np,
                                        d_fp, d_tp)
        done("cls_token", d_cls_t.view(1, 1, EMBED_DIM))
        done("dist_token", d_dist_t.view(1, 1, EMBED_DIM))
        done("new_pos_embed", d_np.view(1, 2, EMBED_DIM))
        done("freq_new_pos_embed", d_fp.view(1, EMBED_DIM, Fp, 1))
        done("time_new_pos_embed", d_tp.view(1, EMBED_DIM, 1, Tt))
        wgrad("patch_embed.proj.weight", "patch_embed.proj.bias", dpatch, ctx["cols"], EMBED_DIM, PATCH * PATCH,
              w_shape=m.patch_embed.proj.weight.shape)
        if ctx.get("want_dx"):
            # d x3 = col2im(dpatch W_patch): the [B*P, 768] x [768, 256] dgrad GEMM, then the gather back onto the mel samples
            # through the forward's own stride / kept tokens / SpecMasking stripes / mixup (csrc/embed.hip: col2im_kernel)
            dcols = gemm_nt(dpatch, W.get(m.patch_embed.proj.weight, dt, transposed=True), None, out_dtype=dt)
            t_str, f_str = ctx["stripes"] if ctx["stripes"] is not None else (None, None)
            G["_input"] = ops.patch_im2col_bwd(dcols, ctx["x_shape"], ctx["x_dtype"], ctx["tok_ft"], perm=ctx["perm"], lam=ctx["lam"],
                                               t_stripes=t_str, f_stripes=f_str, stride=ctx["stride"])
        if side is not None:
            main.wait_stream(side)        # gradients are complete before backward returns to autograd / the optimizer
        return G


class _GraphLease:
    """Held by the autograd node of a forward that was replayed from a captured training graph, until its backward has
    run (or the node is dropped): while it is alive the graph's static activation buffers must not be rewritten."""
    __slots__ = ("__weakref__",)


class _MaestFn(torch.autograd.Function):
    """The single autograd edge: forward = _Engine.forward(save=True); backward = _Engine.backward.  Its outputs: the forward's
    tuple, or the one embedding tensor of a forward truncated at a block (kw["stop_block"] >= 0).  x3 gets a gradient when it
    requires one (saliency, input attribution)."""

    @staticmethod
    def forward(ctx, model, x3, dt, kw, names, *params):
        ctx.set_materialize_grads(False)      # outputs the loss does not use (the features) arrive as None, not as zeros
        ctx.graph_lease = None
        if x3.is_cuda:
            model._engine.throttle()
        # (the captured training forward exists for the bf16 build only, and for the full forward of an input that needs no gradient)
        if (model.hip_graph and x3.is_cuda and not kw.get("f16") and kw.get("stop_block", -1) < 0
                and not x3.requires_grad):
            outs, saved, ctx.graph_lease = model._graph_train_forward(x3, dt, kw)
        else:
            outs, saved = model._engine.forward(x3, dt, save=True, **kw)
        ctx.saved = saved
        ctx.model = model
        ctx.names = names
        return outs

    @staticmethod
    def backward(ctx, *gout):
        if ctx.saved is None:
            raise RuntimeError("maest_amd: backward called twice (activations are released after the first pass)")
        sink = ctx.model._grad_sink
        ctx.saved["want_dx"] = ctx.needs_input_grad[1]
        G = ctx.model._engine.backward(ctx.saved, gout, sink)
        ctx.saved = None
        ctx.graph_lease = None       # the graph's static activation buffers may be rewritten again
        dx = G.pop("_input", None)
        if sink is not None:   # the sink (maest_amd.dist.GradReducer) installs param.grad itself
            return (None, dx, None, None, None, *([None] * len(ctx.names)))
        grads = []
        for n, p in zip(ctx.names, ctx.model._param_list):
            g = G.get(n)
            if g is not None and g.shape != p.shape:
                g = g.reshape(p.shape)
            grads.append(g)
        return (None, dx, None, None, None, *grads)


def _check_rates(drop_rate, attn_drop_rate, drop_path_rate):
    for name, v in (("drop_rate", drop_rate), ("attn_drop_rate", attn_drop_rate), ("drop_path_rate", drop_path_rate)):
        if not 0.0 <= float(v) < 1.0:
            raise ValueError(f"{name} must lie in [0, 1), got {v!r}")
    if float(attn_drop_rate) > 0.0:
        raise NotImplementedError("attn_drop_rate > 0: dropout on the attention probabilities inside the fused attention kernels is "
                                  "not built (drop_rate and drop_path_rate are)")


def _check_deterministic(value):
    if value is not None and not isinstance(value, bool):
        raise ValueError(f"deterministic must be None (follow torch.use_deterministic_algorithms / MAEST_DETERMINISTIC), True or False, "
                         f"got {value!r}")


def regulariser_seed(initial_seed: int, rank: int = 0) -> int:
    """The 64-bit mask seed a model derives when none was set: a pure function of torch.initial_seed() and the process's rank in the
    default process group, so that data-parallel ranks that share a torch seed do not share masks (splitmix64 finaliser of
    initial_seed + (rank + 1) * the 64-bit golden ratio)."""
    m = 0xFFFFFFFFFFFFFFFF
    z = (int(initial_seed) + (int(rank) + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


class MAEST(nn.Module):
    """Music Audio Efficient Spectrogram Transformer (reference class: models/maest.py:423-939)."""

    def __init__(self, u_patchout=0, s_patchout_t=0, s_patchout_f=0, s_patchout_f_indices=(),
                 s_patchout_f_interleaved=0, s_patchout_t_indices=(), s_patchout_t_interleaved=0,
                 img_size=(96, 625), patch_size=16, stride=10, in_chans=1, num_classes=400, embed_dim=768,
                 depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True, distilled=True, distilled_type="mean",
                 precision="auto", drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, *, deterministic=None,
                 _skip_init: bool = False):
        super().__init__()
        _check_rates(drop_rate, attn_drop_rate, drop_path_rate)
        _check_deterministic(deterministic)
        self._skip_init = bool(_skip_init)      # clone_weights(): the twin's parameters are copies, not draws
        self._init_kwargs = dict(u_patchout=u_patchout, s_patchout_t=s_patchout_t, s_patchout_f=s_patchout_f,
                                 s_patchout_f_indices=s_patchout_f_indices,
                                 s_patchout_f_interleaved=s_patchout_f_interleaved,
                                 s_patchout_t_indices=s_patchout_t_indices,
                                 s_patchout_t_interleaved=s_patchout_t_interleaved, img_size=tuple(img_size),
                                 patch_size=patch_size, stride=stride, in_chans=in_chans, num_classes=num_classes,
                                 embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                 qkv_bias=qkv_bias, distilled=distilled, distilled_type=distilled_type,
                                 precision=precision, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate,
                                 drop_path_rate=drop_path_rate, deterministic=deterministic)
        if embed_dim != EMBED_DIM or num_heads != NUM_HEADS or patch_size != PATCH or in_chans != 1:
            raise NotImplementedError("maest_amd kernels are specialised for the MAEST geometry: "
                                      "embed_dim=768, 12 heads x 64, 16x16 patches, mono input")
        if not distilled:
            raise NotImplementedError("every MAEST architecture is DeiT-distilled (cls + dist tokens)")
        self.num_classes = num_classes
        self.u_patchout = u_patchout
        self.img_size = tuple(img_size)
        self.s_patchout_t = s_patchout_t
        self.s_patchout_f = s_patchout_f
        self.s_patchout_f_indices = s_patchout_f_indices
        self.s_patchout_f_interleaved = s_patchout_f_interleaved
        self.s_patchout_t_indices = s_patchout_t_indices
        self.s_patchout_t_interleaved = s_patchout_t_interleaved
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 2
        self.distilled_type = distilled_type
        self.precision = precision
        # regularisers of the training step (models/maest.py:452-454): plain attributes, read at every recording train() forward
        self.drop_rate = float(drop_rate)
        self.attn_drop_rate = float(attn_drop_rate)
        self.drop_path_rate = float(drop_path_rate)
        # Bit-reproducible backward (include/maest_hip.h: MAEST_OPT_DETERMINISTIC): a plain attribute, read at every backward.  None follows
        # torch.are_deterministic_algorithms_enabled() or the library switch (ops.set_option("deterministic", 1) / MAEST_DETERMINISTIC=1);
        # True / False override both for this model's passes.
        self.deterministic = deterministic
        self._reg_seed = None        # set_regulariser_seed(), else derived at the first regularised forward
        self._reg_state = {}         # {device: int32 [4] = seed lo, seed hi, step, 0} (include/maest_hip.h), not a registered buffer
        if num_classes == 400:
            self.labels = discogs_400labels
        elif num_classes == 519:
            self.labels = discogs_519labels

        stride = tuple(stride) if isinstance(stride, (tuple, list)) else (stride, stride)
        self.patch_embed = PatchEmbed(img_size=self.img_size, patch_size=patch_size, stride=stride,
                                      in_chans=in_chans, embed_dim=embed_dim)
        self.num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.dist_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.new_pos_embed = nn.Parameter(torch.zeros(1, self.num_tokens, embed_dim))
        self.freq_new_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, self.patch_embed.grid_size[0], 1))
        self.time_new_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, 1, self.patch_embed.grid_size[1]))
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, mlp_ratio, qkv_bias, eps=1e-6)
                                      for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.pre_logits = nn.Identity()
        self.head = nn.Sequential(nn.LayerNorm(self.num_features),
                                  nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity())
        self.head_dist = nn.Linear(self.embed_dim, self.num_classes) if num_classes > 0 else nn.Identity()
        self.init_weights()
        self.melspectrogram = MelSpectrogram()
        self._engine = _Engine(self)
        self._param_names = None
        self._tok_cache = {}
        self.hip_graph = False
        self.eval_streams = int(os.environ.get("MAEST_EVAL_STREAMS", "2"))     # see _eval_forward
        self._toffset_choices = 1
        self._graphs = {}
        self._param_list = None
        self._grad_sink = None   # set to a maest_amd.dist.GradReducer for data-parallel training

    def clone_weights(self) -> "MAEST":
        """A fresh model of the same architecture, on the same device and in the same mode, holding copies of the
        parameters -- and NOTHING of the engine's run-time state (operand-copy caches keyed on the old parameters,
        side streams, captured HIP graphs, the data-parallel gradient sink with its flat buffer)."""
        twin = type(self)(**self._init_kwargs, _skip_init=True)     # every parameter is overwritten below
        # configuration changed after construction travels too (patchout switched off for evaluation, numeric mode, engine
        # switches) -- run-time state does not, and neither does graph replay: a twin (SWA average, teacher) captures graphs,
        # with their private memory pools, only when its owner calls enable_hip_graph() on it
        for k in ("precision", "drop_rate", "attn_drop_rate", "drop_path_rate", "deterministic", "u_patchout", "s_patchout_t", "s_patchout_f", "s_patchout_f_indices",
                  "s_patchout_f_interleaved", "s_patchout_t_indices", "s_patchout_t_interleaved"):
            setattr(twin, k, getattr(self, k))
        twin._engine.head_tail = self._engine.head_tail
        twin._engine.overlap_wgrad = self._engine.overlap_wgrad
        twin._reg_seed = self._reg_seed      # (the twin's step counter starts at 0 on its own device state)
        dev = next(self.parameters()).device
        twin.to(dev)
        with torch.no_grad():
            for a, b in zip(twin.parameters(), self.parameters()):
                a.copy_(b)
                a.requires_grad_(b.requires_grad)
        twin.train(self.training)
        return twin

    def __deepcopy__(self, memo):
        # copy.deepcopy of a live model (Lightning's StochasticWeightAveraging does exactly that, helpers/
        # swa_callback.py:9-44) must not drag CUDA graphs, streams, process groups or 344 MB gradient buckets along
        twin = self.clone_weights()
        memo[id(self)] = twin
        return twin

    # ---- bit-reproducible training ---------------------------------------------------------------
    def deterministic_mode(self):
        """What this model's backward passes run with: None = the library switch as it stands (self.deterministic is None and torch's
        deterministic-algorithms flag is off), else 1 / 0 = a per-thread override for the pass.  Scope of the guarantee:
        one process on one GPU, the same build, shapes and option values."""
        _check_deterministic(self.deterministic)
        if self.deterministic is None:
            return 1 if torch.are_deterministic_algorithms_enabled() else None
        return 1 if self.deterministic else 0

    @property
    def is_deterministic(self) -> bool:
        """Whether a backward of this model, launched now from this thread, runs the ordered gradient reductions."""
        mode = self.deterministic_mode()
        return bool(ops.get_option("deterministic")) if mode is None else bool(mode)

    # ---- regularisers: dropout and stochastic depth ----------------------------------------------
    @property
    def drop_path_rates(self):
        """Drop-path rate of every block: linspace(0, drop_path_rate, depth), as the reference computes it (models/maest.py:534-536)."""
        return [float(v) for v in torch.linspace(0, self.drop_path_rate, len(self.blocks))]

    def set_regulariser_seed(self, seed: int):
        """Seed of the dropout / drop-path masks (include/maest_hip.h: the Philox key); the step counter restarts at 0.  Without a call
        the seed is regulariser_seed(torch.initial_seed(), rank), taken once at the first regularised forward."""
        self._reg_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for dev, st in self._reg_state.items():      # in place: a captured training graph holds this buffer
            st.copy_(ops.rng_state(self._reg_seed, "cpu"))
        return self

    def _regulariser_state(self, dev):
        st = self._reg_state.get(str(dev))
        if st is None:
            if self._reg_seed is None:
                import torch.distributed as dist
                rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
                self._reg_seed = regulariser_seed(torch.initial_seed(), rank)
            st = self._reg_state[str(dev)] = ops.rng_state(self._reg_seed, dev)
        return st

    def _regulariser_plan(self):
        """What a recording train() forward applies: None (every rate 0: today's launches), else (drop_rate, per-block drop-path rates)."""
        _check_rates(self.drop_rate, self.attn_drop_rate, self.drop_path_rate)
        if not self.training or (self.drop_rate == 0.0 and self.drop_path_rate == 0.0):
            return None
        return float(self.drop_rate), self.drop_path_rates

    # ---- reference API odds and ends --------------------------------------------------------
    def init_weights(self, mode=""):
        assert mode in ("jax", "jax_nlhb", "nlhb", "")
        if self._skip_init:
            return
        for p in (self.new_pos_embed, self.freq_new_pos_embed, self.time_new_pos_embed, self.dist_token,
                  self.cls_token):
            nn.init.trunc_normal_(p, std=0.02, a=-2.0, b=2.0)
        self.apply(_init_vit_weights)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"new_pos_embed", "freq_new_pos_embed", "time_new_pos_embed", "cls_token", "dist_token"}

    def get_classifier(self):
        return self.head, self.head_dist

    def _resolve_precision(self, recording: bool = True) -> str:
        """The numeric mode a forward runs in: "bf16", "bf16x3" or "fp32"."""
        p = self.precision
        if p == "auto":
            # bf16 is the TRAINING mode (the reference trains under 16-bit autocast, ex_maest.py:51); any forward
            # that records no graph -- eval(), no_grad, predict_labels on a fresh train-mode model -- is inference,
            # which the reference computes in fp32: here the split-bf16 products on fp32 tensors, which meet the same
            # 1e-3 / identical-ranking gates as the exact fp32 MFMAs (fixture G1: 1.9e-6 against 1.4e-6) at twice their
            # speed; precision="fp32" selects the exact products
            p = "bf16" if (self.training and recording) else "bf16x3"
        if p in ("fp32", "float32"):
            return "fp32"
        if p == "bf16x3":
            return "bf16x3"
        if p in ("bf16", "bfloat16"):
            return "bf16"
        if p in ("fp16", "float16", "half"):
            # IEEE half operands: the bf16 kernels' schedules on v_mfma_*_f16 (libmaest_hip_f16.so: the same sources, csrc/common.h
            # MAEST_16BIT_F16) -- the reference's own GPU arithmetic (16-mixed autocast, ex_maest.py:51), 6e-4 .. 8e-4 from fp32 where bf16 is at
            # 5e-3 .. 8e-3, at the bf16 mode's speed.  A train() forward records the graph in half as well, like the reference's autocast:
            # gradients in half underflow without LOSS SCALING (torch.amp.GradScaler, which the reference's trainer applies under 16-mixed;
            # Module.training_step leaves that to the loop as the reference's does) -- eval() forwards never record in this mode.
            return "fp16"
        raise ValueError(f"precision must be 'auto', 'fp32', 'bf16x3', 'bf16' or 'fp16', got {self.precision!r}")

    def _compute_dtype(self, recording: bool = True):
        # ("fp16": the kernels' 16-bit container carries the bfloat16 dtype TAG; the half-precision build interprets the bits)
        return torch.bfloat16 if self._resolve_precision(recording) in ("bf16", "fp16") else torch.float32

    # ---- input handling (maest.py:855-895) --------------------------------------------------
    def _prepare_input(self, x, melspectrogram_input):
        assert isinstance(x, torch.Tensor), "Input must be a torch.Tensor"
        assert x.nelement() > 0, "Input tensor must not be empty"
        if len(x.shape) == 1:
            assert melspectrogram_input is False, (
                "Input is 1D, but melspectrogram_input is True. This is not supported.")
            self._check_audio_len(x.shape[-1], chunked=True)
            x = self.melspectrogram(x)
            if x.shape[1] >= self.img_size[1]:
                trim = x.shape[1] % self.img_size[1]
                if trim:
                    x = x[:, :-trim]
                x = x.reshape(self.img_size[0], 1, -1, self.img_size[1])
                x = torch.swapaxes(x, 0, 2)
            else:
                x = x.reshape(1, 1, x.shape[0], x.shape[1])
        elif len(x.shape) == 2 and melspectrogram_input:
            trim = x.shape[1] % self.img_size[1]
            if trim:
                x = x[:, :-trim]
            x = x.reshape(self.img_size[0], 1, -1, self.img_size[1])
            x = torch.swapaxes(x, 0, 2)
        elif len(x.shape) == 2 and not melspectrogram_input:
            self._check_audio_len(x.shape[-1], chunked=False)
            x = self.melspectrogram(x)
            x.unsqueeze_(1)
        elif len(x.shape) == 3:
            x.unsqueeze_(1)  # in place, like the reference (maest.py:895): the caller's tensor becomes 4-D
        return x

    def _check_patches_fit(self, T):
        Tp = (T - PATCH) // self.patch_embed.stride[1] + 1
        table = self.time_new_pos_embed.shape[-1]
        if Tp > table:
            raise Exception(
                f"the patches shape:{(EMBED_DIM, self.patch_embed.grid_size[0], Tp)} are larger than the expected "
                f"time encodings {tuple(self.time_new_pos_embed.shape)}, please reduce the input duration.")
        return Tp

    def _check_audio_len(self, S, chunked):
        # Same exception the reference raises from forward_features (maest.py:664-668), detected before
        # any device work: un-chunked audio whose mel is longer than the time positional table.
        if not chunked:
            self._check_patches_fit(1 + S // MelSpectrogram.hop_len)

    def _resolve_tokens(self, Fp, Tp, pinned=None):
        """Every patchout variant of the reference (maest.py:645-657, 678-780) resolved on the host into
        (toffset, kept patch tokens [P, 2] = (f, t) in sequence order).  RNG: the reference's generator
        calls in the reference's order -- randint (time-table offset), randperm(T') (s_patchout_t),
        randperm(F') (s_patchout_f), ..., randperm(seq) (u_patchout) -- so a shared torch.manual_seed
        reproduces the reference's draws.  `pinned = (toffset, t_keep)` overrides the two training draws."""
        table = self.time_new_pos_embed.shape[-1]
        f_list = torch.arange(Fp)
        t_list = torch.arange(Tp)
        toffset = 0
        if pinned is not None:
            toffset, t_keep = pinned
            # the reference slices time_new_pos_embed[..., toffset:toffset + T'] (maest.py:648-657): an offset that does
            # not leave T' columns makes its broadcast add fail; here it would read past the table in the kernel
            if not 0 <= int(toffset) <= table - Tp:
                raise ValueError(f"patchout offset {toffset} outside 0..{table - Tp} (time table {table}, {Tp} time patches)")
            if t_keep is not None:
                t_list = torch.as_tensor(t_keep, dtype=torch.long).cpu()
                if t_list.numel() and (int(t_list.min()) < 0 or int(t_list.max()) >= Tp):
                    raise ValueError(f"kept time columns must lie in 0..{Tp - 1}")
        elif self.training:
            toffset = torch.randint(1 + table - Tp, (1,)).item()
            if self.s_patchout_t:
                t_list = t_list[torch.randperm(Tp)[: Tp - self.s_patchout_t].sort().values]
        if self.training and self.s_patchout_f:
            f_list = f_list[torch.randperm(Fp)[: Fp - self.s_patchout_f].sort().values]
        if self.s_patchout_f_indices:
            pos = torch.arange(len(f_list))
            for i in self.s_patchout_f_indices:
                pos = pos[pos != int(i)]
            f_list = f_list[pos]
        if self.s_patchout_f_interleaved:
            f_list = f_list[torch.arange(0, len(f_list), self.s_patchout_f_interleaved)]
        if self.s_patchout_t_indices:
            pos = torch.arange(len(t_list))
            for i in self.s_patchout_t_indices:
                pos = pos[pos != int(i)]
            t_list = t_list[pos]
        if self.s_patchout_t_interleaved:
            t_list = t_list[torch.arange(0, len(t_list), self.s_patchout_t_interleaved)]
        tok = torch.stack(torch.meshgrid(f_list, t_list, indexing="ij"), dim=-1).reshape(-1, 2)   # f-major (maest.py:769)
        if self.training and self.u_patchout:
            seq_len = tok.shape[0]
            tok = tok[torch.randperm(seq_len)[: seq_len - self.u_patchout].sort().values]
        return int(toffset), tok.to(torch.int32).contiguous()

    # ---- forward ----------------------------------------------------------------------------
    def forward(self, x, transformer_block: int = -1, return_self_attention: bool = False,
                melspectrogram_input: bool = False, *, _mixup=None, _patchout=None, _specmask=None
                ) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """Same contract as the reference's ``MAEST.forward`` (maest.py:831-933).

        ``_mixup=(perm, lam)``, ``_specmask=(t_stripes, f_stripes)`` and ``_patchout=(toffset, kept_time_columns)``
        are private hooks used by ``maest_amd.module.Module.training_step`` (mixup and SpecMasking fused into the
        patch-embedding operand load) and by the parity tests (pinned draws)."""
        x3, dt, kw, need_grad, _ = self._resolve_call(x, melspectrogram_input, _mixup, _patchout, _specmask)
        return self._run(x3, dt, kw, need_grad, transformer_block, return_self_attention,
                         plain=_mixup is None and _patchout is None and _specmask is None)

    def _resolve_call(self, x, melspectrogram_input, _mixup, _patchout, _specmask, recording=None):
        """What a forward call resolves before it launches anything: the rank dispatch, the shape checks, the numeric mode, the kept
        tokens and the private hooks -> (x3 [B, F, T] on the device, compute dtype, the engine's keyword arguments, whether a graph is
        recorded, (F', T') of the patch grid).  recording=False (attention_maps): never record, whatever grad mode says; "always"
        (attention_relevance): the mode of a recording forward of the current train() / eval() state, whatever grad mode says."""
        x = self._prepare_input(x, melspectrogram_input)
        if x.dim() != 4 or x.shape[1] != 1:
            raise Exception(f"expected input of shape [B, 1, F, T], got {tuple(x.shape)}")
        B, _, F, T = x.shape
        Tp = self._check_patches_fit(T)
        Fp = (F - PATCH) // self.patch_embed.stride[0] + 1
        Fg = self.freq_new_pos_embed.shape[2]
        if Fp != Fg:
            # the reference adds the whole frequency table to the patch grid (models/maest.py:676: x + self.freq_new_pos_embed), which
            # broadcasts only when the two agree: torch's error, raised before any device work.  (PatchEmbed.grid_size is img // stride,
            # models/maest.py:234, the convolution yields (F - 16) // stride + 1 rows: at 96 bands they agree for strides 10, 11, 13 .. 16.)
            raise RuntimeError(f"The size of tensor a ({Fp}) must match the size of tensor b ({Fg}) at non-singleton dimension 2")
        if not x.is_cuda and not ops._lib.host_emulation():
            raise ops._lib.MaestHipError(
                f"maest_amd runs on MI355X only: input is on {x.device}. Move the model and the input to a HIP "
                "device (model.cuda(); x.cuda()). There is no CPU fallback.")
        x3 = x.reshape(B, F, T)
        if x3.dtype not in (torch.float32, torch.float16):   # float16 batches (the loader's, discogs/dataset.py:58-67) go
            x3 = x3.float()                                  # straight into the patch-embedding operand load
        x3 = x3.contiguous()
        # a graph is recorded when grad mode is on and a parameter or the input requires grad -- for the full forward and for the
        # embedding of block k alike (the reference's forward_features is ordinary autograd, models/maest.py:808-829)
        need_grad = (recording is not False and torch.is_grad_enabled()
                     and (x3.requires_grad or any(p.requires_grad for p in self.parameters())))
        if recording == "always":
            need_grad = True      # (an explicit call: precision="fp16" runs in half in eval() too)
        elif need_grad and not self.training and self.precision in ("fp16", "float16", "half"):
            need_grad = False     # precision="fp16": eval() forwards record no graph even outside no_grad (a backward through them fails loudly
                                  # on outputs that do not require grad); a train() forward records in half and wants a scaled loss (_resolve_precision)
        dt = self._compute_dtype(need_grad)

        tok_key = (Fp, Tp, str(x3.device))
        # how many time-table offsets this call could have drawn (1: none drawn / pinned); the train-graph cache looks at it
        self._toffset_choices = (1 + self.time_new_pos_embed.shape[-1] - Tp) if (self.training and _patchout is None) else 1
        if not self.training and _patchout is None and tok_key in self._tok_cache:
            toffset, tok_ft = self._tok_cache[tok_key]        # eval: deterministic, already on the device
        else:
            toffset, tok_ft = self._resolve_tokens(Fp, Tp, _patchout)
            if tok_ft.shape[0] < 1:
                raise Exception("patchout removed every patch token")
            if x3.is_cuda and not tok_ft.is_cuda:     # training: a fresh list every step; no stream-draining copy
                # (asynchronous copy out of a pinned block; torch's caching host allocator holds the block back until the
                # copy's stream event has completed)
                tok_ft = tok_ft.contiguous().pin_memory().to(x3.device, non_blocking=True)
            else:
                tok_ft = tok_ft.to(x3.device)
            if not self.training and _patchout is None:
                self._tok_cache[tok_key] = (toffset, tok_ft)
        perm = lam = None
        if _mixup is not None:
            perm, lam = _mixup
            perm = perm.to(device=x3.device, dtype=torch.int32).contiguous()
            lam = lam.to(device=x3.device, dtype=torch.float32).contiguous()
        stripes = None
        if _specmask is not None:
            stripes = tuple(None if t is None else t.to(device=x3.device, dtype=torch.int32).contiguous()
                            for t in _specmask)
        mode = self._resolve_precision(need_grad)
        kw = dict(toffset=int(toffset), tok_ft=tok_ft, perm=perm, lam=lam, stripes=stripes, x3m=mode == "bf16x3")
        if mode == "fp16":
            kw["f16"] = True
        return x3, dt, kw, need_grad, (Fp, Tp)

    def _run(self, x3, dt, kw, need_grad, transformer_block, return_self_attention, plain):
        """The launches of a resolved forward call.  plain: no private hook is set (the HIP-graph replay serves such calls only)."""
        if need_grad and self._param_names is None:
            named = list(self.named_parameters())
            self._param_names = [n for n, _ in named]
            self._param_list = [p for _, p in named]
        if transformer_block != -1:
            if need_grad:
                kw.update(stop_block=transformer_block, return_self_attention=return_self_attention)
                return None, _MaestFn.apply(self, x3, dt, kw, self._param_names, *self._param_list)
            with torch.no_grad():
                emb, _ = self._engine.forward(x3, dt, stop_block=transformer_block,
                                              return_self_attention=return_self_attention, **kw)
            return None, emb

        if need_grad:
            outs = _MaestFn.apply(self, x3, dt, kw, self._param_names, *self._param_list)
        else:
            with torch.no_grad():
                if self.hip_graph and x3.is_cuda and not self.training and plain:
                    outs = self._graph_forward(x3, dt, kw)
                else:
                    outs = self._eval_forward(x3, dt, kw)
        return outs

    # Rows of a batch (clips x tokens) from which an eager evaluation forward runs as two half batches on two streams (below, ~1.5 rounds of
    # 256 x 256 tiles per half at N = 768, the split costs more launches than its tails give back)
    EVAL_SPLIT_ROWS = 98304

    def _eval_forward(self, x3, dt, kw):
        """Eager evaluation forward.  A large batch runs as TWO HALF BATCHES ON TWO STREAMS: every kernel of the forward is per clip or per
        token, so the halves are independent and their results are the full batch's, bit for bit; what the second stream buys is the tail of
        every persistent GEMM launch -- 1680 tiles of 256 x 256 over 256 CUs are 6.56 rounds, the seventh runs on 144 CUs (proj / fc2 at 256
        clips x 560 tokens; 3.9 % of the GEMM time over the four linears) -- which the other half's kernels now fill: -2.0 ... -3.3 % on the
        inference pass in every numeric mode (profiles/r06_eval_two_streams.txt).  MAEST_EVAL_STREAMS = 1 (or model.eval_streams = 1): one
        stream.  The first half runs on the caller's stream; the second starts beside it when the operand copies of the weights are warm, and
        behind it when this very forward had to rebuild them (they are made on the caller's stream)."""
        eng = self._engine
        B = x3.shape[0]
        tok = kw["tok_ft"]
        rows = B * (2 + int(tok.shape[-2]))      # ([P, 2], or a table per clip [B, P, 2]: each half gets its own clips' rows, below)
        if (self.eval_streams < 2 or not x3.is_cuda or B < 2 or rows < self.EVAL_SPLIT_ROWS or kw.get("perm") is not None
                or kw.get("stripes") is not None or torch.cuda.is_current_stream_capturing()):
            return eng.forward(x3, dt, **kw)[0]
        dev = x3.device
        wc = eng.w_f16 if kw.get("f16") else eng.w
        cur, side = torch.cuda.current_stream(dev), eng._eval_stream(dev)
        start = torch.cuda.Event()
        start.record(cur)                      # the input (and everything the caller queued before it) is ready
        h = (B + 1) // 2
        xa, xb = x3[:h], x3[h:]
        kwa = kwb = kw
        if tok.dim() == 3:
            kwa, kwb = dict(kw, tok_ft=tok[:h]), dict(kw, tok_ft=tok[h:])
        n_tok = kw.get("n_tok")
        if n_tok is not None:                  # (ragged batches: each half its own clips' counts)
            kwa["n_tok"], kwb["n_tok"] = n_tok[:h], n_tok[h:]
        built = wc.builds
        outs_a, _ = eng.forward(xa, dt, **kwa)
        if wc.builds != built:
            side.wait_stream(cur)              # cold cache: the copies were made by kernels of the first half's stream
        else:
            side.wait_event(start)
        with torch.cuda.stream(side):
            outs_b, _ = eng.forward(xb, dt, **kwb)
        xb.record_stream(side)                 # (allocated on the caller's stream, read on the other one)
        if tok.dim() == 3:
            tok.record_stream(side)
        if n_tok is not None:
            n_tok.record_stream(side)
        cur.wait_stream(side)
        for o in outs_b:
            if o is not None:
                o.record_stream(cur)
        return tuple(None if a is None else torch.cat([a, b]) for a, b in zip(outs_a, outs_b))

    # ---- hipGraph-captured inference forward (north_star / BASELINE configs[4]) ---------------------------
    def enable_hip_graph(self, on: bool = True):
        """Forwards of a fixed input shape are captured into a HIP graph on their second call and replayed
        afterwards: one graph launch instead of ~170 kernel launches (the C ABI does no allocation and no
        synchronisation, so the whole forward is capturable).  Outputs are bit-identical to the eager path.
        Eval mode: a parameter update (version counters) or a new shape triggers a fresh capture.  Training mode
        (forward with activations saved for backward, weight recast inside the graph): see _graph_train_forward."""
        self.hip_graph = bool(on)
        if not on:
            self._graphs.clear()
        return self

    def _graph_forward(self, x3, dt, kw):
        wc = self._engine.w_f16 if kw.get("f16") else self._engine.w
        if wc.seen_train != self._engine._train_forwards:    # a training step happened since this cache was filled
            wc.clear()
            wc.seen_train = self._engine._train_forwards
            self._engine._weights_dirty = False
        key = (tuple(x3.shape), x3.dtype, dt, self.precision, kw["x3m"], bool(kw.get("f16")), kw["toffset"], int(kw["tok_ft"].shape[0]), str(x3.device),
               sum(p._version for p in self.parameters()), wc.epoch)
        st = self._graphs.get(key)
        if st is None:                                   # first call: eager (fills the operand-copy caches)
            if len(self._graphs) >= 8:
                self._graphs.clear()
            self._graphs[key] = {"graph": None}
            outs, _ = self._engine.forward(x3, dt, **kw)
            return outs
        if st["graph"] is None:                          # second call: capture
            static_x = x3.clone()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_outs, _ = self._engine.forward(static_x, dt, **kw)
            st.update(graph=g, x=static_x, outs=static_outs)
        else:
            st["x"].copy_(x3)
        st["graph"].replay()
        return tuple(o.clone() for o in st["outs"])

    def _graph_train_forward(self, x3, dt, kw):
        """Training-mode forward (activations saved for the hand-written backward) replayed from a HIP graph
        (BASELINE configs[4]: "hipGraph-captured forward").  Per input signature: call 1 runs eagerly, call 2 captures,
        later calls copy the step's inputs (batch, kept-token list, mixup / stripe draws) into the graph's static
        buffers and replay ~190 launches (weight recast included) as one.  Returns (outputs, ctx, graph state | None).

        The saved activations live in the graph's private pool and are rewritten by every replay, so a graph serves ONE
        forward at a time: the autograd node of that forward holds a lease on it until its backward has run (or the
        node is dropped), and a second grad-enabled forward of the same signature in between (two-view / consistency losses, a teacher and a
        student sharing the net) runs eagerly with its own activations instead of corrupting the first one's.
        The time-table offset is a launch argument baked into the captured kernels (and part of the graph key): inputs
        shorter than the table draw a fresh offset every step (models/maest.py:648-650); with more than 4 possible
        offsets they are not captured at all (eager) instead of re-capturing almost every step."""
        eng = self._engine
        if self._toffset_choices > 4:      # more offsets than the 8-entry graph cache should be spent on
            return (*eng.forward(x3, dt, save=True, **kw), None)
        stripes = kw.get("stripes")
        dyn = {"tok_ft": kw["tok_ft"], "perm": kw["perm"], "lam": kw["lam"],
               "t_stripes": None if stripes is None else stripes[0], "f_stripes": None if stripes is None else stripes[1]}
        plan = self._regulariser_plan()
        if plan is not None:
            self._regulariser_state(x3.device)      # (made outside any capture: the graph holds it as a static buffer)
        key = ("train", tuple(x3.shape), x3.dtype, dt, self.precision, kw["x3m"], kw["toffset"], str(x3.device), bool(eng.head_tail),
               bool(self.training), None if plan is None else (plan[0], self.drop_path_rate), tuple((k, None if v is None else tuple(v.shape)) for k, v in dyn.items()))
        st = self._graphs.get(key)
        if st is None:
            if len(self._graphs) >= 8:
                self._graphs.clear()
            self._graphs[key] = {"graph": None, "lease": None}
            return (*eng.forward(x3, dt, save=True, **kw), None)
        if st["lease"] is not None and st["lease"]() is not None:
            return (*eng.forward(x3, dt, save=True, **kw), None)
        if st["graph"] is None:
            sx = x3.clone()
            sdyn = {k: None if v is None else v.clone() for k, v in dyn.items()}
            skw = dict(toffset=kw["toffset"], tok_ft=sdyn["tok_ft"], perm=sdyn["perm"], lam=sdyn["lam"],
                       stripes=None if stripes is None else (sdyn["t_stripes"], sdyn["f_stripes"]), x3m=kw["x3m"])
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs, ctx = eng.forward(sx, dt, save=True, **skw)
            # the operand copies cast inside the graph are static buffers too: keep them as THE cache entries
            st.update(graph=g, x=sx, dyn=sdyn, outs=outs, ctx=ctx, wcache=dict(eng.w._cache))
        else:
            st["x"].copy_(x3)
            for k, v in dyn.items():
                if v is not None:
                    st["dyn"][k].copy_(v)
            # what an eager training forward does first (W.clear()): forget copies made outside the graph (the padded
            # head transposes of the last backward) -- fused optimizers update parameters without a version bump
            eng.w._cache = {k: (v[2]()._version if v[2]() is not None else v[0], v[1], v[2])
                            for k, v in st["wcache"].items()}
            eng.w.epoch += 1
            eng._weights_dirty = True
            eng._train_forwards += 1          # (the operand copies of other caches predate this step's weights)
        lease = _GraphLease()
        st["lease"] = weakref.ref(lease)
        st["graph"].replay()
        ctx = dict(st["ctx"])
        ctx["blocks"] = [dict(b) for b in st["ctx"]["blocks"]]      # backward empties these dicts as it goes
        return tuple(o.clone() for o in st["outs"]), ctx, lease

    def predict_labels(self, x):
        with torch.no_grad():      # the result is detached anyway (maest.py:936-938): take the inference path
            logits = self.forward(x)[0]
        activations = ops.sigmoid_mean(logits.detach().contiguous())
        return activations.cpu().numpy(), self.labels

    def attention_maps(self, x, blocks=None, queries: str = "head", heads: str = "all", melspectrogram_input: bool = False, *,
                       _patchout=None) -> "AttentionMaps":
        """The attention probabilities softmax(q k^T * scale) of the reference's Attention.forward (models/maest.py:371-372), per block
        -- what the HF-AST layout calls output_attentions --, next to the outputs of the same forward.

        x: everything ``forward`` accepts (1-D / 2-D audio, 2-D / 3-D / 4-D mel: the same rank dispatch, chunking and exceptions).
        blocks: an int, an iterable of ints or None (all); negative indices count from the end.  queries: "head" -- the rows of the cls
        and the dist token, [.., 2, N] -- or "all", [.., N, N].  heads: "all" -- [B, 12, Q, N] -- or "mean" -- [B, Q, N], the mean over
        the heads.  One forward under no_grad in the model's current mode and precision (eval(): the evaluation kernels, "auto" = bf16x3;
        train(): the patchout draws apply and ``tokens`` says which patches were kept), run eagerly to its end on the caller's stream
        (no two-stream split, no HIP-graph replay; the weights' operand copies are the ones every forward shares); in every requested
        block one more launch writes the map from the qkv tensor the block computed anyway (ops.attn_probs).  The maps are detached
        fp32 tensors.  `return_self_attention=True` of ``forward`` is a different tensor: proj(attn @ v) of one block, pooled."""
        return explain.attention_maps(self, x, blocks, queries, heads, melspectrogram_input, _patchout=_patchout)

    def hidden_states(self, x, blocks=None, pool="embedding", melspectrogram_input: bool = False, *, _patchout=None) -> "HiddenStates":
        """The output stream of every requested block from ONE forward -- what the HF-AST layout calls output_hidden_states --, pooled
        into the reference's embedding and along the two axes of the patch grid, next to the outputs of the same forward.

        x: everything ``forward`` accepts (the same rank dispatch, chunking and exceptions, as in ``attention_maps``).  blocks: an int,
        an iterable of ints or None (all); negative indices count from the end.  pool: "embedding", "time", "freq", "states" or an
        iterable of them (ValueError otherwise).  For every requested block k, of the stream x_k [B, N, 768] behind that block (no final
        LayerNorm; the state before block 0 is not offered):
          "embedding"  fp32 [B, 2304] = cat[x_k[:, 0], x_k[:, 1], mean(x_k[:, 2:], 1)]: what ``forward(x, transformer_block=k)[1]`` returns
          "time"       fp32 [B, Tk, 768]: per kept time patch the mean of its Fk kept frequency patches
          "freq"       fp32 [B, Fk, 768]: per kept frequency patch the mean of its Tk kept time patches
          "states"     fp32 [B, N, 768]: x_k itself, as the forward carries it; the caller owns the tensor, no later launch writes it
        "time" and "freq" need the kept tokens to be a full Fk x Tk grid in frequency-major order: every structured patchout variant and
        every eval() forward give one; a train() model with u_patchout > 0 does not (ValueError, before any device work).  Every mean is
        an fp32 sum from 0.0f in ascending token order and one division (ops.embed_pool; ops.grid_pools: one launch per block writes the
        embedding and both axis pools): bit-reproducible.

        One forward under no_grad in the model's current mode and precision, run eagerly to its end on the caller's stream (no
        two-stream split, no HIP-graph replay), recording nothing: no output requires grad, and there are no gradients through this
        call.  When the last block is not among `blocks`, logits and features are those of ``forward``, bit for bit.  When it is, the
        last block runs complete instead of on the cls / dist rows only (``_engine.head_tail``), and logits and features are, bit for
        bit, those of a forward with ``_engine.head_tail = False``.  In the 16-bit modes the stream of a block that is not the last one
        of the pass gets its fc2 add in the next block's LayerNorm pass, from a 16-bit rounded fc2 output (``_engine.split_add_eval``):
        states and pools are the forward's own values, and equal ``forward(x, transformer_block=k)`` -- which ends its pass at block k
        with an fp32 fc2 epilogue -- bit for bit in the fp32 modes, for the last block, and for every block once split_add_eval = 0.
        Returns HiddenStates: embedding / time / freq / states ({block: tensor}, ascending; empty when not requested), time_index,
        freq_index, on_time_axis(block), on_freq_axis(block) (NaN rows where the forward dropped the column / row), and logits,
        features, logits_dist, tokens, grid as in AttentionMaps.  Memory: "states" keeps B * N * 768 floats per requested block."""
        return hidden.hidden_states(self, x, blocks, pool, melspectrogram_input, _patchout=_patchout)

    def attention_rollout(self, x, start="head", blocks=None, alpha: float = 0.5, melspectrogram_input: bool = False, *,
                          _patchout=None) -> "AttentionRollout":
        """Attention rollout (Abnar & Zuidema): which input tokens feed the rows of `start` through the blocks,

            r_last = start,    r_{l-1} = alpha r_l + (1 - alpha) (r_l . A_l),    A_l = mean over the heads of softmax(q k^T * scale) of block l,

        from block `last` down to block `first`, next to the outputs of the same forward.  Each step is one weighted pooling of the block's
        attention (ops.attn_apply: R row vectors times the head-mean matrix, formed from the block's qkv tensor without writing an N x N
        map) and one elementwise mix.

        x: everything ``forward`` accepts (the same rank dispatch, chunking and exceptions).  start: "head" -- R = 2, one-hot on the cls and
        the dist token -- or a non-negative fp32 tensor [R, N] (shared by the clips) or [B, R, N], R <= 8, N the token count of the forward
        (2 + the kept patches).  blocks: None (all) or a contiguous (first, last) pair; negative indices count from the end.  alpha in
        [0, 1] weights the identity (residual) path; alpha = 1 returns `start`.  One forward under no_grad in the model's current mode and
        precision, run eagerly on the caller's stream as ``attention_maps`` runs it (eval(): the evaluation kernels; train(): the patchout
        draws apply and ``tokens`` says which patches were kept); then the sweep, top down, on the same stream.  logits and features are
        those of ``forward``.  Memory: the qkv tensor of every swept block lives until the sweep ends -- 12 x B * N * 2304 elements of the
        mode's type for a full rollout -- so split very large batches."""
        return explain.attention_rollout(self, x, start, blocks, alpha, melspectrogram_input, _patchout=_patchout)

    def attention_relevance(self, x, target, start="head", blocks=None, melspectrogram_input: bool = False, *, target_dist=None,
                            grad_scale: float = 1.0, _patchout=None) -> "AttentionRelevance":
        """Gradient-weighted attention rollout (Chefer, Gur & Wolf 2021, the self-attention rule): which input tokens make the model say
        `target`.  With s = sum(target * logits), P_h the attention probabilities of a block's head and dP_h = ds / dP_h,

            r_last = start,    r_{l-1} = r_l + r_l . A_l,    A_l = mean over the heads of max(P_h * dP_h, 0) of block l,

        from block `last` down to block `first`, next to the outputs of the same forward.  Each step is one ops.attn_relevance on the
        block's qkv tensor and on the gradient of s with respect to its attention output, which the walk forms as a backward would
        (the input-gradient chain only): no N x N tensor is written, no weight gradient is computed, no .grad is touched and no graph
        is recorded; the walk ends at block `first`.

        x, start, blocks: as in ``attention_rollout``.  target: an int class index (every clip), an integer tensor [B] of class indices,
        or a float tensor [C] / [B, C] of weights on the logits.  target_dist (distilled_type="separated" only): the same forms, on
        logits_dist.  grad_scale: a positive power of two; the seed is multiplied by it and every pooled step divided by it -- exact in
        fp32, there so that precision="fp16" gradients do not underflow.  The forward runs in the mode a grad-enabled ``forward`` of the
        model's current train() / eval() state would (precision="fp16": in half in eval() too); dropout and drop-path are not applied and
        their step counter does not move; patchout applies in train(), as for the maps.  Memory: the activations of a training forward."""
        return explain.attention_relevance(self, x, target, start, blocks, melspectrogram_input, target_dist=target_dist, grad_scale=grad_scale,
                                           _patchout=_patchout)

    def attention_heads(self, x, target=None, start="head", blocks=None, alpha: float = 0.5, melspectrogram_input: bool = False, *,
                        target_dist=None, grad_scale: float = 1.0, _patchout=None) -> "AttentionHeads":
        """Which heads carry the walk of ``attention_rollout`` (target=None) or of ``attention_relevance`` (a target): the same walk with
        the same arguments, checks and outputs, but every swept block's step is pooled head by head,

            per_head[l][b, h] = r_l . P_h of block l    (a target: r_l . max(P_h * dP_h, 0)),    fp32 [B, 12, R, N],

        kept, and the walk goes on with its mean over the heads -- the step the other two methods take, bit for bit, so ``result`` is
        their ``rollout`` / ``relevance`` (the latter where the backward repeats: deterministic=True).  One ops.attn_apply_heads /
        ops.attn_relevance_heads per block: no N x N tensor is written, and dP_h is never materialised.

        x, start, blocks: as in ``attention_rollout``.  target=None: alpha as in ``attention_rollout``; target_dist and grad_scale stay at
        their defaults.  target given: target, target_dist, grad_scale as in ``attention_relevance``; alpha stays at its default
        (ValueError otherwise: that walk has no alpha).  Returns AttentionHeads: per_head, result, kind, head_scores(row), to_grid(block,
        head, row).  Memory: that of the walk, and 12 x B * R * N floats per swept block."""
        return explain.attention_heads(self, x, target, start, blocks, alpha, melspectrogram_input, target_dist=target_dist,
                                       grad_scale=grad_scale, _patchout=_patchout)

    def forward_tokens(self, x, keep, blank=None, melspectrogram_input: bool = False, *, _patchout=None, **options):
        """``forward`` on a chosen set of patch tokens PER CLIP: what ``self(x)`` returns, from one evaluation forward under no_grad (eager, the
        two-stream split included; no HIP-graph replay, and nothing is recorded).

        x: everything ``forward`` accepts.  keep, blank: bool [B, P] over the call's own token sequence -- what the call resolves before it
        launches anything: the full patch grid in eval(), with the static patchout variants honoured; P = len of ``tokens`` of the explain
        methods.  Clip b keeps the tokens where keep[b] is set, in ascending sequence order: the reference's unstructured patchout
        (u_patchout, models/maest.py:773-780) with a chosen index list per clip; a removed patch is never computed and the attention gets
        shorter.  Tokens where blank[b] is set stay in the sequence with zeroed content: the convolution's bias plus the positional terms.
        Every row of keep must hold the same count, at least 1, and blank must be a subset of keep (ValueError; TypeError for masks that
        are no bool tensors; the value checks cost one device sync).  Gradients, maps, pools and HIP-graph replay on per-clip tokens are
        not offered.

        options: one keyword, ``ragged=False`` (any other: TypeError, as for an unknown keyword; it is taken through ``**options`` because
        the keyword-only list of this method is pinned as it was before ragged batches).
        ragged=True (a bool: TypeError otherwise): the rows of keep may hold DIFFERENT counts, each at least 1.  The batch runs at the
        longest clip's length: every clip's kept tokens in ascending sequence order, then blank pad slots, and every block's attention
        is told the clip's own token count (MAEST_ATTN_LENS: pads are neither attended nor computed there).  Cost: the per-token
        kernels run B x max count rows, attention runs the sum of the squared counts; sorting or bucketing clips by length is the
        caller's choice.  With equal counts the call is the ragged=False one, bit for bit."""
        opt = perturb.take_options("forward_tokens", options, ragged=False)
        return perturb.forward_tokens(self, x, keep, blank, melspectrogram_input, _patchout=_patchout, ragged=opt["ragged"])

    def forward_lengths(self, x, frames):
        """Clips of different durations in one batch: what ``self(x, melspectrogram_input=True)`` returns, from one evaluation forward under
        no_grad (eager; ValueError in train() mode), with clip b run on its first frames[b] mel frames only.

        x: a mel batch [B, F, T] or [B, 1, F, T], padded to the longest clip (1-D / 2-D audio: ValueError -- the STFT's edge padding makes
        a padded waveform differ from the clip alone).  frames: an integer tensor or a sequence of ints [B], 16 <= frames[b] <= T
        (TypeError / ValueError, before any launch).  Clip b runs on the tokens (f, t) of the call's evaluation token sequence with
        t < Tp_b = (frames[b] - 16) // stride_t + 1: the time patches that lie wholly inside it.  Frames >= frames[b] of x are never read
        and may hold anything, NaN included.  For a model without evaluation-time time-patchout (the default) clip b equals
        ``model(x[b:b+1, ..., :frames[b]], melspectrogram_input=True)``.  The batch runs as ``forward_tokens(ragged=True)`` does, at that
        cost: per-token kernels on B x the longest clip's rows, attention on the sum of the squared token counts."""
        return perturb.forward_lengths(self, x, frames)

    def perturbation_curve(self, x, scores, target, order: str = "positive", fractions=None, mode: str = "drop", row: int = 0,
                           melspectrogram_input: bool = False, *, seed: int = 0, _patchout=None, **options) -> "PerturbationCurve":
        """The perturbation test of Chefer, Gur & Wolf 2021 (deletion curves, MoRF / LeRF) for a score per patch token: remove a growing
        fraction of each clip's tokens in the order of its scores and record the target label's probability.  Faithful scores make it
        fall fast under order="positive" (the highest scores leave first) and slowly under "negative"; scores="random" is the baseline.

        x: everything ``forward`` accepts.  scores: fp32 [B, P] over the call's token sequence (see ``forward_tokens``); or the result of
        ``attention_rollout`` / ``attention_relevance``, whose [:, row, 2:] is used and whose ``tokens`` must be this call's (ValueError
        otherwise); or "random": per clip a permutation from a CPU torch.Generator seeded with `seed`.  Non-finite scores: ValueError.
        Equal scores leave in ascending token index in both orders (a stable sort on the device).  fractions: ascending floats in
        [0, 1), default (0.0, 0.1, .., 0.9); step k removes r_k = floor(fraction_k * P) tokens of every clip.  mode: "drop" -- the tokens
        leave the sequence, N_k = 2 + P - r_k -- or "blank" -- they stay with zeroed content (bias plus positions), N constant: the
        token-level counterpart of zeroing pixels, without the leak the overlap of the 16 x 16 patches at stride 10 would cause.
        target: a label index, or an integer tensor [B] with one per clip.  Each step is one ``forward_tokens``.  Returns
        PerturbationCurve: fractions, removed [S], logits [S, B, C], logits_dist, logit and prob [S, B], auc [B], order, mode, tokens,
        keep_mask(step).

        options: one keyword, ``by="fraction"`` (any other: TypeError; taken through ``**options`` for the reason given in ``forward_tokens``).
        by="mass" (the sufficiency / comprehensiveness form; needs order="positive" and scores >= 0 with a positive sum in every clip,
        ValueError otherwise): at fraction phi clip b removes the smallest r whose r highest scores sum to >= phi x the clip's total
        (float64 cumulative sums in the removal order; phi = 0 removes nothing; r is capped at P - 1) -- a different count per clip, so
        ``removed`` is int64 [S, B] and mode="drop" runs through the ragged forward (``forward_tokens(ragged=True)``)."""
        opt = perturb.take_options("perturbation_curve", options, by="fraction")
        return perturb.perturbation_curve(self, x, scores, target, order, fractions, mode, row, melspectrogram_input, seed=seed,
                                          _patchout=_patchout, by=opt["by"])


# --------------------------------------------------------------------------------------
# architecture registry + factory (models/maest.py:1151-1388, 1467-1569)
# --------------------------------------------------------------------------------------
_ARCH_DEFAULT_T = {
    "passt_deit_bd_p16_384": 998,
    "passt_s_swa_p16_128_ap476": 998,
    "discogs-maest-10s-fs-129e": 625,
    "discogs-maest-10s-pw-129e": 625,
    "discogs-maest-10s-dw-75e": 625,
    "discogs-maest-5s-pw-129e": 312,
    "discogs-maest-20s-pw-129e": 1250,
    "discogs-maest-30s-pw-129e": 1875,
    "discogs-maest-30s-pw-73e-ts": 1875,
    "discogs-maest-30s-pw-129e-519l": 1875,
}


def get_maest(arch, pretrained: bool = True, n_classes: int = 400, in_channels: int = 1, stride_f: int = 10,
              stride_t: int = 10, input_f: int = 96, input_t: int = None, u_patchout: int = 0, s_patchout_t: int = 0,
              s_patchout_f: int = 0, s_patchout_f_indices: tuple = (), s_patchout_f_interleaved: int = 0,
              s_patchout_t_indices: tuple = (), s_patchout_t_interleaved: int = 0, distilled_type: str = "mean",
              checkpoint: str = None, checkpoint_swa_weigts: bool = True, checkpoint_discard_head: bool = False,
              precision: str = "auto", *, drop_rate: float = 0.0, drop_path_rate: float = 0.0, deterministic=None):
    """Same signature and semantics as the reference factory (models/maest.py:1467-1569), plus
    ``precision`` (see the module docstring) and the keyword-only ``drop_rate`` / ``drop_path_rate`` / ``deterministic`` of the MAEST
    constructor.
    Returns the model in train mode, like the reference."""
    if arch not in _ARCH_DEFAULT_T:
        raise NotImplementedError(f"model {arch} not implemented")
    if pretrained:
        raise RuntimeError(
            "pretrained=True downloads release checkpoints over the network (reference: timm load_pretrained, "
            "models/helpers/vit_helpers.py:257-267), which this build does not do. Use pretrained=False and "
            "checkpoint=<local .ckpt>.")
    if not input_t:
        input_t = _ARCH_DEFAULT_T[arch]
    if (stride_f, stride_t) != (10, 10):
        warnings.warn(f"This model was pre-trained with strides {(10, 10)}, but now you set (fstride,tstride) "
                      f"to {(stride_f, stride_t)}.")
    if arch == "discogs-maest-30s-pw-129e-519l" and n_classes != 519:
        _logger.debug("Forcing `num_classes` to 519")
        n_classes = 519
    model = MAEST(u_patchout=u_patchout, s_patchout_t=s_patchout_t, s_patchout_f=s_patchout_f,
                  s_patchout_f_indices=s_patchout_f_indices, s_patchout_f_interleaved=s_patchout_f_interleaved,
                  s_patchout_t_indices=s_patchout_t_indices, s_patchout_t_interleaved=s_patchout_t_interleaved,
                  img_size=(input_f, input_t), patch_size=16, stride=(stride_f, stride_t), in_chans=in_channels,
                  num_classes=n_classes, embed_dim=768, depth=12, num_heads=12, distilled=True,
                  distilled_type=distilled_type, precision=precision, drop_rate=drop_rate, drop_path_rate=drop_path_rate,
                  deterministic=deterministic)
    if checkpoint:
        state_dict = torch.load(checkpoint, map_location="cpu")["state_dict"]
        replace_str = "net_swa." if checkpoint_swa_weigts else ""
        state_dict = {k.replace(replace_str, ""): v for k, v in state_dict.items()}
        if checkpoint_discard_head:
            state_dict = {k: v for k, v in state_dict.items() if "head" not in k}
        model.load_state_dict(state_dict, strict=False)
    return model


from . import explain  # noqa: E402  (attention maps, rollout, relevance: a module of their own, which reads the names above)
from .explain import (AttentionHeads, AttentionMaps, AttentionRelevance, AttentionRollout, _INT_DTYPES, _check_target, _check_target_clips,  # noqa: E402, F401
                      _scatter_on_grid, _target_seed)
from . import hidden  # noqa: E402  (the hidden states: reads the names above and explain's)
from .hidden import HiddenStates  # noqa: E402, F401
from . import perturb  # noqa: E402  (per-clip token removal and the perturbation curves: reads explain's names)
from .perturb import PerturbationCurve  # noqa: E402, F401
