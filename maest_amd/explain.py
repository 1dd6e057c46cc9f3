"""What MAEST.attention_maps / attention_rollout / attention_relevance / attention_heads run (their contracts are the docstrings of those methods,
maest_amd/maest.py): the argument checks -- all of them before any device work --, one engine forward with a tap on every block's qkv
tensor, the sweeps over the blocks, and the result classes.  The engine knows nothing of these features: the forward hands a tap
(i, qkv, mode) behind each qkv GEMM, and the relevance step rides as a tap on the engine's one backward chain."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import ops
from .maest import HEAD_TOKENS


class _Explained:
    """logits, features: the outputs of the forward that was explained (logits_dist: the distillation head's, with
    distilled_type="separated"; else None).  Key token 0 is cls, 1 is dist, tokens[j] = (frequency patch, time patch) of key token 2 + j
    (int32 [N - 2, 2]: the patches the forward kept, in sequence order); grid = (F', T') of the complete patch grid."""

    def __init__(self, logits, features, tokens, grid, logits_dist=None):
        self.logits, self.features, self.tokens, self.grid, self.logits_dist = logits, features, tokens, tuple(grid), logits_dist

    def _on_grid(self, row: torch.Tensor) -> torch.Tensor:
        return _scatter_on_grid(row, self.tokens, self.grid)


def _scatter_on_grid(row: torch.Tensor, tokens: torch.Tensor, grid) -> torch.Tensor:
    """[.., N - 2] values of the kept patch tokens -> [.., F', T'] on the complete patch grid, NaN where the forward dropped the patch."""
    Fp, Tp = grid
    tok = tokens.to(device=row.device, dtype=torch.long)
    out = torch.full(row.shape[:-1] + (Fp * Tp,), float("nan"), dtype=row.dtype, device=row.device)
    out[..., tok[:, 0] * Tp + tok[:, 1]] = row
    return out.reshape(row.shape[:-1] + (Fp, Tp))


class AttentionMaps(_Explained):
    """What MAEST.attention_maps returns.  logits, features: the outputs of the same forward (logits_dist: the distillation head's, with
    distilled_type="separated"; else None).  maps: {block index: fp32 [B, 12, Q, N] or, heads="mean", [B, Q, N]}; key token 0 is cls, 1 is
    dist, tokens[j] = (frequency patch, time patch) of key token 2 + j (int32 [N - 2, 2]: the patches the forward kept, in sequence
    order); grid = (F', T') of the complete patch grid."""

    def __init__(self, logits, features, maps, tokens, grid, logits_dist=None):
        super().__init__(logits, features, tokens, grid, logits_dist)
        self.maps = maps

    def to_grid(self, block: int, query: int = 0, head: Optional[int] = None) -> torch.Tensor:
        """Row `query` of block `block`'s map (0: cls, 1: dist) laid out on the patch grid: [B, F', T'] for one head (or a map of
        heads="mean"), [B, 12, F', T'] for every head (head=None); NaN where the forward dropped the patch."""
        p = self.maps[block]
        if p.dim() == 4:
            return self._on_grid(p[:, :, query, 2:] if head is None else p[:, head, query, 2:])
        if head is not None:
            raise ValueError("these maps are the mean over the heads: there is no head to select")
        return self._on_grid(p[:, query, 2:])


class AttentionRollout(_Explained):
    """What MAEST.attention_rollout returns.  rollout: fp32 [B, R, N], detached; key token 0 is cls, 1 is dist, tokens[j] = (frequency patch,
    time patch) of key token 2 + j; every row sums to the sum of its start row.  logits, features, logits_dist, tokens, grid: of the same
    forward, as in AttentionMaps."""

    def __init__(self, rollout, logits, features, tokens, grid, logits_dist=None):
        super().__init__(logits, features, tokens, grid, logits_dist)
        self.rollout = rollout

    def to_grid(self, row: int = 0) -> torch.Tensor:
        """Row `row` of the rollout (start="head": 0 = cls, 1 = dist) over the patch tokens, laid out on the patch grid: [B, F', T'], NaN
        where the forward dropped the patch."""
        return self._on_grid(self.rollout[:, row, 2:])


class AttentionRelevance(_Explained):
    """What MAEST.attention_relevance returns.  relevance: fp32 [B, R, N], detached, >= start elementwise; key token 0 is cls, 1 is dist,
    tokens[j] = (frequency patch, time patch) of key token 2 + j.  logits, features, logits_dist, tokens, grid: of the same forward, as
    in AttentionMaps."""

    def __init__(self, relevance, logits, features, tokens, grid, logits_dist=None):
        super().__init__(logits, features, tokens, grid, logits_dist)
        self.relevance = relevance

    def to_grid(self, row: int = 0) -> torch.Tensor:
        """Row `row` of the relevance (start="head": 0 = cls, 1 = dist) over the patch tokens, laid out on the patch grid: [B, F', T'],
        NaN where the forward dropped the patch."""
        return self._on_grid(self.relevance[:, row, 2:])


class AttentionHeads(_Explained):
    """What MAEST.attention_heads returns.  kind: "rollout" (no target) or "relevance".  per_head: {block index: fp32 [B, 12, R, N]}, detached,
    the swept blocks in ascending order: per_head[l][b, h, r, k] is what head h of block l alone pools from the walk's row r onto key token
    k -- the term whose mean over the heads is the step of the walk at that block.  result: fp32 [B, R, N], the end of the walk: bit for
    bit the rollout / the relevance of the same arguments.  logits, features, logits_dist, tokens, grid: of the same forward, as in
    AttentionMaps."""

    def __init__(self, per_head, result, kind, logits, features, tokens, grid, logits_dist=None):
        super().__init__(logits, features, tokens, grid, logits_dist)
        self.per_head, self.result, self.kind = per_head, result, kind

    def head_scores(self, row: int = 0) -> torch.Tensor:
        """[B, number of swept blocks, 12]: per block (ascending) and head, the sum over the key tokens of per_head[block][:, head, row, :]
        -- how much of row `row` (start="head": 0 = cls, 1 = dist) that head passes on at that block."""
        return torch.stack([self.per_head[i][:, :, row, :].sum(dim=-1) for i in sorted(self.per_head)], dim=1)

    def to_grid(self, block: int, head: int, row: int = 0) -> torch.Tensor:
        """Row `row` of one head of block `block` over the patch tokens, laid out on the patch grid: [B, F', T'], NaN where the forward
        dropped the patch."""
        return self._on_grid(self.per_head[block][:, head, row, 2:])


def _outputs(outs, kw, grid):
    """The arguments every result class ends with, from the engine's output tuple."""
    return dict(logits=outs[0], features=outs[-1], tokens=kw["tok_ft"], grid=grid, logits_dist=outs[1] if len(outs) == 3 else None)


def _check_blocks(model, blocks) -> frozenset:
    """The blocks a per-block output is wanted of: an int, an iterable of ints or None (all); negative indices count from the end."""
    depth = len(model.blocks)
    if blocks is None:
        return frozenset(range(depth))
    if isinstance(blocks, (bool, str)) or not (isinstance(blocks, int) or hasattr(blocks, "__iter__")):
        raise TypeError(f"blocks must be an int, an iterable of ints or None, got {blocks!r}")
    want = [blocks] if isinstance(blocks, int) else list(blocks)
    for i in want:
        if isinstance(i, bool) or not isinstance(i, int):
            raise TypeError(f"blocks must be an int, an iterable of ints or None, got an element {i!r}")
        if not -depth <= i < depth:
            raise ValueError(f"block index {i} out of range for a model of {depth} blocks")
    return frozenset(i % depth for i in want)


def attention_maps(model, x, blocks, queries, heads, melspectrogram_input, *, _patchout):
    if queries not in ("head", "all"):
        raise ValueError(f"queries must be 'head' or 'all', got {queries!r}")
    if heads not in ("all", "mean"):
        raise ValueError(f"heads must be 'all' or 'mean', got {heads!r}")
    want = _check_blocks(model, blocks)
    x3, dt, kw, _, grid = model._resolve_call(x, melspectrogram_input, None, _patchout, None, recording=False)
    maps = {}
    q_rows = HEAD_TOKENS if queries == "head" else None

    def tap(i, qkv, mode):
        if i in want:
            B, N, scale, x3m, qs = mode
            maps[i] = ops.attn_probs(qkv, B, N, scale, q_rows=q_rows, x3=x3m, q_prescaled=qs, head_mean=heads == "mean")

    with torch.no_grad():
        outs, _ = model._engine.forward(x3, dt, tap=tap, **kw)
    return AttentionMaps(maps={i: maps[i] for i in sorted(maps)}, **_outputs(outs, kw, grid))


def _check_sweep(model, start, blocks):
    """The checks ``attention_rollout`` makes on `start` and `blocks` before any device work -> (head_start, first, last)."""
    head_start = isinstance(start, str)
    if head_start:
        if start != "head":
            raise ValueError(f"start must be 'head' or a tensor [R, N] / [B, R, N], got {start!r}")
    else:
        if not torch.is_tensor(start) or start.dtype != torch.float32 or start.dim() not in (2, 3):
            raise ValueError("start must be 'head' or a float32 tensor [R, N] / [B, R, N], got "
                             + (f"a {start.dtype} tensor of shape {tuple(start.shape)}" if torch.is_tensor(start) else repr(start)))
        if not 1 <= start.shape[-2] <= 8:
            raise ValueError(f"start has R = {start.shape[-2]} rows: 1 .. 8 are served")
        if not bool((start >= 0).all()):
            raise ValueError("start must be non-negative (and hold no NaN)")
    depth = len(model.blocks)
    if blocks is None:
        return head_start, 0, depth - 1
    sel = list(blocks) if isinstance(blocks, (tuple, list)) else None
    if sel is None or any(isinstance(i, bool) or not isinstance(i, int) for i in sel):
        raise TypeError(f"blocks must be None or a (first, last) pair of ints, got {blocks!r}")
    if len(sel) != 2:
        raise ValueError(f"blocks must be a contiguous range given as a (first, last) pair, got {blocks!r}")
    for i in sel:
        if not -depth <= i < depth:
            raise ValueError(f"block index {i} out of range for a model of {depth} blocks")
    first, last = (i % depth for i in sel)
    if first > last:
        raise ValueError(f"blocks = {blocks!r}: first must not lie above last")
    return head_start, first, last


def _resolve_sweep(model, x, melspectrogram_input, _patchout, recording, start, head_start):
    """_resolve_call for a sweep, and the check of `start` against the forward's clips and tokens."""
    x3, dt, kw, _, grid = model._resolve_call(x, melspectrogram_input, None, _patchout, None, recording=recording)
    B, N = x3.shape[0], 2 + int(kw["tok_ft"].shape[0])
    if not head_start and (start.shape[-1] != N or (start.dim() == 3 and start.shape[0] != B)):
        raise ValueError(f"start has shape {tuple(start.shape)}: this forward has B = {B} clips of N = {N} tokens")
    return x3, dt, kw, grid, B, N


def _sweep_start(start, head_start, B, N, dev):
    if head_start:
        r = torch.zeros((B, HEAD_TOKENS, N), dtype=torch.float32, device=dev)
        r[:, 0, 0] = 1.0
        r[:, 1, 1] = 1.0
        return r
    r = start.detach().to(dev)
    r = (r.unsqueeze(0).expand(B, -1, -1) if r.dim() == 2 else r).contiguous()
    return r.clone() if r.data_ptr() % 16 else r      # (a contiguous slice of a larger tensor: the kernel wants 16-byte aligned operands)


def _check_alpha(alpha):
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha must be a number in [0, 1], got {alpha!r}")


def _rollout_walk(model, x, start, blocks, alpha, melspectrogram_input, _patchout, per_head=None):
    """The walk of attention_rollout -> (r, the result classes' closing arguments).  per_head (a dict): every step is pooled head by head
    (ops.attn_apply_heads), kept there under its block index, and the walk goes on with its mean -- the same bits (ops.heads_mean)."""
    _check_alpha(alpha)
    head_start, first, last = _check_sweep(model, start, blocks)
    x3, dt, kw, grid, B, N = _resolve_sweep(model, x, melspectrogram_input, _patchout, False, start, head_start)
    kept = {}      # block index -> (qkv, mode), alive until the sweep below has read it

    def tap(i, qkv, mode):
        if first <= i <= last:
            kept[i] = qkv, mode

    with torch.no_grad():
        outs, _ = model._engine.forward(x3, dt, tap=tap, **kw)
        r = _sweep_start(start, head_start, B, N, x3.device)
        # r_{l-1} = alpha r_l + (1 - alpha) (r_l . mean_h P_l), top down: one ops.attn_apply per block -- no N x N tensor -- and one
        # elementwise mix on [B, R, N]; a one-hot start reads the two head-token query rows only at the top block
        with model._engine._pass(kw.get("f16")):
            for i in range(last, first - 1, -1):
                qkv, (_, _, scale, x3m, qs) = kept[i]
                q_rows = HEAD_TOKENS if head_start and i == last else None
                if per_head is None:
                    y = ops.attn_apply(qkv, r, B, N, scale, q_rows=q_rows, x3=x3m, q_prescaled=qs)
                else:
                    per_head[i] = ops.attn_apply_heads(qkv, r, B, N, scale, q_rows=q_rows, x3=x3m, q_prescaled=qs)
                    y = ops.heads_mean(per_head[i])
                r = torch.add(r * float(alpha), y, alpha=1.0 - float(alpha))
    return r, _outputs(outs, kw, grid)


def attention_rollout(model, x, start, blocks, alpha, melspectrogram_input, *, _patchout):
    r, out = _rollout_walk(model, x, start, blocks, alpha, melspectrogram_input, _patchout)
    return AttentionRollout(rollout=r, **out)


_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def _check_target(target, C: int, what: str):
    """What can be said about a target of attention_relevance without the batch size: its form, the range of class indices, finiteness."""
    if isinstance(target, bool):
        raise TypeError(f"{what} must be an int class index, an integer tensor [B] or a float tensor [C] / [B, C], got {target!r}")
    if isinstance(target, int):
        if not 0 <= target < C:
            raise ValueError(f"{what} = {target} out of range for {C} classes")
        return
    if not torch.is_tensor(target):
        raise TypeError(f"{what} must be an int class index, an integer tensor [B] or a float tensor [C] / [B, C], got {target!r}")
    if target.dtype in _INT_DTYPES:
        if target.dim() != 1:
            raise ValueError(f"{what}: an integer tensor holds one class index per clip, [B]; got shape {tuple(target.shape)}")
        if target.numel() and not (0 <= int(target.min()) and int(target.max()) < C):
            raise ValueError(f"{what} holds a class index out of range for {C} classes")
    elif target.is_floating_point():
        if target.dim() not in (1, 2) or target.shape[-1] != C:
            raise ValueError(f"{what}: a float tensor holds weights on the {C} logits, [C] or [B, C]; got shape {tuple(target.shape)}")
        if not bool(torch.isfinite(target).all()):
            raise ValueError(f"{what} must be finite")
    else:
        raise TypeError(f"{what} must be an int class index, an integer tensor [B] or a float tensor [C] / [B, C], got a {target.dtype} tensor")


def _check_target_clips(target, B: int, what: str):
    if torch.is_tensor(target) and target.dim() == (1 if target.dtype in _INT_DTYPES else 2) and target.shape[0] != B:
        raise ValueError(f"{what} has shape {tuple(target.shape)}: this forward has B = {B} clips")


def _target_seed(target, B: int, C: int, what: str, dev, grad_scale: float) -> torch.Tensor:
    """grad_scale * d(sum(target * logits)) / d logits: fp32 [B, C] on the device."""
    _check_target_clips(target, B, what)
    if isinstance(target, int) or target.dtype in _INT_DTYPES:
        idx = torch.full((B,), target, dtype=torch.long) if isinstance(target, int) else target.detach().cpu().long()
        seed = torch.zeros((B, C), dtype=torch.float32)
        seed[torch.arange(B), idx] = grad_scale
        return seed.to(dev)
    seed = target.detach().to(device=dev, dtype=torch.float32) * grad_scale
    return (seed.unsqueeze(0).expand(B, -1) if seed.dim() == 1 else seed).contiguous()


def _relevance_walk(model, x, target, start, blocks, melspectrogram_input, target_dist, grad_scale, _patchout, per_head=None):
    """The walk of attention_relevance -> (r, the result classes' closing arguments).  per_head (a dict): as in _rollout_walk, with
    ops.attn_relevance_heads."""
    head_start, first, last = _check_sweep(model, start, blocks)
    C = model.head[1].out_features
    _check_target(target, C, "target")
    if target_dist is not None:
        if model.distilled_type != "separated":
            raise ValueError(f"target_dist needs distilled_type='separated': this model's is {model.distilled_type!r}")
        _check_target(target_dist, model.head_dist.out_features, "target_dist")
    if (isinstance(grad_scale, bool) or not isinstance(grad_scale, (int, float)) or not 0.0 < float(grad_scale) < float("inf")
            or math.frexp(float(grad_scale))[0] != 0.5):
        raise ValueError(f"grad_scale must be a positive power of two, got {grad_scale!r}")
    if torch.is_tensor(x) and x.dim() in (3, 4):      # a mel batch says how many clips it holds before anything is launched
        for t, what in ((target, "target"), (target_dist, "target_dist")):
            _check_target_clips(t, x.shape[0], what)
    x3, dt, kw, grid, B, N = _resolve_sweep(model, x, melspectrogram_input, _patchout, "always", start, head_start)
    seeds = [_target_seed(target, B, C, "target", x3.device, float(grad_scale))]
    if model.distilled_type == "separated":
        seeds.append(None if target_dist is None else
                     _target_seed(target_dist, B, model.head_dist.out_features, "target_dist", x3.device, float(grad_scale)))
    seeds.append(None)
    with torch.no_grad():
        outs, ctx = model._engine.forward(x3, dt, save=True, explain=True, **kw)
        r = _sweep_start(start, head_start, B, N, x3.device)

        def step(i, s, dao):
            # r_{l-1} = r_l + r_l . mean_h max(P_l * dP_l, 0) at block l = i, dP_l formed inside ops.attn_relevance from `dao`, the gradient
            # of s = sum(seeds * outputs) / grad_scale with respect to the block's attention output: no N x N tensor
            nonlocal r
            if i > last:
                return
            # behind a head-rows block only the head tokens' queries have a gradient (the other rows of dao are zero or unwritten);
            # a one-hot start reads those two rows at the top of the sweep as well
            q_rows = HEAD_TOKENS if s["tail"] or (head_start and i == last) else None
            scale = model.blocks[i].attn.scale
            if per_head is None:
                y = ops.attn_relevance(s["qkv"], dao, r, B, N, scale, q_rows=q_rows, x3=ctx["x3m"], q_prescaled=ctx["qs"])
            else:
                per_head[i] = ops.attn_relevance_heads(s["qkv"], dao, r, B, N, scale, q_rows=q_rows, x3=ctx["x3m"], q_prescaled=ctx["qs"])
                y = ops.heads_mean(per_head[i])
            r = torch.add(r, y, alpha=1.0 / float(grad_scale))

        # the input-gradient chain of a backward, down to block `first`: no weight gradient, no .grad, no side stream, no sink
        model._engine.backward(ctx, tuple(seeds), weights=False, first=first, tap=step)
    return r, _outputs(outs, kw, grid)


def attention_relevance(model, x, target, start, blocks, melspectrogram_input, *, target_dist, grad_scale, _patchout):
    r, out = _relevance_walk(model, x, target, start, blocks, melspectrogram_input, target_dist, grad_scale, _patchout)
    return AttentionRelevance(relevance=r, **out)


def attention_heads(model, x, target, start, blocks, alpha, melspectrogram_input, *, target_dist, grad_scale, _patchout):
    per_head = {}
    if target is None:
        if target_dist is not None:
            raise ValueError("target_dist needs a target: without one the walk is the rollout, which reads no label")
        if isinstance(grad_scale, bool) or not isinstance(grad_scale, (int, float)) or float(grad_scale) != 1.0:
            raise ValueError(f"grad_scale belongs to the walk with a target: without one leave it at its default, got {grad_scale!r}")
        r, out = _rollout_walk(model, x, start, blocks, alpha, melspectrogram_input, _patchout, per_head)
    else:
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or float(alpha) != 0.5:
            raise ValueError(f"alpha belongs to the rollout walk (target=None): with a target leave it at its default, got {alpha!r}")
        r, out = _relevance_walk(model, x, target, start, blocks, melspectrogram_input, target_dist, grad_scale, _patchout, per_head)
    return AttentionHeads(per_head={i: per_head[i] for i in sorted(per_head)}, result=r, kind="rollout" if target is None else "relevance",
                          **out)
