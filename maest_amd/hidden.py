"""What MAEST.hidden_states runs (its contract is that method's docstring, maest_amd/maest.py): the argument checks -- all of them before
any device work --, one engine forward with a tap on every block's output stream (tap_x), the pools of the tapped streams, and the result
class.  The engine knows nothing of the feature: its forward hands tap_x(i, x) the fp32 stream behind block i as soon as it exists."""
from __future__ import annotations

import torch

from . import ops
from .explain import _Explained, _check_blocks, _outputs, _scatter_on_grid
from .maest import EMBED_DIM, HEAD_TOKENS

POOLS = ("embedding", "time", "freq", "states")


class HiddenStates(_Explained):
    """What MAEST.hidden_states returns.  logits, features, logits_dist, tokens, grid: of the same forward, as in AttentionMaps.
    embedding, time, freq, states: {block index: fp32 tensor}, the requested blocks in ascending order; a pool that was not requested is an
    empty dict.  embedding[k]: [B, 2304] = cat[cls, dist, mean of the patch tokens] of block k's output stream; time[k]: [B, Tk, 768], per
    kept time patch the mean of its Fk kept frequency patches; freq[k]: [B, Fk, 768], per kept frequency patch the mean of its Tk kept time
    patches; states[k]: [B, N, 768], the stream itself.  time_index, freq_index: int64 [Tk] / [Fk], the kept time and frequency patch
    numbers (None where the kept tokens are no full grid: a train() model with u_patchout)."""

    def __init__(self, logits, features, tokens, grid, logits_dist=None, embedding=None, time=None, freq=None, states=None,
                 time_index=None, freq_index=None):
        super().__init__(logits, features, tokens, grid, logits_dist)
        self.embedding, self.time, self.freq, self.states = ({} if d is None else d for d in (embedding, time, freq, states))
        self.time_index, self.freq_index = time_index, freq_index

    @staticmethod
    def _on_axis(rows: torch.Tensor, index: torch.Tensor, size: int) -> torch.Tensor:
        """[B, kept, 768] -> [B, size, 768]: the axis as a 1 x size patch grid, NaN where the forward dropped the patch."""
        tok = torch.stack([torch.zeros_like(index), index], dim=1)
        return _scatter_on_grid(rows.transpose(1, 2), tok, (1, size)).squeeze(2).transpose(1, 2).contiguous()

    def on_time_axis(self, block: int) -> torch.Tensor:
        """time[block] laid out on the complete time axis: [B, T', 768], NaN rows where the forward dropped the column (the convention
        of to_grid)."""
        return self._on_axis(self.time[block], self.time_index, self.grid[1])

    def on_freq_axis(self, block: int) -> torch.Tensor:
        """freq[block] laid out on the complete frequency axis: [B, F', 768], NaN rows where the forward dropped the row."""
        return self._on_axis(self.freq[block], self.freq_index, self.grid[0])


def _check_pool(pool) -> frozenset:
    if isinstance(pool, str):
        want = [pool]
    elif hasattr(pool, "__iter__"):
        want = list(pool)
    else:
        raise ValueError(f"pool must be one of {POOLS} or an iterable of them, got {pool!r}")
    for p in want:
        if not isinstance(p, str) or p not in POOLS:
            raise ValueError(f"pool must be one of {POOLS} or an iterable of them, got {p!r}")
    if not want:
        raise ValueError(f"pool must name at least one of {POOLS}")
    return frozenset(want)


def kept_axes(tokens: torch.Tensor):
    """tokens int [P, 2] = (frequency patch, time patch) in sequence order -> (freq_index [Fk], time_index [Tk]) when they are the full
    Fk x Tk grid of those in frequency-major order, else None."""
    tok = tokens.detach().cpu().long()
    P = int(tok.shape[0])
    Tk = int((tok[:, 0] == tok[0, 0]).sum()) if P else 0
    if Tk < 1 or P % Tk:
        return None
    f, t = tok[::Tk, 0].contiguous(), tok[:Tk, 1].contiguous()
    full = torch.stack(torch.meshgrid(f, t, indexing="ij"), dim=-1).reshape(-1, 2)
    return (f, t) if torch.equal(full, tok) else None


def _axes_of(model, kw, grid, cached: bool):
    """kept_axes of this call's tokens; an evaluation forward's token list is the model's cached tensor, read back from the device once."""
    tok = kw["tok_ft"]
    if not cached:
        return kept_axes(tok)
    memo = model.__dict__.setdefault("_hidden_axes", {})
    key = (tuple(grid), str(tok.device))
    if key not in memo or memo[key][0] is not tok:
        memo[key] = (tok, kept_axes(tok))
    return memo[key][1]


def hidden_states(model, x, blocks, pool, melspectrogram_input, *, _patchout):
    pools = _check_pool(pool)
    want = _check_blocks(model, blocks)
    axis_pools = bool(pools & {"time", "freq"})
    if axis_pools and model.training and model.u_patchout:
        raise ValueError("pool 'time' / 'freq' needs the kept tokens to be a full frequency x time grid: a train() model with u_patchout "
                         f"= {model.u_patchout} drops single patches (structured patchout and every eval() forward keep a grid)")
    x3, dt, kw, _, grid = model._resolve_call(x, melspectrogram_input, None, _patchout, None, recording=False)
    axes = _axes_of(model, kw, grid, cached=not model.training and _patchout is None)
    if axis_pools and axes is None:
        raise ValueError("pool 'time' / 'freq' needs the kept tokens to be a full frequency x time grid")
    B = x3.shape[0]
    N = HEAD_TOKENS + int(kw["tok_ft"].shape[0])
    out = {p: {} for p in POOLS}

    def tap_x(i, xs):
        if i not in want:
            return
        xs = xs.reshape(B, N, EMBED_DIM)
        if "states" in pools:
            out["states"][i] = xs
        if axis_pools:      # one launch: the head rows, the mean row (the three of them: the embedding) and both axis pools
            head, mean, freq, time = ops.grid_pools(xs, int(axes[1].numel()), HEAD_TOKENS)
            if "embedding" in pools:
                assert mean.data_ptr() == head.data_ptr() + 4 * HEAD_TOKENS * EMBED_DIM      # cls, dist and the mean row lie in a row
                out["embedding"][i] = torch.as_strided(head, (B, 3 * EMBED_DIM), (head.stride(0), 1))
            if "time" in pools:
                out["time"][i] = time
            if "freq" in pools:
                out["freq"][i] = freq
        elif "embedding" in pools:
            out["embedding"][i] = ops.embed_pool(xs)

    with torch.no_grad():
        # the last block runs complete when its stream is wanted (eager, on the caller's stream: no two-stream split, no HIP-graph replay)
        outs, _ = model._engine.forward(x3, dt, tap_x=tap_x, full_last=len(model.blocks) - 1 in want, **kw)
    return HiddenStates(**_outputs(outs, kw, grid), **{p: {i: out[p][i] for i in sorted(out[p])} for p in POOLS},
                        time_index=None if axes is None else axes[1], freq_index=None if axes is None else axes[0])
