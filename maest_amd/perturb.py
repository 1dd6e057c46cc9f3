"""What MAEST.forward_tokens / MAEST.perturbation_curve run (their contracts are the docstrings of those methods, maest_amd/maest.py): the
argument checks, the ranking and the masks -- pure torch, on whatever device the scores live (removal_order, keep_mask: testable without a
kernel) --, the table of kept tokens per clip, one evaluation forward per step, and the result class.  The engine takes the table as a
3-D tok_ft (include/maest_hip.h: MAEST_IM2COL_CLIP_TOKENS); a removed patch is never computed and the attention gets shorter."""
from __future__ import annotations

import math

import torch

from ._lib import TOK_BLANK
from .explain import _INT_DTYPES, AttentionRelevance, AttentionRollout

ORDERS = ("positive", "negative")
MODES = ("drop", "blank")
BYS = ("fraction", "mass")
PATCH = 16      # frames (and bands) of a patch: the convolution's kernel (models/maest.py:214-241)
DEFAULT_FRACTIONS = tuple(k / 10 for k in range(10))


# ------------------------------------------------------------------------------------------------ ranking and masks (pure torch)
def removal_order(scores: torch.Tensor, order: str) -> torch.Tensor:
    """scores [B, P] -> int64 [B, P]: per clip the token indices in the order they are removed -- "positive": the highest score first,
    "negative": the lowest first; equal scores leave in ascending token index in both orders (a stable sort, on the scores' device)."""
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    key = -scores if order == "positive" else scores      # (negation is exact, and -0.0 == 0.0 stays a tie)
    return torch.sort(key, dim=1, stable=True).indices


def keep_mask(rank: torch.Tensor, removed: int) -> torch.Tensor:
    """rank int64 [B, P] (removal_order), removed = r in 0 .. P -> bool [B, P], False at the first r tokens of every clip's order."""
    B, P = rank.shape
    if not 0 <= removed <= P:
        raise ValueError(f"removed = {removed} outside 0 .. {P}")
    keep = torch.ones((B, P), dtype=torch.bool, device=rank.device)
    keep.scatter_(1, rank[:, :removed], False)
    return keep


def keep_mask_counts(rank: torch.Tensor, removed: torch.Tensor) -> torch.Tensor:
    """keep_mask with a count per clip: removed int64 [B], 0 .. P each -> bool [B, P], False at the first removed[b] tokens of clip b's order."""
    B, P = rank.shape
    removed = removed.to(rank.device)
    if tuple(removed.shape) != (B,) or not bool(((removed >= 0) & (removed <= P)).all()):
        raise ValueError(f"removed must hold {B} counts in 0 .. {P}")
    gone = torch.arange(P, device=rank.device).unsqueeze(0) < removed.unsqueeze(1)      # in removal order
    return torch.ones((B, P), dtype=torch.bool, device=rank.device).scatter_(1, rank, ~gone)


def mass_removed_counts(scores: torch.Tensor, rank: torch.Tensor, fractions) -> torch.Tensor:
    """by="mass": scores [B, P] >= 0 with a positive sum per clip, rank = removal_order(scores, "positive") -> int64 [S, B]: at fraction
    phi clip b removes the smallest r whose r highest scores sum to >= phi x the clip's total (float64 cumulative sums in the order of
    `rank`; the total is the last of them), capped at P - 1.  phi = 0 removes nothing."""
    P = scores.shape[1]
    cum = scores.gather(1, rank).to(torch.float64).cumsum(1)                             # c_1 .. c_P; c_0 = 0
    cum = torch.cat([torch.zeros_like(cum[:, :1]), cum], 1)
    out = []
    for f in fractions:
        r = (cum < float(f) * cum[:, -1:]).sum(1)                                        # c_j ascends: the first j with c_j >= phi c_P
        out.append(r.clamp(max=P - 1))
    return torch.stack(out).to(torch.int64)


def frames_to_time_patches(frames: torch.Tensor, stride_t: int) -> torch.Tensor:
    """frames int [B] >= 16 -> the time patches that lie wholly inside each clip, Tp_b = (frames[b] - 16) // stride_t + 1."""
    return torch.div(frames.to(torch.int64) - PATCH, int(stride_t), rounding_mode="floor") + 1


def random_scores(B: int, P: int, seed: int) -> torch.Tensor:
    """The "random" ranking: per clip a permutation of 0 .. P - 1 as fp32 scores, drawn from a CPU torch.Generator seeded with `seed`."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.stack([torch.randperm(P, generator=gen) for _ in range(B)]).to(torch.float32)


def removed_counts(fractions, P: int):
    """r_k = floor(fraction_k * P) per step."""
    return [int(math.floor(f * P)) for f in fractions]


def trapezoid_auc(prob: torch.Tensor, fractions) -> torch.Tensor:
    """prob [S, B] over `fractions` (S >= 2, ascending) -> [B]: the trapezoid rule divided by the span of the fractions."""
    f = torch.tensor(list(fractions), dtype=torch.float64, device=prob.device)
    p = prob.to(torch.float64)
    area = ((p[1:] + p[:-1]) * 0.5 * (f[1:] - f[:-1]).unsqueeze(1)).sum(0)
    return (area / (f[-1] - f[0])).to(torch.float32)


class PerturbationCurve:
    """What MAEST.perturbation_curve returns.  fractions: the S fractions as floats; removed: int64 [S] on the CPU, r_k = floor(fraction_k * P)
    tokens removed per clip at step k (by="mass": int64 [S, B] on the CPU, a count per step and clip).  logits: fp32 [S, B, C], detached (logits_dist: the distillation head's, with
    distilled_type="separated"; else None); logit, prob: [S, B], the target label's logit and its sigmoid; auc: [B], the trapezoid of prob
    over the fractions divided by their span (None for a single step) -- small after a "positive" run and large after a "negative" one
    when the scores are faithful.  order, mode: as given; tokens: int32 [P, 2], (frequency patch, time patch) of the call's token sequence;
    target: int64 [B]."""

    def __init__(self, fractions, removed, logits, logit, prob, auc, order, mode, tokens, target, rank, logits_dist=None):
        self.fractions, self.removed, self.logits, self.logit, self.prob, self.auc = tuple(fractions), removed, logits, logit, prob, auc
        self.order, self.mode, self.tokens, self.target, self.logits_dist = order, mode, tokens, target, logits_dist
        self._rank = rank

    def keep_mask(self, step: int) -> torch.Tensor:
        """bool [B, P]: the tokens step `step` left in place with their content (mode "blank": the others stayed, with zeroed content)."""
        r = self.removed[step]
        return keep_mask_counts(self._rank, r) if r.dim() == 1 else keep_mask(self._rank, int(r))


# ------------------------------------------------------------------------------------------------ argument checks (before any launch of the model)
def take_options(method: str, given: dict, **defaults) -> dict:
    """The keywords a method takes through ``**options`` (MAEST.forward_tokens: ragged; MAEST.perturbation_curve: by) -> their values,
    defaults filled in; any other keyword is the TypeError Python raises for an unknown one."""
    for name in given:
        if name not in defaults:
            raise TypeError(f"{method}() got an unexpected keyword argument {name!r}")
    return dict(defaults, **given)


def _check_ragged(ragged):
    if not isinstance(ragged, bool):
        raise TypeError(f"ragged must be a bool, got {ragged!r}")


def _check_masks(keep, blank, ragged: bool = False):
    """The form and the values of the masks of forward_tokens -> the number of tokens every clip keeps (masks on a device: one sync).
    ragged: the rows of keep may hold different counts, each >= 1 -> (the largest count, the counts int64 [B] on keep's device -- None
    when they are all equal: such a call is the plain one)."""
    for name, m in (("keep", keep), ("blank", blank)):
        if m is None and name == "blank":
            continue
        if not torch.is_tensor(m):
            raise TypeError(f"{name} must be a bool tensor [B, P], got {type(m).__name__}")
        if m.dtype != torch.bool:
            raise TypeError(f"{name} must be a bool tensor [B, P], got dtype {m.dtype}")
        if m.dim() != 2:
            raise ValueError(f"{name} must be a bool tensor [B, P], got shape {tuple(m.shape)}")
    if blank is not None and blank.shape != keep.shape:
        raise ValueError(f"blank has shape {tuple(blank.shape)}, keep {tuple(keep.shape)}")
    if keep.numel() == 0:
        raise ValueError(f"keep must be a bool tensor [B, P] with B, P >= 1, got shape {tuple(keep.shape)}")
    counts = keep.sum(1)
    stray = (blank.to(keep.device) & ~keep).any() if blank is not None else torch.zeros((), dtype=torch.bool, device=keep.device)
    lo, hi, stray = (int(v) for v in torch.stack([counts.min(), counts.max(), stray.to(counts.dtype)]).cpu())
    if lo != hi and not ragged:
        raise ValueError(f"every clip must keep the same number of tokens: the rows of keep hold {lo} .. {hi}")
    if lo < 1:
        raise ValueError("keep removes every patch token" if not ragged else "keep removes every patch token of a clip: a row of keep holds no token")
    if stray:
        raise ValueError("blank must be a subset of keep")
    return (hi, counts if lo != hi else None) if ragged else lo


def _check_frames(frames, B: int, T: int) -> torch.Tensor:
    """frames of forward_lengths -> int64 [B] on the CPU."""
    if torch.is_tensor(frames):
        if frames.dtype not in _INT_DTYPES:
            raise TypeError(f"frames must be an integer tensor or a sequence of ints [B], got a {frames.dtype} tensor")
        fr = frames.detach().cpu().to(torch.int64)
    else:
        if isinstance(frames, (str, bytes)) or not hasattr(frames, "__iter__"):
            raise TypeError(f"frames must be an integer tensor or a sequence of ints [B], got {frames!r}")
        vals = list(frames)
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"frames must be an integer tensor or a sequence of ints [B], got an element {v!r}")
        fr = torch.tensor(vals, dtype=torch.int64)
    if tuple(fr.shape) != (B,):
        raise ValueError(f"frames has shape {tuple(fr.shape)}: this call has B = {B} clips, [B] wanted")
    if int(fr.min()) < PATCH or int(fr.max()) > T:
        raise ValueError(f"frames must lie in {PATCH} .. {T} (one patch .. the padded length), got {int(fr.min())} .. {int(fr.max())}")
    return fr


def _check_fractions(fractions):
    if fractions is None:
        return DEFAULT_FRACTIONS
    if isinstance(fractions, (str, bytes)) or not hasattr(fractions, "__iter__"):
        raise TypeError(f"fractions must be an iterable of floats in [0, 1), got {fractions!r}")
    fr = list(fractions)
    for f in fr:
        if isinstance(f, bool) or not isinstance(f, (int, float)):
            raise TypeError(f"fractions must be an iterable of floats in [0, 1), got an element {f!r}")
    fr = [float(f) for f in fr]
    if not fr:
        raise ValueError("fractions must name at least one step")
    if any(not 0.0 <= f < 1.0 for f in fr):      # (NaN fails both comparisons)
        raise ValueError(f"fractions must lie in [0, 1), got {fractions!r}")
    if any(b <= a for a, b in zip(fr, fr[1:])):
        raise ValueError(f"fractions must ascend, got {fractions!r}")
    return tuple(fr)


def _check_curve_target(target, C: int):
    """An int label index, or an integer tensor [B] of them."""
    if isinstance(target, bool) or not (isinstance(target, int) or torch.is_tensor(target)):
        raise TypeError(f"target must be an int label index or an integer tensor [B], got {target!r}")
    if isinstance(target, int):
        if not 0 <= target < C:
            raise ValueError(f"target = {target} out of range for {C} labels")
        return
    if target.dtype not in _INT_DTYPES:
        raise TypeError(f"target must be an int label index or an integer tensor [B], got a {target.dtype} tensor")
    if target.dim() != 1:
        raise ValueError(f"target: an integer tensor holds one label index per clip, [B]; got shape {tuple(target.shape)}")
    if target.numel() and not (0 <= int(target.min()) and int(target.max()) < C):
        raise ValueError(f"target holds a label index out of range for {C} labels")


def _check_scores(scores, row):
    """The form of `scores` -> its tensor [B, P] (None for "random") and the token sequence it was computed on (None: not known)."""
    if isinstance(row, bool) or not isinstance(row, int) or row < 0:
        raise ValueError(f"row must be a non-negative int, got {row!r}")
    if isinstance(scores, str):
        if scores != "random":
            raise ValueError(f"scores must be a float32 tensor [B, P], an AttentionRollout / AttentionRelevance or 'random', got {scores!r}")
        return None, None
    tokens = None
    if isinstance(scores, (AttentionRollout, AttentionRelevance)):
        full = scores.rollout if isinstance(scores, AttentionRollout) else scores.relevance
        if row >= full.shape[1]:
            raise ValueError(f"row = {row}: the result holds {full.shape[1]} rows")
        scores, tokens = full[:, row, 2:], scores.tokens
    elif not torch.is_tensor(scores):
        raise TypeError(f"scores must be a float32 tensor [B, P], an AttentionRollout / AttentionRelevance or 'random', got {type(scores).__name__}")
    if scores.dtype != torch.float32:
        raise TypeError(f"scores must be float32, got {scores.dtype}")
    if scores.dim() != 2:
        raise ValueError(f"scores must have shape [B, P], got {tuple(scores.shape)}")
    if not bool(torch.isfinite(scores).all()):
        raise ValueError("scores must be finite")
    return scores.detach(), tokens


# ------------------------------------------------------------------------------------------------ the forward
def _clip_table(tok: torch.Tensor, keep: torch.Tensor, blank, K: int, counts=None) -> torch.Tensor:
    """tok int32 [P, 2], keep / blank bool [B, P] with K kept tokens in every row -> int32 [B, K, 2]: per clip its kept tokens in
    ascending sequence order, the blank ones with TOK_BLANK in the f word.  counts (ragged batches; int [B], K their largest): clip b
    keeps counts[b] tokens, and the K - counts[b] slots behind them are pads: TOK_BLANK entries (of removed tokens, whose content is
    never read) that the attention does not see (MAEST_ATTN_LENS)."""
    idx = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :K]      # kept positions first, each group ascending
    table = tok[idx]
    if blank is not None:
        table[..., 0] |= blank.gather(1, idx).to(torch.int32) * TOK_BLANK
    if counts is not None:
        pad = torch.arange(K, device=idx.device).unsqueeze(0) >= counts.to(idx.device).unsqueeze(1)
        table[..., 0] |= pad.to(torch.int32) * TOK_BLANK
    return table.contiguous()


def _forward_resolved(model, x3, dt, kw, keep, blank, K, counts=None):
    """One evaluation forward of a resolved call (MAEST._resolve_call) on per-clip tokens: masks that passed _check_masks (or that the
    curve made itself), K kept tokens in every row -- or, counts (int [B], not all equal), counts[b] <= K of them in row b: the ragged
    forward, n_tok = 2 + counts."""
    tok = kw["tok_ft"]
    B, P = int(x3.shape[0]), int(tok.shape[0])
    if tuple(keep.shape) != (B, P):
        raise ValueError(f"keep has shape {tuple(keep.shape)}: this call has B = {B} clips of P = {P} patch tokens")
    keep = keep.to(tok.device)
    blank = None if blank is None else blank.to(tok.device)
    kw = dict(kw, tok_ft=_clip_table(tok, keep, blank, K, counts))
    if counts is not None:
        kw["n_tok"] = (counts.to(tok.device) + 2).to(torch.int32).contiguous()
    with torch.no_grad():
        return model._eval_forward(x3, dt, kw)


def forward_tokens(model, x, keep, blank, melspectrogram_input, *, _patchout, ragged=False):
    _check_ragged(ragged)
    K, counts = _check_masks(keep, blank, True) if ragged else (_check_masks(keep, blank), None)
    x3, dt, kw, _, _ = model._resolve_call(x, melspectrogram_input, None, _patchout, None, recording=False)
    return _forward_resolved(model, x3, dt, kw, keep, blank, K, counts)


def forward_lengths(model, x, frames):
    if not torch.is_tensor(x):
        raise TypeError(f"x must be a mel batch [B, F, T] or [B, 1, F, T], got {type(x).__name__}")
    if x.dim() in (1, 2):
        raise ValueError("forward_lengths takes mel batches [B, F, T] / [B, 1, F, T] only: the STFT's edge padding makes a padded waveform "
                         "differ from the clip alone (waveform input is not offered)")
    if x.dim() not in (3, 4):
        raise ValueError(f"x must be a mel batch [B, F, T] or [B, 1, F, T], got shape {tuple(x.shape)}")
    if model.training:
        raise ValueError("forward_lengths is an evaluation forward: call model.eval() first (training and gradients on ragged batches are "
                         "not offered)")
    fr = _check_frames(frames, int(x.shape[0]), int(x.shape[-1]))
    x3, dt, kw, _, _ = model._resolve_call(x, True, None, None, None, recording=False)
    tok = kw["tok_ft"]
    tp = frames_to_time_patches(fr, model.patch_embed.stride[1]).to(tok.device)
    keep = tok[:, 1].to(torch.int64).unsqueeze(0) < tp.unsqueeze(1)
    K, counts = _check_masks(keep, None, True)
    return _forward_resolved(model, x3, dt, kw, keep, None, K, counts)


def _fraction_steps(model, x3, dt, kw, rank, removed, mode, P):
    steps = []
    for r in removed:
        m = keep_mask(rank, r)
        if mode == "drop":
            steps.append(_forward_resolved(model, x3, dt, kw, m, None, K=P - r))
        else:
            steps.append(_forward_resolved(model, x3, dt, kw, torch.ones_like(m), ~m, K=P))
    return steps


def _check_mass_scores(scores):
    """by="mass": every score >= 0 and a positive sum in every clip."""
    if bool((scores < 0).any()):
        raise ValueError("by='mass' needs scores >= 0 (the mass of a clip is the sum of its scores)")
    if not bool((scores.to(torch.float64).sum(1) > 0).all()):
        raise ValueError("by='mass' needs a positive sum of scores in every clip")


def perturbation_curve(model, x, scores, target, order, fractions, mode, row, melspectrogram_input, *, seed, _patchout, by="fraction"):
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if not isinstance(by, str) or by not in BYS:
        raise ValueError(f"by must be one of {BYS}, got {by!r}")
    if by == "mass" and order != "positive":
        raise ValueError(f"by='mass' removes the highest scores first: order must be 'positive', got {order!r}")
    fractions = _check_fractions(fractions)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"seed must be an int, got {seed!r}")
    C = model.head[1].out_features
    _check_curve_target(target, C)
    scores, score_tokens = _check_scores(scores, row)
    if by == "mass" and scores is not None:
        _check_mass_scores(scores)
    x3, dt, kw, _, _ = model._resolve_call(x, melspectrogram_input, None, _patchout, None, recording=False)
    tok = kw["tok_ft"]
    dev = tok.device
    B, P = int(x3.shape[0]), int(tok.shape[0])
    if torch.is_tensor(target) and target.shape[0] != B:
        raise ValueError(f"target has shape {tuple(target.shape)}: this call has B = {B} clips")
    if scores is None:
        scores = random_scores(B, P, seed)
    if tuple(scores.shape) != (B, P):
        raise ValueError(f"scores have shape {tuple(scores.shape)}: this call has B = {B} clips of P = {P} patch tokens")
    if score_tokens is not None and not torch.equal(score_tokens.to(dev), tok):
        raise ValueError("the scores were computed on another token sequence than this call's (compare .tokens: patchout draws differ)")
    rank = removal_order(scores.to(dev), order)
    if by == "mass":
        _check_mass_scores(scores)      # (the "random" permutation of a single token sums to 0)
        removed = mass_removed_counts(scores.to(dev), rank, fractions)
        steps = []
        for r in removed:
            m = keep_mask_counts(rank, r)
            if mode == "drop":
                kept = P - r
                lo, hi = int(kept.min()), int(kept.max())
                steps.append(_forward_resolved(model, x3, dt, kw, m, None, K=hi, counts=kept if lo != hi else None))
            else:
                steps.append(_forward_resolved(model, x3, dt, kw, torch.ones_like(m), ~m, K=P))
        removed = removed.cpu()
    else:
        removed = removed_counts(fractions, P)
        steps = _fraction_steps(model, x3, dt, kw, rank, removed, mode, P)
        removed = torch.tensor(removed, dtype=torch.int64)
    logits = torch.stack([o[0] for o in steps])
    logits_dist = torch.stack([o[1] for o in steps]) if len(steps[0]) == 3 else None
    tgt = (torch.full((B,), target, dtype=torch.long) if isinstance(target, int) else target.detach().long()).to(dev)
    logit = logits.gather(2, tgt.reshape(1, B, 1).expand(len(steps), B, 1)).squeeze(2)
    prob = torch.sigmoid(logit)
    auc = trapezoid_auc(prob, fractions) if len(steps) > 1 else None
    return PerturbationCurve(fractions, removed, logits, logit, prob, auc, order, mode, tok, tgt, rank,
                             logits_dist=logits_dist)
