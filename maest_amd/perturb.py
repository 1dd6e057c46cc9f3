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
    tokens removed per clip at step k.  logits: fp32 [S, B, C], detached (logits_dist: the distillation head's, with
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
        return keep_mask(self._rank, int(self.removed[step]))


# ------------------------------------------------------------------------------------------------ argument checks (before any launch of the model)
def _check_masks(keep, blank) -> int:
    """The form and the values of the masks of forward_tokens -> the number of tokens every clip keeps (masks on a device: one sync)."""
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
    if lo != hi:
        raise ValueError(f"every clip must keep the same number of tokens: the rows of keep hold {lo} .. {hi}")
    if lo < 1:
        raise ValueError("keep removes every patch token")
    if stray:
        raise ValueError("blank must be a subset of keep")
    return lo


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
def _clip_table(tok: torch.Tensor, keep: torch.Tensor, blank, K: int) -> torch.Tensor:
    """tok int32 [P, 2], keep / blank bool [B, P] with K kept tokens in every row -> int32 [B, K, 2]: per clip its kept tokens in
    ascending sequence order, the blank ones with TOK_BLANK in the f word."""
    idx = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :K]      # kept positions first, each group ascending
    table = tok[idx]
    if blank is not None:
        table[..., 0] |= blank.gather(1, idx).to(torch.int32) * TOK_BLANK
    return table.contiguous()


def _forward_resolved(model, x3, dt, kw, keep, blank, K):
    """One evaluation forward of a resolved call (MAEST._resolve_call) on per-clip tokens: masks that passed _check_masks (or that the
    curve made itself), K kept tokens in every row."""
    tok = kw["tok_ft"]
    B, P = int(x3.shape[0]), int(tok.shape[0])
    if tuple(keep.shape) != (B, P):
        raise ValueError(f"keep has shape {tuple(keep.shape)}: this call has B = {B} clips of P = {P} patch tokens")
    keep = keep.to(tok.device)
    blank = None if blank is None else blank.to(tok.device)
    with torch.no_grad():
        return model._eval_forward(x3, dt, dict(kw, tok_ft=_clip_table(tok, keep, blank, K)))


def forward_tokens(model, x, keep, blank, melspectrogram_input, *, _patchout):
    K = _check_masks(keep, blank)
    x3, dt, kw, _, _ = model._resolve_call(x, melspectrogram_input, None, _patchout, None, recording=False)
    return _forward_resolved(model, x3, dt, kw, keep, blank, K)


def perturbation_curve(model, x, scores, target, order, fractions, mode, row, melspectrogram_input, *, seed, _patchout):
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    fractions = _check_fractions(fractions)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"seed must be an int, got {seed!r}")
    C = model.head[1].out_features
    _check_curve_target(target, C)
    scores, score_tokens = _check_scores(scores, row)
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
    removed = removed_counts(fractions, P)
    steps = []
    for r in removed:
        m = keep_mask(rank, r)
        if mode == "drop":
            steps.append(_forward_resolved(model, x3, dt, kw, m, None, K=P - r))
        else:
            steps.append(_forward_resolved(model, x3, dt, kw, torch.ones_like(m), ~m, K=P))
    logits = torch.stack([o[0] for o in steps])
    logits_dist = torch.stack([o[1] for o in steps]) if len(steps[0]) == 3 else None
    tgt = (torch.full((B,), target, dtype=torch.long) if isinstance(target, int) else target.detach().long()).to(dev)
    logit = logits.gather(2, tgt.reshape(1, B, 1).expand(len(steps), B, 1)).squeeze(2)
    prob = torch.sigmoid(logit)
    auc = trapezoid_auc(prob, fractions) if len(steps) > 1 else None
    return PerturbationCurve(fractions, torch.tensor(removed, dtype=torch.int64), logits, logit, prob, auc, order, mode, tok, tgt, rank,
                             logits_dist=logits_dist)
