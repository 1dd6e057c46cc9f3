"""CPU (no kernel launches): the surface of the perturbation curves -- the signatures of MAEST.forward_tokens / MAEST.perturbation_curve,
their argument checks (all of them before any launch), the ranking and mask helper against a numpy stable sort, the "random" ranking,
the area under a hand-made curve, and the C ABI the feature must leave as it was (no new entry point, ABI 9; one flag and one table bit
declared in the header and in _lib)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from maest_amd import _lib, ops, perturb
from maest_amd.maest import MAEST, AttentionRollout, PerturbationCurve
from tests import guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty
P625 = 9 * 61     # patch tokens of a 625-frame clip


@pytest.fixture(scope="module")
def model():
    return MAEST(depth=3).eval()


def _params(fn):
    sig = inspect.signature(fn)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    kwo = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY]
    return pos, kwo


def test_signatures_and_defaults():
    pos, kwo = _params(MAEST.forward_tokens)
    assert pos == [("self", E), ("x", E), ("keep", E), ("blank", None), ("melspectrogram_input", False)]
    assert kwo == [("_patchout", None)]
    pos, kwo = _params(MAEST.perturbation_curve)
    assert pos == [("self", E), ("x", E), ("scores", E), ("target", E), ("order", "positive"), ("fractions", None), ("mode", "drop"), ("row", 0),
                   ("melspectrogram_input", False)]
    assert kwo == [("seed", 0), ("_patchout", None)]
    assert perturb.DEFAULT_FRACTIONS == (0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
    assert perturb.ORDERS == ("positive", "negative") and perturb.MODES == ("drop", "blank")
    # MAEST.forward keeps its signature
    pos, kwo = _params(MAEST.forward)
    assert [n for n, _ in pos] == ["self", "x", "transformer_block", "return_self_attention", "melspectrogram_input"]
    assert [n for n, _ in kwo] == ["_mixup", "_patchout", "_specmask"]
    assert list(inspect.signature(ops.patch_im2col).parameters) == ["x", "tok_ft", "dtype", "perm", "lam", "t_stripes", "f_stripes", "stride"]


def test_abi_is_unchanged_and_the_header_declares_the_form():
    assert _lib.ABI_VERSION == 9 and len(_lib.SIGNATURES) == 52 and len(_lib.WRITTEN) == 47
    assert len(guard.device_entries()) == 47
    P, I = _lib._P, _lib._I
    assert _lib.SIGNATURES["maest_patch_im2col_strided"] == [P, I, I, I, I, I, I, P, P, P, I, P, I, P, I, P, I, P]
    assert _lib.SIGNATURES["maest_patch_im2col"] == [P, I, I, I, I, P, P, P, I, P, I, P, I, P, I, P]
    assert _lib.WRITTEN["maest_patch_im2col_strided"] == (15,) and _lib.WRITTEN["maest_patch_im2col"] == (13,)
    assert _lib.SIGNATURES["maest_token_assemble"] == [P, P, P, P, P, P, I, I, I, P, I, I, P, P]
    hdr = open(os.path.join(REPO, "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
    assert int(re.search(r"^#define MAEST_IM2COL_CLIP_TOKENS (\w+)", hdr, flags=re.M).group(1), 0) == _lib.IM2COL_CLIP_TOKENS == 0x100
    assert int(re.search(r"^#define MAEST_TOK_BLANK (\w+)", hdr, flags=re.M).group(1), 0) == _lib.TOK_BLANK == 0x40000000
    codes = [int(v) for v in re.findall(r"^#define MAEST_(?:F32|BF16|F32X3|F16|BF16_QS|SPLIT3_A|SPLIT3_B|F32X3_A3) (\d+)", hdr, flags=re.M)]
    assert len(codes) == 8 and max(codes) < 0x80 < _lib.IM2COL_CLIP_TOKENS      # the flag above every dtype code, above bit 7
    assert all(c & _lib.IM2COL_CLIP_TOKENS == 0 for c in codes)
    assert 0 < _lib.TOK_BLANK < 2 ** 31 and _lib.TOK_BLANK > 32767      # a positive int32 above every patch index


def _keep(B=1, P=P625, n=None):
    k = torch.ones(B, P, dtype=torch.bool)
    if n is not None:
        k[:, n:] = False
    return k


def _some(P=P625):
    b = torch.zeros(1, P, dtype=torch.bool)
    b[0, 3] = True
    return b


@pytest.mark.parametrize("keep,blank,exc,match", [
    (None, None, TypeError, "keep must be a bool tensor"),
    ([[True]], None, TypeError, "keep must be a bool tensor"),
    (torch.ones(1, P625), None, TypeError, "got dtype torch.float32"),
    (torch.ones(1, P625, dtype=torch.uint8), None, TypeError, "got dtype torch.uint8"),
    (torch.ones(P625, dtype=torch.bool), None, ValueError, "got shape"),
    (_keep(), torch.ones(1, P625), TypeError, "blank must be a bool tensor"),
    (_keep(), "all", TypeError, "blank must be a bool tensor"),
    (_keep(), torch.zeros(1, 5, dtype=torch.bool), ValueError, "blank has shape"),
    (torch.zeros(1, 0, dtype=torch.bool), None, ValueError, "B, P >= 1"),
    (torch.zeros(1, P625, dtype=torch.bool), None, ValueError, "removes every patch token"),
    (torch.cat([_keep(n=5), _keep(n=6)]), None, ValueError, "same number of tokens: the rows of keep hold 5 .. 6"),
    (_keep(n=3), _some(), ValueError, "blank must be a subset of keep"),
])
def test_forward_tokens_refuses_bad_masks_before_any_launch(model, keep, blank, exc, match):
    """On a CPU model every launch raises MaestHipError: an argument error that surfaces first was raised before any device work."""
    x = torch.rand(1 if not torch.is_tensor(keep) or keep.dim() < 2 else keep.shape[0], 96, 625)
    with pytest.raises(exc, match=match):
        model.forward_tokens(x, keep, blank)


def _curve_args(**kw):
    a = dict(scores=torch.rand(1, P625), target=3)
    a.update(kw)
    return a


def _rollout(r):
    return AttentionRollout(r, torch.zeros(1, 400), torch.zeros(1, 768), torch.zeros(P625, 2, dtype=torch.int32), (9, 61))


@pytest.mark.parametrize("kw,exc,match", [
    (dict(order="highest"), ValueError, "order must be one of"),
    (dict(order=None), ValueError, "order must be one of"),
    (dict(mode="zero"), ValueError, "mode must be one of"),
    (dict(fractions=0.5), TypeError, "fractions must be an iterable"),
    (dict(fractions="0.5"), TypeError, "fractions must be an iterable"),
    (dict(fractions=["a"]), TypeError, "got an element 'a'"),
    (dict(fractions=[True]), TypeError, "got an element True"),
    (dict(fractions=()), ValueError, "at least one step"),
    (dict(fractions=(0.0, 1.0)), ValueError, r"must lie in \[0, 1\)"),
    (dict(fractions=(-0.1, 0.5)), ValueError, r"must lie in \[0, 1\)"),
    (dict(fractions=(0.0, float("nan"))), ValueError, r"must lie in \[0, 1\)"),
    (dict(fractions=(0.5, 0.2)), ValueError, "must ascend"),
    (dict(fractions=(0.2, 0.2)), ValueError, "must ascend"),
    (dict(seed=0.5), TypeError, "seed must be an int"),
    (dict(seed=True), TypeError, "seed must be an int"),
    (dict(target=400), ValueError, "out of range for 400 labels"),
    (dict(target=-1), ValueError, "out of range for 400 labels"),
    (dict(target=True), TypeError, "target must be an int label index"),
    (dict(target=1.0), TypeError, "target must be an int label index"),
    (dict(target=torch.tensor([0.5])), TypeError, "integer tensor"),
    (dict(target=torch.tensor([[1]])), ValueError, "one label index per clip"),
    (dict(target=torch.tensor([400])), ValueError, "label index out of range"),
    (dict(row=-1), ValueError, "row must be a non-negative int"),
    (dict(row=1.0), ValueError, "row must be a non-negative int"),
    (dict(scores="shuffled"), ValueError, "or 'random', got 'shuffled'"),
    (dict(scores=None), TypeError, "scores must be a float32 tensor"),
    (dict(scores=[[0.5]]), TypeError, "scores must be a float32 tensor"),
    (dict(scores=torch.rand(1, P625).double()), TypeError, "scores must be float32"),
    (dict(scores=torch.rand(P625)), ValueError, r"shape \[B, P\]"),
    (dict(scores=torch.full((1, P625), float("nan"))), ValueError, "scores must be finite"),
    (dict(scores=torch.full((1, P625), float("inf"))), ValueError, "scores must be finite"),
    (dict(scores=_rollout(torch.rand(1, 2, 2 + P625)), row=2), ValueError, "the result holds 2 rows"),
    (dict(scores=_rollout(torch.full((1, 2, 2 + P625), float("nan")))), ValueError, "scores must be finite"),
])
def test_perturbation_curve_refuses_bad_arguments_before_any_launch(model, kw, exc, match):
    with pytest.raises(exc, match=match):
        model.perturbation_curve(torch.rand(1, 96, 625), **_curve_args(**kw))


def test_sound_arguments_reach_the_device_and_there_is_no_cpu_fallback(model):
    x = torch.rand(1, 96, 625)
    for kw in (dict(), dict(scores="random", seed=7), dict(order="negative", mode="blank", fractions=[0.0, 0.5]),
               dict(scores=_rollout(torch.rand(1, 2, 2 + P625)), row=1), dict(target=torch.tensor([5]))):
        with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
            model.perturbation_curve(x, **_curve_args(**kw))
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        model.forward_tokens(x, _keep(n=100), _some())
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        ops.patch_im2col(torch.zeros(1, 96, 64), torch.zeros(1, 1, 2, dtype=torch.int32), torch.float32)


def test_the_engine_refuses_per_clip_tables_where_something_is_saved(model):
    tok = torch.zeros(1, 4, 2, dtype=torch.int32)
    x3 = torch.zeros(1, 96, 64)
    base = dict(toffset=0, tok_ft=tok, perm=None, lam=None)
    for kw in (dict(save=True), dict(tap=lambda *a: None), dict(tap_x=lambda *a: None), dict(stop_block=1)):
        with pytest.raises(ValueError, match="forwards that save nothing"):
            model._engine._forward(x3, torch.float32, **base, **kw)
    with pytest.raises(ValueError, match=r"\[B, P, 2\] wanted"):
        model._engine._forward(torch.zeros(2, 96, 64), torch.float32, **base)


# ---------------------------------------------------------------------------------------------- the ranking helper
def _np_order(s, order):
    return np.stack([np.argsort(-r if order == "positive" else r, kind="stable") for r in s])


def _scores_with_ties():
    rng = np.random.Generator(np.random.PCG64(5))
    s = rng.integers(0, 6, (4, 37)).astype(np.float32)      # six levels over 37 tokens: every level is a tie
    s[1] = 2.0                                              # one clip is all one tie
    s[2, ::3] = -0.0                                        # signed zeros are one level
    s[2, 1::3] = 0.0
    s[3] = rng.standard_normal(37).astype(np.float32)       # and one without ties
    return s


@pytest.mark.parametrize("order", ["positive", "negative"])
def test_removal_order_is_a_stable_sort_with_ties_by_ascending_index(order):
    s = _scores_with_ties()
    rank = perturb.removal_order(torch.from_numpy(s), order)
    want = _np_order(s, order)
    assert rank.dtype == torch.int64 and np.array_equal(rank.numpy(), want)
    assert rank[1].tolist() == list(range(37))              # all equal: ascending token index, in both orders
    B, P = s.shape
    for r in (0, 1, 17, P - 1, P):
        keep = perturb.keep_mask(rank, r)
        assert keep.dtype == torch.bool and keep.shape == (B, P) and keep.sum(1).tolist() == [P - r] * B
        for b in range(B):
            assert sorted(np.flatnonzero(~keep[b].numpy()).tolist()) == sorted(want[b, :r].tolist())
    assert bool(perturb.keep_mask(rank, 0).all()) and int(perturb.keep_mask(rank, P - 1).sum()) == B
    for bad in (-1, P + 1):
        with pytest.raises(ValueError, match="outside 0"):
            perturb.keep_mask(rank, bad)
    with pytest.raises(ValueError, match="order must be one of"):
        perturb.removal_order(torch.from_numpy(s), "random")


def test_positive_and_negative_kept_sets_partition_the_tokens():
    """Removing the r highest and removing the P - r lowest keep complementary sets.  On distinct scores: the tie rule (ascending token
    index in BOTH orders) hands a tie that straddles the cut to both runs' removals by its low indices, so there the two kept sets share the
    tie's high indices instead -- the second half of the test."""
    rng = np.random.Generator(np.random.PCG64(6))
    s = torch.from_numpy(np.stack([rng.permutation(41) for _ in range(3)]).astype(np.float32))
    pos, neg = perturb.removal_order(s, "positive"), perturb.removal_order(s, "negative")
    assert torch.equal(pos, neg.flip(1))
    for r in (0, 1, 20, 40, 41):
        a, b = perturb.keep_mask(pos, r), perturb.keep_mask(neg, 41 - r)
        assert bool((a ^ b).all()), r
    tie = torch.zeros(1, 4)
    a, b = perturb.keep_mask(perturb.removal_order(tie, "positive"), 2), perturb.keep_mask(perturb.removal_order(tie, "negative"), 2)
    assert a.tolist() == b.tolist() == [[False, False, True, True]]


def test_removed_counts_are_the_floor():
    assert perturb.removed_counts((0.0, 0.2, 0.5, 0.8), 225) == [0, 45, 112, 180]
    assert perturb.removed_counts(perturb.DEFAULT_FRACTIONS, 558) == [0, 55, 111, 167, 223, 279, 334, 390, 446, 502]
    assert perturb.removed_counts((0.999,), 7) == [6] and perturb.removed_counts((0.0,), 1) == [0]


def test_random_scores_are_reproducible_permutations():
    a, b, c = perturb.random_scores(3, 50, 11), perturb.random_scores(3, 50, 11), perturb.random_scores(3, 50, 12)
    assert a.dtype == torch.float32 and a.shape == (3, 50) and torch.equal(a, b) and not torch.equal(a, c)
    assert all(sorted(r.tolist()) == list(range(50)) for r in a) and not torch.equal(a[0], a[1])
    gen = torch.Generator(device="cpu").manual_seed(11)
    assert torch.equal(a[0], torch.randperm(50, generator=gen).float())


def test_auc_on_a_hand_made_curve_and_the_result_object():
    fr = (0.0, 0.25, 0.5, 0.9)
    prob = torch.tensor([[1.0, 0.5], [0.5, 0.5], [0.5, 0.5], [0.0, 0.5]])
    # clip 0: 0.25 * 0.75 + 0.25 * 0.5 + 0.4 * 0.25 = 0.4125, over a span of 0.9; clip 1: constant
    auc = perturb.trapezoid_auc(prob, fr)
    assert auc.dtype == torch.float32 and torch.allclose(auc, torch.tensor([0.4125 / 0.9, 0.5]), rtol=1e-6, atol=0)
    rank = perturb.removal_order(torch.tensor([[0.1, 0.9, 0.5, 0.5], [4.0, 3.0, 2.0, 1.0]]), "positive")
    tokens = torch.zeros(4, 2, dtype=torch.int32)
    c = PerturbationCurve(fr, torch.tensor([0, 1, 2, 3]), torch.zeros(4, 2, 400), torch.zeros(4, 2), prob, auc, "positive", "drop", tokens,
                          torch.tensor([3, 3]), rank)
    assert c.fractions == fr and c.logits_dist is None and c.order == "positive" and c.mode == "drop" and c.tokens is tokens
    assert c.keep_mask(0).all() and c.keep_mask(2).tolist() == [[True, False, False, True], [False, False, True, True]]
    assert c.keep_mask(3).tolist() == [[True, False, False, False], [False, False, False, True]]
