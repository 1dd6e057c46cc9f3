"""CPU (no kernel launches): the surface of the ragged batches -- the table of kept tokens with pad slots, the removal counts of
perturbation_curve(by="mass") on hand-made scores, frames -> time patches, every argument check of MAEST.forward_tokens(ragged=...),
MAEST.forward_lengths and by= (all of them before any launch), and the C ABI the feature must leave as it was (no new entry point, ABI 9;
one flag bit declared in the header and in _lib)."""
import inspect
import os
import re

import pytest
import torch

from maest_amd import _lib, ops, perturb
from maest_amd.maest import MAEST
from tests import guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P625 = 9 * 61     # patch tokens of a 625-frame clip
BLANK = _lib.TOK_BLANK


@pytest.fixture(scope="module")
def model():
    return MAEST(depth=3).eval()


def test_signatures():
    # ragged= and by= are keywords only; they come in through **options (the keyword-only lists of the two methods are pinned by
    # test_api_perturbation_cpu as they were), with their defaults, and no other keyword does
    for fn in (MAEST.forward_tokens, MAEST.perturbation_curve):
        assert list(inspect.signature(fn).parameters.values())[-1].kind is inspect.Parameter.VAR_KEYWORD
    assert perturb.take_options("forward_tokens", {}, ragged=False) == {"ragged": False}
    assert perturb.take_options("forward_tokens", {"ragged": True}, ragged=False) == {"ragged": True}
    assert perturb.take_options("perturbation_curve", {}, by="fraction") == {"by": "fraction"}
    net = MAEST(depth=1).eval()
    with pytest.raises(TypeError, match=r"forward_tokens\(\) got an unexpected keyword argument 'raged'"):
        net.forward_tokens(torch.rand(1, 96, 625), torch.ones(1, P625, dtype=torch.bool), raged=True)
    with pytest.raises(TypeError, match=r"perturbation_curve\(\) got an unexpected keyword argument 'By'"):
        net.perturbation_curve(torch.rand(1, 96, 625), torch.rand(1, P625), 3, By="mass")
    with pytest.raises(TypeError):
        net.forward_tokens(torch.rand(1, 96, 625), torch.ones(1, P625, dtype=torch.bool), None, False, True)      # not positional
    assert list(inspect.signature(MAEST.forward_lengths).parameters) == ["self", "x", "frames"]
    sig = inspect.signature(ops.attn_fwd).parameters
    assert list(sig)[-1] == "n_tok" and sig["n_tok"].default is None
    assert perturb.BYS == ("fraction", "mass")


def test_abi_is_unchanged_and_the_header_declares_the_flag():
    assert _lib.ABI_VERSION == 9 and len(_lib.SIGNATURES) == 52 and len(_lib.WRITTEN) == 47
    assert len(guard.device_entries()) == 47
    P, I, F = _lib._P, _lib._I, _lib._F
    assert _lib.SIGNATURES["maest_attn_fwd_rows"] == [P, P, P, I, I, I, F, I, P] and _lib.WRITTEN["maest_attn_fwd_rows"] == (1, 2)
    assert _lib.SIGNATURES["maest_attn_fwd"] == [P, P, P, I, I, I, F, P]
    hdr = open(os.path.join(REPO, "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
    assert int(re.search(r"^#define MAEST_ATTN_LENS (\w+)", hdr, flags=re.M).group(1), 0) == _lib.ATTN_LENS
    # a bit of its own: above every dtype code, beside the other flags of the attention entries, below the rows field
    lens = _lib.ATTN_LENS
    assert lens & (lens - 1) == 0 and 0xFF < lens < 0x10000
    others = [_lib.ATTN_PROBS, _lib.ATTN_PROBS_MEAN, _lib.ATTN_APPLY, _lib.ATTN_APPLY_GRAD, _lib.ATTN_APPLY_HEADS]
    assert all(lens & f == 0 for f in others) and all(_lib.attn_apply_rows(r) & lens == 0 for r in range(1, 9))
    flags = re.findall(r"^#define MAEST_ATTN_(\w+) (0x\w+)", hdr, flags=re.M)
    assert sorted(int(v, 0) for _, v in flags) == sorted(others + [lens])
    # the header declares exactly the entry points of _lib.SIGNATURES (and the two that report the version and the last error)
    assert set(re.findall(r"^\w[\w \*]*?\b(maest_\w+)\(", hdr, flags=re.M)) - {"maest_version", "maest_last_error"} == set(_lib.SIGNATURES)


# ------------------------------------------------------------------------------------------------ the table
def test_clip_table_with_pad_slots():
    tok = torch.tensor([[f, t] for f in range(2) for t in range(3)], dtype=torch.int32)      # P = 6
    keep = torch.tensor([[0, 1, 0, 1, 1, 0], [0, 0, 0, 0, 1, 0], [1, 1, 1, 1, 1, 1]], dtype=torch.bool)
    blank = torch.tensor([[0, 0, 0, 1, 0, 0], [0] * 6, [1, 0, 0, 0, 0, 0]], dtype=torch.bool)
    K, counts = perturb._check_masks(keep, blank, True)
    assert K == 6 and counts.tolist() == [3, 1, 6]
    table = perturb._clip_table(tok, keep, blank, K, counts)
    assert table.dtype == torch.int32 and table.shape == (3, 6, 2) and table.is_contiguous()
    f, t = table[..., 0], table[..., 1]
    # kept tokens first, in ascending sequence order, the blank ones marked
    assert (f[0, :3] & ~BLANK).tolist() == [0, 1, 1] and t[0, :3].tolist() == [1, 0, 1] and (f[0, :3] & BLANK != 0).tolist() == [False, True, False]
    assert (f[1, 0].item(), t[1, 0].item()) == (1, 1)
    assert (f[2] & ~BLANK).tolist() == [0, 0, 0, 1, 1, 1] and (f[2] & BLANK != 0).tolist() == [True] + [False] * 5
    # the slots behind them: TOK_BLANK entries of tokens inside the grid
    assert bool((f[0, 3:] & BLANK != 0).all()) and bool((f[1, 1:] & BLANK != 0).all())
    pads = torch.cat([table[0, 3:], table[1, 1:]])
    assert bool(((pads[:, 0] & ~BLANK) < 2).all()) and bool(((pads[:, 1] >= 0) & (pads[:, 1] < 3)).all())
    # equal counts: no counts come back, and the table is the plain call's
    keep2 = torch.tensor([[1, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1, 0]], dtype=torch.bool)
    K2, c2 = perturb._check_masks(keep2, None, True)
    assert (K2, c2) == (2, None) and perturb._check_masks(keep2, None) == 2
    assert torch.equal(perturb._clip_table(tok, keep2, None, 2, None), perturb._clip_table(tok, keep2, None, 2))
    with pytest.raises(ValueError, match="same number of tokens: the rows of keep hold 1 .. 6"):
        perturb._check_masks(keep, blank)


# ------------------------------------------------------------------------------------------------ by="mass"
def _counts(scores, fractions):
    s = torch.tensor(scores, dtype=torch.float32)
    return perturb.mass_removed_counts(s, perturb.removal_order(s, "positive"), fractions).tolist()


def test_mass_counts_on_hand_made_scores():
    fr = (0.0, 0.25, 0.5, 0.75, 0.9)
    # clip 0: 4, 3, 2, 1 of 10 -> prefix sums 4, 7, 9, 10;  clip 1: everything in one token;  clip 2: four equal scores (a tie)
    got = _counts([[1, 4, 2, 3], [0, 0, 8, 0], [2, 2, 2, 2]], fr)
    assert got == [[0, 0, 0], [1, 1, 1], [2, 1, 2], [3, 1, 3], [3, 1, 3]]      # (0.9: clips 0 and 2 need all four -- capped at P - 1 = 3)
    assert perturb.mass_removed_counts(torch.ones(1, 4), torch.arange(4).reshape(1, 4), (0.5,)).dtype == torch.int64
    # the tie leaves in ascending token index, and keep_mask_counts follows the counts per clip
    s = torch.tensor([[1, 4, 2, 3], [0, 0, 8, 0], [2, 2, 2, 2]], dtype=torch.float32)
    rank = perturb.removal_order(s, "positive")
    m = perturb.keep_mask_counts(rank, torch.tensor([2, 1, 2]))
    assert m.tolist() == [[True, False, True, False], [True, True, False, True], [False, False, True, True]]
    assert torch.equal(perturb.keep_mask_counts(rank, torch.tensor([2, 2, 2])), perturb.keep_mask(rank, 2))
    assert bool(perturb.keep_mask_counts(rank, torch.zeros(3, dtype=torch.int64)).all())
    with pytest.raises(ValueError, match="counts in 0 .. 4"):
        perturb.keep_mask_counts(rank, torch.tensor([5, 0, 0]))
    # an exact threshold: 0.7 x 10 is reached by the first two (4 + 3 = 7 >= fp64(0.7) * 10)
    assert _counts([[1, 4, 2, 3]], (0.7,)) == [[2]] and _counts([[1, 4, 2, 3]], (0.71,)) == [[3]]


def test_curve_result_follows_the_counts():
    rank = perturb.removal_order(torch.tensor([[1.0, 4, 2, 3], [5, 0, 0, 0]]), "positive")
    removed = torch.tensor([[0, 0], [2, 1]])
    c = perturb.PerturbationCurve((0.0, 0.5), removed, None, None, None, None, "positive", "drop", None, None, rank)
    assert bool(c.keep_mask(0).all()) and c.keep_mask(1).tolist() == [[True, False, True, False], [False, True, True, True]]
    c1 = perturb.PerturbationCurve((0.0, 0.5), torch.tensor([0, 2]), None, None, None, None, "positive", "drop", None, None, rank)
    assert c1.keep_mask(1).tolist() == [[True, False, True, False], [False, False, True, True]]


# ------------------------------------------------------------------------------------------------ frames
def test_frames_to_time_patches():
    fr = torch.tensor([16, 25, 26, 100, 256, 625])
    assert perturb.frames_to_time_patches(fr, 10).tolist() == [1, 1, 2, 9, 25, 61]
    assert perturb.frames_to_time_patches(fr, 16).tolist() == [1, 1, 1, 6, 16, 39]
    assert perturb._check_frames([16, 625], 2, 625).tolist() == [16, 625]
    assert perturb._check_frames(torch.tensor([20, 30], dtype=torch.int32), 2, 625).dtype == torch.int64


# ------------------------------------------------------------------------------------------------ argument checks, before any launch
@pytest.mark.parametrize("frames,exc,match", [
    (None, TypeError, "frames must be an integer tensor or a sequence"),
    ("12", TypeError, "frames must be an integer tensor or a sequence"),
    (torch.tensor([100.0, 200.0]), TypeError, "got a torch.float32 tensor"),
    ([100, 200.0], TypeError, "got an element 200.0"),
    ([100, True], TypeError, "got an element True"),
    ([100], ValueError, r"frames has shape \(1,\)"),
    (torch.tensor([[100, 200]]), ValueError, r"frames has shape \(1, 2\)"),
    ([15, 200], ValueError, "frames must lie in 16 .. 625"),
    ([100, 626], ValueError, "frames must lie in 16 .. 625"),
])
def test_forward_lengths_refuses_bad_frames_before_any_launch(model, frames, exc, match):
    """On a CPU model every launch raises MaestHipError: an argument error that surfaces first was raised before any device work."""
    with pytest.raises(exc, match=match):
        model.forward_lengths(torch.rand(2, 96, 625), frames)


def test_forward_lengths_refuses_audio_and_training(model):
    for x in (torch.rand(16000), torch.rand(2, 16000)):
        with pytest.raises(ValueError, match="waveform input is not offered"):
            model.forward_lengths(x, [100, 200])
    with pytest.raises(ValueError, match="got shape"):
        model.forward_lengths(torch.rand(2, 1, 1, 96, 625), [100, 200])
    with pytest.raises(TypeError, match="mel batch"):
        model.forward_lengths([1.0], [100])
    train = MAEST(depth=1).train()
    with pytest.raises(ValueError, match="model.eval"):
        train.forward_lengths(torch.rand(2, 96, 625), [100, 200])
    # good arguments reach the device work, which a CPU model refuses
    with pytest.raises(_lib.MaestHipError, match="MI355X only"):
        model.forward_lengths(torch.rand(2, 96, 625), [100, 200])


@pytest.mark.parametrize("ragged", [None, 1, "yes", 0])
def test_ragged_must_be_a_bool(model, ragged):
    with pytest.raises(TypeError, match="ragged must be a bool"):
        model.forward_tokens(torch.rand(1, 96, 625), torch.ones(1, P625, dtype=torch.bool), ragged=ragged)


def test_ragged_masks(model):
    x = torch.rand(2, 96, 625)
    keep = torch.ones(2, P625, dtype=torch.bool)
    keep[1] = False
    with pytest.raises(ValueError, match="a row of keep holds no token"):
        model.forward_tokens(x, keep, ragged=True)
    keep[1, 5] = True
    blank = torch.zeros_like(keep)
    blank[1, 6] = True
    with pytest.raises(ValueError, match="blank must be a subset of keep"):
        model.forward_tokens(x, keep, blank, ragged=True)
    with pytest.raises(ValueError, match="same number of tokens: the rows of keep hold 1 .. 549"):
        model.forward_tokens(x, keep)                      # ragged=False stays the pinned error
    with pytest.raises(_lib.MaestHipError, match="MI355X only"):
        model.forward_tokens(x, keep, ragged=True)         # different counts pass the checks


@pytest.mark.parametrize("kw,exc,match", [
    (dict(by="rank"), ValueError, "by must be one of"),
    (dict(by=None), ValueError, "by must be one of"),
    (dict(by=0.5), ValueError, "by must be one of"),
    (dict(by="mass", order="negative"), ValueError, "order must be 'positive'"),
    (dict(by="mass", mode="zero"), ValueError, "mode must be one of"),
    (dict(by="mass", scores=-torch.rand(1, P625)), ValueError, "needs scores >= 0"),
    (dict(by="mass", scores=torch.zeros(1, P625)), ValueError, "positive sum of scores in every clip"),
    (dict(by="mass", scores=torch.cat([torch.rand(1, P625), torch.zeros(1, P625)])), ValueError, "positive sum of scores in every clip"),
])
def test_curve_by_refuses_bad_arguments_before_any_launch(model, kw, exc, match):
    a = dict(scores=torch.rand(1, P625), target=3)
    a.update(kw)
    with pytest.raises(exc, match=match):
        model.perturbation_curve(torch.rand(a["scores"].shape[0], 96, 625), **a)


def test_engine_refuses_counts_without_a_table_and_with_saved_activations(model):
    eng = model._engine
    x3 = torch.rand(2, 96, 625)
    tok = torch.zeros(P625, 2, dtype=torch.int32)
    n = torch.tensor([5, 7], dtype=torch.int32)
    kw = dict(toffset=0, perm=None, lam=None)
    with pytest.raises(ValueError, match="go with a table of kept tokens per clip"):
        eng._forward(x3, torch.float32, tok_ft=tok, n_tok=n, **kw)
    table = torch.zeros(2, 9, 2, dtype=torch.int32)
    for bad in (dict(save=True), dict(stop_block=1), dict(tap=lambda *a: None), dict(tap_x=lambda *a: None)):
        with pytest.raises(ValueError, match="serves forwards that save nothing"):
            eng._forward(x3, torch.float32, tok_ft=table, n_tok=n, **kw, **bad)
    with pytest.raises(ValueError, match=r"n_tok must be an int32 tensor \[2\]"):
        eng._forward(x3, torch.float32, tok_ft=table, n_tok=n.long(), **kw)
    with pytest.raises(ValueError, match=r"n_tok must be an int32 tensor \[2\]"):
        eng._forward(x3, torch.float32, tok_ft=table, n_tok=n[:1], **kw)
