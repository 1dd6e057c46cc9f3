"""GPU (`-m gpu`): ragged batches -- MAEST.forward_tokens(ragged=True), MAEST.forward_lengths and perturbation_curve(by="mass") -- on the
three-block model and the two 256-frame clips of tests/test_attention_heads_gpu.py (a 9 x 25 patch grid, P = 225), in every precision of its
PRECISIONS.

The reference is test_perturbation_gpu.oracle_clip, the oracle composed on the CPU clip by clip on the clip's own kept tokens, at that
module's gates (rel_err < 1e-3 in "fp32" / "auto"; the 16-bit modes within 3e-2 of the "fp32" model on the same ragged batch); for
forward_lengths the model itself on the clip alone, cut to its own frames.  The kept sets come from a seeded numpy permutation per clip,
the removal counts of by="mass" from a numpy stable sort and float64 cumulative sums made here, not read from the result."""
import functools

import numpy as np
import pytest
import torch

from maest_amd.maest import PerturbationCurve
from tests import test_attention_heads_gpu as AH
from tests import test_perturbation_gpu as PT
from tests.test_model_gpu import rel_err

pytestmark = pytest.mark.gpu
P = PT.P
CLASS = AH.CLASS
PRECISIONS = AH.PRECISIONS
gate = PT.gate
# kept patch tokens of (clip 0, clip 1): N = 2 + count in {227, 3, 128, 32, 129, 33, 64, 65}
PAIRS = [(225, 1), (126, 30), (127, 31), (62, 63)]
FRACTIONS = (0.0, 0.2, 0.5, 0.8)


def kept(b, count):
    """The ascending list of the `count` tokens clip b keeps: the head of a seeded permutation."""
    return sorted(np.random.Generator(np.random.PCG64(620 + b)).permutation(P)[:count].tolist())


def masks(pair):
    return PT._mask([kept(b, c) for b, c in enumerate(pair)])


@functools.lru_cache(maxsize=None)
def oracle(b, count):
    """(logits, features) of clip b on its kept tokens; computed once, shared, never modified."""
    return PT.oracle_clip(b, kept(b, count))


@functools.lru_cache(maxsize=None)
def fp32_ragged(pair):
    """The "fp32" model on the same ragged batch: the reference of the 16-bit modes."""
    return tuple(o.cpu() for o in AH.make("fp32").forward_tokens(AH.mel(), masks(pair), ragged=True))


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_forward_tokens_against_the_oracle(precision, pair):
    net = AH.make(precision)
    seen = []
    inner = net._engine.forward
    net._engine.forward = lambda *a, **kw: (seen.append((tuple(kw["tok_ft"].shape), kw["n_tok"].tolist())), inner(*a, **kw))[1]
    out = net.forward_tokens(AH.mel(), masks(pair), ragged=True)
    assert seen == [((2, max(pair), 2), [2 + pair[0], 2 + pair[1]])], seen      # one forward at the longest clip's length, with the counts
    assert len(out) == 2 and out[0].shape == (2, 400) and out[1].shape == (2, 768) and not out[0].requires_grad
    for b, count in enumerate(pair):
        want = oracle(b, count) if precision in ("fp32", "auto") else tuple(o[b] for o in fp32_ragged(pair))
        for name, got, ref in (("logits", out[0], want[0]), ("features", out[-1], want[-1])):
            e = rel_err(got[b].cpu(), ref)
            print(f"  {precision} counts {pair} clip {b} (N = {2 + count}) {name}: rel_err {e:.3g}")
            assert e < gate(precision), (pair, b, name, e)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_counts_are_the_plain_call_bit_for_bit(precision):
    net = AH.make(precision)
    keep = PT._mask([kept(0, 112), kept(1, 112)])
    blank = PT._mask([kept(0, 112)[::3], kept(1, 112)[1::2]])
    for bl in (None, blank):
        for a, b in zip(net.forward_tokens(AH.mel(), keep, bl, ragged=True), net.forward_tokens(AH.mel(), keep, bl)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_clip_of_the_ragged_batch_against_the_clip_alone(precision):
    """The GEMM forms may differ with the row count: the gates of the oracle test, no equality."""
    net = AH.make(precision)
    x = AH.mel()
    for pair in ((126, 30), (1, 225)):
        keep = masks(pair)
        blank = PT._mask([kept(0, pair[0])[::3], kept(1, pair[1])[1::2]])
        for bl in (None, blank):
            both = net.forward_tokens(x, keep, bl, ragged=True)
            for b in range(2):
                alone = net.forward_tokens(x[b:b + 1], keep[b:b + 1], None if bl is None else bl[b:b + 1])
                for o2, o1 in zip(both, alone):
                    e = rel_err(o2[b].cpu(), o1[0].cpu())
                    print(f"  {precision} counts {pair} blank={bl is not None} clip {b}: rel_err {e:.3g}")
                    assert e < gate(precision)


@pytest.mark.parametrize("frames", [(256, 100), (26, 16)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_lengths_against_the_clip_alone(precision, frames):
    """Tp = 25, 9 and 2, 1 time patches; frames past a clip's own hold NaN in the second call: never read."""
    net = AH.make(precision)
    x = AH.mel()
    out = net.forward_lengths(x.clone(), list(frames))
    poisoned = x.clone()
    for b, f in enumerate(frames):
        poisoned[b, ..., f:] = float("nan")
    again = net.forward_lengths(poisoned, torch.tensor(frames))
    assert len(out) == 2 and out[0].shape == (2, 400)
    for a, b in zip(out, again):
        assert torch.equal(a, b)
    for b, f in enumerate(frames):
        with torch.no_grad():
            alone = net(x[b:b + 1, ..., :f].clone(), melspectrogram_input=True)
        for name, o2, o1 in (("logits", out[0], alone[0]), ("features", out[-1], alone[-1])):
            e = rel_err(o2[b].cpu(), o1[0].cpu())
            print(f"  {precision} frames {f} ({(f - 16) // 10 + 1} time patches) clip {b} {name}: rel_err {e:.3g}")
            assert e < gate(precision), (frames, b, name, e)


def test_forward_lengths_with_separated_heads():
    net = AH.make("auto", distilled_type="separated")
    x = AH.mel()
    out = net.forward_lengths(x.clone(), [256, 100])
    assert len(out) == 3 and out[1].shape == (2, 400)
    for b, f in enumerate((256, 100)):
        with torch.no_grad():
            alone = net(x[b:b + 1, ..., :f].clone(), melspectrogram_input=True)
        for o2, o1 in zip(out, alone):
            e = rel_err(o2[b].cpu(), o1[0].cpu())
            print(f"  separated heads, frames {f} clip {b}: rel_err {e:.3g}")
            assert e < gate("auto")
    with pytest.raises(ValueError, match="model.eval"):
        net.train().forward_lengths(x.clone(), [256, 100])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_streams_equal_one_stream_on_a_ragged_batch(precision):
    net = AH.make(precision)
    assert net.eval_streams == 2
    net.EVAL_SPLIT_ROWS = 2          # (the instance attribute shadows the class constant: two clips take the split)
    x = AH.mel()
    keep = masks((126, 30))
    split = []
    side = net._engine._eval_stream(x.device)
    inner = net._engine.forward
    net._engine.forward = lambda *a, **kw: (split.append((torch.cuda.current_stream() == side, kw["n_tok"].tolist())), inner(*a, **kw))[1]
    two = tuple(o.clone() for o in net.forward_tokens(x, keep, ragged=True))
    assert split == [(False, [128]), (True, [32])], split      # two halves, the second on the side stream, each with its own clip's count
    net.eval_streams = 1
    one = tuple(o.clone() for o in net.forward_tokens(x, keep, ragged=True))
    assert len(split) == 3 and split[2][1] == [128, 32]
    for a, b in zip(two, one):
        assert torch.equal(a, b)


def mass_counts(s, fractions):
    """numpy: per fraction and clip the smallest r whose r highest scores (stable order) sum to >= phi x the total, capped at P - 1."""
    out = []
    for f in fractions:
        row = []
        for b in range(s.shape[0]):
            rank = np.argsort(-s[b], kind="stable")
            cum = np.concatenate([[0.0], np.cumsum(s[b][rank].astype(np.float64))])
            row.append(min(int(np.argmax(cum >= f * cum[-1])), s.shape[1] - 1))
        out.append(row)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_curve_by_mass_on_rollout_scores(precision):
    net = AH.make(precision)
    x = AH.mel()
    # (the rollout of the head rows through three random blocks is close to uniform, where a fraction of the mass is the same fraction of
    # the tokens in both clips: the dense start rows of the per-head tests carry another weight per clip and token)
    ROW = 3
    roll = net.attention_rollout(x, start=AH.dense_start().to(x.device))
    s = roll.rollout[:, ROW, 2:].cpu().numpy()
    want = mass_counts(s, FRACTIONS)
    c = net.perturbation_curve(x, roll, CLASS, fractions=FRACTIONS, row=ROW, by="mass")
    assert isinstance(c, PerturbationCurve) and c.removed.dtype == torch.int64 and c.removed.shape == (4, 2)
    assert c.removed.tolist() == want and want[0] == [0, 0] and any(r[0] != r[1] for r in want), (c.removed.tolist(), want)
    with torch.no_grad():
        assert torch.equal(c.logits[0], net(x)[0])
    ref_net = None if precision in ("fp32", "auto") else AH.make("fp32")
    for k, row in enumerate(want):
        ks = []
        for b, r in enumerate(row):
            rank = np.argsort(-s[b], kind="stable")
            ks.append(sorted(set(range(P)) - set(rank[:r].tolist())))
        assert torch.equal(c.keep_mask(k).cpu(), PT._mask(ks))
        ref = (torch.stack([PT.oracle_clip(b, ks[b])[0] for b in range(2)]) if ref_net is None
               else ref_net.forward_tokens(x, PT._mask(ks), ragged=True)[0].cpu())
        for b in range(2):
            e = rel_err(c.logits[k, b].cpu(), ref[b])
            print(f"  {precision} by mass step {k} clip {b} ({row[b]} removed): rel_err {e:.3g}")
            assert e < gate(precision), (k, b, e)
    cb = net.perturbation_curve(x, roll, CLASS, fractions=FRACTIONS, row=ROW, by="mass", mode="blank")
    assert cb.removed.tolist() == want and torch.equal(cb.logits[0], c.logits[0])
