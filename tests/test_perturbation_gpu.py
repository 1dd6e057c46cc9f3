"""GPU (`-m gpu`): MAEST.forward_tokens and MAEST.perturbation_curve on the three-block model and the two 256-frame clips of
tests/test_attention_heads_gpu.py (a 9 x 25 patch grid, P = 225, N = 227), in every precision of its PRECISIONS.

The reference is the oracle composed on the CPU clip by clip: O.patch_embed, O.tokens_from_patches(.., u_keep = the clip's kept tokens),
O.block x 3, the final norm and the head as in O.forward; for "blank" the convolution's output is set to its bias at the blank positions.
Gates: rel_err < 1e-3 in "fp32" / "auto" (tests/test_model_gpu.py's gate, with its rel_err); the 16-bit modes within that file's 3e-2
band of the "fp32" model's curve.  The kept sets the oracle gets are made here with a numpy stable sort, not read from the result."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maest_amd.maest import AttentionRollout, PerturbationCurve
from oracle import maest_oracle as O
from tests import test_attention_heads_gpu as AH
from tests.test_model_gpu import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 225
CLASS = AH.CLASS
FRACTIONS = (0.0, 0.2, 0.5, 0.8)
REMOVED = (0, 45, 112, 180)
PRECISIONS = AH.PRECISIONS


def gate(precision):
    return 1e-3 if precision in ("fp32", "auto") else 3e-2


@functools.lru_cache(maxsize=None)
def scores():
    """fp32 [2, 225], another ranking per clip, with a tie that straddles a cut; shared, never modified."""
    s = AH.RG.randn((2, P), 611)
    s[0, 10:20] = s[0, 10]
    return s


def kept(order, r):
    """Per clip the ascending list of the tokens step r keeps (numpy, stable)."""
    s = scores().numpy()
    out = []
    for b in range(2):
        rank = np.argsort(-s[b] if order == "positive" else s[b], kind="stable")
        out.append(sorted(set(range(P)) - set(rank[:r].tolist())))
    return out


@functools.lru_cache(maxsize=None)
def conv():
    return O.patch_embed(AH.RG.mel(), AH.state_dict())      # [2, 768, 9, 25]


def oracle_clip(b, keep_idx, blank_idx=()):
    """The oracle's logits and features of clip b on the tokens `keep_idx`, those of `blank_idx` with the convolution's bias as content."""
    sd = AH.state_dict()
    c = conv()[b:b + 1].clone()
    if len(blank_idx):
        c.flatten(2)[:, :, list(blank_idx)] = sd["patch_embed.proj.bias"].reshape(1, -1, 1)
    x = O.tokens_from_patches(c, sd, u_keep=keep_idx)
    for i in range(AH.DEPTH):
        x = O.block(x, sd, i)
    x = F.layer_norm(x, (768,), sd["norm.weight"], sd["norm.bias"], 1e-6)
    feat = (x[:, 0] + x[:, 1]) / 2
    z = F.layer_norm(feat, (768,), sd["head.0.weight"], sd["head.0.bias"], 1e-5)
    return F.linear(z, sd["head.1.weight"], sd["head.1.bias"])[0], feat[0]


@functools.lru_cache(maxsize=None)
def oracle_curve(mode):
    """fp32 [S, 2, C]: every step and clip of the order="positive" curve; computed once, shared, never modified."""
    rows = []
    for r in REMOVED:
        ks = kept("positive", r)
        if mode == "drop":
            rows.append(torch.stack([oracle_clip(b, ks[b])[0] for b in range(2)]))
        else:
            rows.append(torch.stack([oracle_clip(b, list(range(P)), sorted(set(range(P)) - set(ks[b])))[0] for b in range(2)]))
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def fp32_curve(mode):
    """The "fp32" model's curve, the reference of the 16-bit modes."""
    return AH.make("fp32").perturbation_curve(AH.mel(), scores(), CLASS, fractions=FRACTIONS, mode=mode).logits.cpu()


@functools.lru_cache(maxsize=None)
def fp32_features():
    return AH.make("fp32").forward_tokens(AH.mel(), _mask(kept("positive", 112)))[-1].cpu()


def _mask(idx_lists):
    m = torch.zeros((len(idx_lists), P), dtype=torch.bool)
    for b, idx in enumerate(idx_lists):
        m[b, idx] = True
    return m


@pytest.mark.parametrize("precision", PRECISIONS)
def test_curve_shortens_the_sequence_and_step_zero_is_the_plain_forward(precision):
    net = AH.make(precision)
    seen = []
    inner = net._eval_forward
    net._eval_forward = lambda x3, dt, kw: (seen.append(tuple(kw["tok_ft"].shape)), inner(x3, dt, kw))[1]
    c = net.perturbation_curve(AH.mel(), scores(), CLASS, fractions=FRACTIONS)
    assert isinstance(c, PerturbationCurve) and c.order == "positive" and c.mode == "drop" and c.fractions == FRACTIONS
    assert c.removed.tolist() == list(REMOVED) and [2 + s[1] for s in seen] == [227, 182, 115, 47] and all(s[0] == 2 and s[2] == 2 for s in seen)
    assert c.logits.shape == (4, 2, 400) and c.logits.dtype == torch.float32 and not c.logits.requires_grad and c.logits_dist is None
    assert c.logit.shape == c.prob.shape == (4, 2) and c.auc.shape == (2,) and c.tokens.shape == (P, 2)
    assert torch.equal(c.logit, c.logits[:, :, CLASS]) and torch.equal(c.prob, torch.sigmoid(c.logit))
    for k, r in enumerate(REMOVED):
        assert torch.equal(c.keep_mask(k).cpu(), _mask(kept("positive", r)))
    del seen[:]
    cb = net.perturbation_curve(AH.mel(), scores(), CLASS, fractions=FRACTIONS, mode="blank")
    assert [2 + s[1] for s in seen] == [227] * 4 and cb.mode == "blank"
    del net._eval_forward
    with torch.no_grad():
        plain = net(AH.mel())
    # every launch behind x0 is the plain forward's, and x0 is bit-identical (tests/test_im2col_clips_gpu.py)
    assert torch.equal(c.logits[0], plain[0]) and torch.equal(cb.logits[0], plain[0])
    everything = net.forward_tokens(AH.mel(), torch.ones(2, P, dtype=torch.bool))
    assert len(everything) == len(plain) and torch.equal(everything[0], plain[0]) and torch.equal(everything[-1], plain[-1])


@pytest.mark.parametrize("mode", ["drop", "blank"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_step_and_clip_against_the_oracle(precision, mode):
    c = AH.make(precision).perturbation_curve(AH.mel(), scores(), CLASS, fractions=FRACTIONS, mode=mode)
    ref = oracle_curve(mode) if precision in ("fp32", "auto") else fp32_curve(mode)
    got = c.logits.cpu()
    for k in range(len(FRACTIONS)):
        for b in range(2):
            e = rel_err(got[k, b], ref[k, b])
            print(f"  {precision} {mode} step {k} clip {b}: rel_err {e:.3g}")
            assert e < gate(precision), (k, b, e)
    if mode == "drop":      # and the features of one step, through forward_tokens
        feats = AH.make(precision).forward_tokens(AH.mel(), _mask(kept("positive", 112)))[-1].cpu()
        for b in range(2):
            want = oracle_clip(b, kept("positive", 112)[b])[1] if precision in ("fp32", "auto") else fp32_features()[b]
            assert rel_err(feats[b], want) < gate(precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_clip_of_the_batch_against_the_clip_alone(precision):
    """The GEMM forms may differ with the row count: the gates of the oracle test, no equality."""
    net = AH.make(precision)
    x = AH.mel()
    ks = kept("positive", 112)
    keep = _mask(ks)
    blank = _mask([ks[0][::3], ks[1][1::2]])
    for bl in (None, blank):
        both = net.forward_tokens(x, keep, bl)
        for b in range(2):
            alone = net.forward_tokens(x[b:b + 1], keep[b:b + 1], None if bl is None else bl[b:b + 1])
            for o2, o1 in zip(both, alone):
                e = rel_err(o2[b].cpu(), o1[0].cpu())
                print(f"  {precision} blank={bl is not None} clip {b}: rel_err {e:.3g}")
                assert e < gate(precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_masks_are_per_clip(precision):
    """Swapping the two clips' masks changes the logits, into what the oracle says of the swapped masks."""
    net = AH.make(precision)
    x = AH.mel()
    keep = _mask(kept("positive", 180))
    assert not torch.equal(keep[0], keep[1])
    a, b = net.forward_tokens(x, keep)[0], net.forward_tokens(x, keep.flip(0))[0]
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    if precision in ("fp32", "auto"):
        ks = kept("positive", 180)
        for c in range(2):
            assert rel_err(b[c].cpu(), oracle_clip(c, ks[1 - c])[0]) < gate(precision)
    for bad, match in ((keep[:1], "keep has shape"), (torch.cat([keep[:1], _mask([list(range(44))])]), "same number of tokens")):
        with pytest.raises(ValueError, match=match):
            net.forward_tokens(x, bad)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_streams_equal_one_stream_on_per_clip_tokens(precision):
    net = AH.make(precision)
    assert net.eval_streams == 2
    net.EVAL_SPLIT_ROWS = 2          # (the instance attribute shadows the class constant: two clips take the split)
    x = AH.mel()
    ks = kept("positive", 112)
    keep, blank = _mask(ks), _mask([ks[0][::3], ks[1][1::2]])      # the two halves hold different masks
    split = []
    side = net._engine._eval_stream(x.device)
    inner = net._engine.forward
    net._engine.forward = lambda *a, **kw: (split.append(torch.cuda.current_stream() == side), inner(*a, **kw))[1]
    two = [tuple(o.clone() for o in net.forward_tokens(x, keep, bl)) for bl in (None, blank)]
    assert split == [False, True] * 2, split      # each call ran as two halves, the second on the side stream
    net.eval_streams = 1
    one = [tuple(o.clone() for o in net.forward_tokens(x, keep, bl)) for bl in (None, blank)]
    assert len(split) == 6
    for t, o in zip(two, one):
        for a, b in zip(t, o):
            assert torch.equal(a, b)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_curves_from_rollout_scores_run_end_to_end(precision):
    """Whether the map turns out faithful is not asserted: the weights are random."""
    net = AH.make(precision)
    x = AH.mel()
    roll = net.attention_rollout(x)
    target = torch.tensor([CLASS, 3])
    for order in ("positive", "negative"):
        for mode in ("drop", "blank"):
            c = net.perturbation_curve(x, roll, target, order=order, mode=mode, row=1)
            assert c.logits.shape == (10, 2, 400) and c.removed.tolist() == [0, 22, 45, 67, 90, 112, 135, 157, 180, 202]
            assert bool(torch.isfinite(c.prob).all()) and bool(torch.isfinite(c.auc).all())
            assert torch.equal(c.logit[:, 1], c.logits[:, 1, 3]) and torch.equal(c.logits[0], roll.logits)
            p, f = c.prob.double().cpu(), torch.tensor(c.fractions, dtype=torch.float64)
            want = sum((p[k] + p[k + 1]) / 2 * (f[k + 1] - f[k]) for k in range(9)) / (f[-1] - f[0])
            assert torch.allclose(c.auc.double().cpu(), want, rtol=1e-6, atol=0)
            rank = np.argsort(-roll.rollout[0, 1, 2:].cpu().numpy() if order == "positive" else roll.rollout[0, 1, 2:].cpu().numpy(), kind="stable")
            assert sorted(np.flatnonzero(~c.keep_mask(3)[0].cpu().numpy()).tolist()) == sorted(rank[:67].tolist())
    rnd = net.perturbation_curve(x, "random", CLASS, seed=5)
    assert torch.equal(rnd.logits, net.perturbation_curve(x, "random", CLASS, seed=5).logits)
    assert not torch.equal(rnd.logits[5], net.perturbation_curve(x, "random", CLASS, seed=6).logits[5])
    assert net.perturbation_curve(x, roll, CLASS, fractions=(0.5,)).auc is None
    with pytest.raises(ValueError, match="scores have shape"):
        net.perturbation_curve(x, net.attention_rollout(x[:, :, :, :200]), CLASS)
    moved = AttentionRollout(roll.rollout, roll.logits, roll.features, roll.tokens.flip(0), roll.grid)
    with pytest.raises(ValueError, match="another token sequence"):
        net.perturbation_curve(x, moved, CLASS)
