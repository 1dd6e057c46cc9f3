"""CPU (no kernel launches): the surface of the per-head walks -- MAEST.attention_heads' signature, the argument checks and messages it shares
with attention_rollout and attention_relevance, its own alpha-with-target refusal, the AttentionHeads result object, ops.heads_mean, and
the C ABI the feature must leave as it was (no new entry point, ABI 9, one more flag declared in the header; the pinned signatures of
the existing methods and wrappers unchanged).  No model-level emulator test, as for the siblings: a forward of even a small model is too
slow there."""
import inspect
import os
import re

import pytest
import torch

from maest_amd import _lib, ops
from maest_amd.maest import MAEST
from tests import guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty


@pytest.fixture(scope="module")
def model():
    return MAEST(depth=3).eval()


def _params(fn):
    sig = inspect.signature(fn)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    kwo = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY]
    return pos, kwo


def test_signature_and_defaults():
    pos, kwo = _params(MAEST.attention_heads)
    assert pos == [("self", E), ("x", E), ("target", None), ("start", "head"), ("blocks", None), ("alpha", 0.5), ("melspectrogram_input", False)]
    assert kwo == [("target_dist", None), ("grad_scale", 1.0), ("_patchout", None)]
    for fn, names in ((ops.attn_apply_heads, ["qkv", "w", "B", "N", "scale", "q_rows", "x3", "q_prescaled"]),
                      (ops.attn_relevance_heads, ["qkv", "dout", "w", "B", "N", "scale", "q_rows", "x3", "q_prescaled"])):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == names
        assert [sig.parameters[n].default for n in ("q_rows", "x3", "q_prescaled")] == [None, False, False]
    assert list(inspect.signature(ops.heads_mean).parameters) == ["y"]


def test_the_pinned_signatures_are_unchanged():
    pos, kwo = _params(MAEST.attention_rollout)
    assert pos == [("self", E), ("x", E), ("start", "head"), ("blocks", None), ("alpha", 0.5), ("melspectrogram_input", False)]
    assert kwo == [("_patchout", None)]
    pos, kwo = _params(MAEST.attention_relevance)
    assert pos == [("self", E), ("x", E), ("target", E), ("start", "head"), ("blocks", None), ("melspectrogram_input", False)]
    assert kwo == [("target_dist", None), ("grad_scale", 1.0), ("_patchout", None)]
    sig = inspect.signature(ops.attn_apply)
    assert list(sig.parameters) == ["qkv", "w", "B", "N", "scale", "q_rows", "x3", "q_prescaled"]
    assert [sig.parameters[n].default for n in ("q_rows", "x3", "q_prescaled")] == [None, False, False]
    sig = inspect.signature(ops.attn_relevance)
    assert list(sig.parameters) == ["qkv", "dout", "w", "B", "N", "scale", "q_rows", "x3", "q_prescaled"]
    assert [sig.parameters[n].default for n in ("q_rows", "x3", "q_prescaled")] == [None, False, False]


def test_abi_is_unchanged_and_the_header_declares_the_flag():
    assert _lib.ABI_VERSION == 9 and len(_lib.SIGNATURES) == 52 and len(_lib.WRITTEN) == 47
    assert len(guard.device_entries()) == 47
    P, I, F = _lib._P, _lib._I, _lib._F
    assert _lib.SIGNATURES["maest_attn_bwd_rows"] == [P, P, P, P, P, P, I, I, I, F, I, P] and _lib.WRITTEN["maest_attn_bwd_rows"] == (4, 5)
    assert _lib.SIGNATURES["maest_attn_bwd"] == [P, P, P, P, P, P, I, I, I, F, P] and _lib.WRITTEN["maest_attn_bwd"] == (4, 5)
    assert not any("heads" in name or "apply" in name for name in _lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
    assert int(re.search(r"^#define MAEST_ATTN_APPLY_HEADS (\w+)", hdr, flags=re.M).group(1), 0) == _lib.ATTN_APPLY_HEADS == 0x1000
    # a bit of its own: above every dtype code, beside the four other flags, below the rows field
    codes = [int(v) for v in re.findall(r"^#define MAEST_(?:F32|BF16|F32X3|F16|BF16_QS|SPLIT3_A|SPLIT3_B|F32X3_A3) (\d+)", hdr, flags=re.M)]
    assert len(codes) == 8 and all(c & _lib.ATTN_APPLY_HEADS == 0 for c in codes)
    flags = [int(v, 0) for v in re.findall(r"^#define MAEST_ATTN_(?:PROBS|PROBS_MEAN|APPLY|APPLY_GRAD) (\w+)", hdr, flags=re.M)]
    assert sorted(flags) == [0x100, 0x200, 0x400, 0x800] == sorted([_lib.ATTN_PROBS, _lib.ATTN_PROBS_MEAN, _lib.ATTN_APPLY, _lib.ATTN_APPLY_GRAD])
    assert all(f & _lib.ATTN_APPLY_HEADS == 0 for f in flags)
    assert all(_lib.attn_apply_rows(r) & _lib.ATTN_APPLY_HEADS == 0 for r in range(1, 9)) and _lib.attn_apply_rows(2) > _lib.ATTN_APPLY_HEADS
    assert re.search(r"^#define MAEST_ATTN_APPLY_ROWS\(r\) \(\(\(r\) - 1\) << 16\)", hdr, flags=re.M)


# start, blocks and alpha: the checks and the texts of attention_rollout
SWEEP = [
    (dict(start="cls"), ValueError, "start must be"),
    (dict(start=torch.ones(9, 10)), ValueError, "R = 9 rows"),
    (dict(start=torch.ones(10)), ValueError, "start must be"),
    (dict(start=torch.ones(2, 10, dtype=torch.float64)), ValueError, "float32"),
    (dict(start=-torch.ones(2, 10)), ValueError, "non-negative"),
    (dict(start=torch.full((2, 10), float("nan"))), ValueError, "non-negative"),
    (dict(blocks=(0, 1, 2)), ValueError, "contiguous"),
    (dict(blocks=(2, 0)), ValueError, "first must not lie above last"),
    (dict(blocks=(0, 3)), ValueError, "block index 3 out of range"),
    (dict(blocks=(-4, 2)), ValueError, "block index -4 out of range"),
    (dict(blocks=1), TypeError, "pair of ints"),
    (dict(blocks=(0.0, 1)), TypeError, "pair of ints"),
]
ALPHA = [
    (dict(alpha=1.5), ValueError, r"alpha must be a number in \[0, 1\]"),
    (dict(alpha=-0.1), ValueError, r"alpha must be a number in \[0, 1\]"),
    (dict(alpha=True), ValueError, r"alpha must be a number in \[0, 1\]"),
    (dict(alpha="0.5"), ValueError, r"alpha must be a number in \[0, 1\]"),
    (dict(alpha=float("nan")), ValueError, r"alpha must be a number in \[0, 1\]"),
]
# target, target_dist and grad_scale: the checks and the texts of attention_relevance
TARGET = [
    (dict(target=400), ValueError, "target = 400 out of range for 400 classes"),
    (dict(target=-1), ValueError, "out of range"),
    (dict(target=True), TypeError, "target must be"),
    (dict(target="rock"), TypeError, "target must be"),
    (dict(target=3.0), TypeError, "target must be"),
    (dict(target=torch.tensor([[1, 2]])), ValueError, r"one class index per clip, \[B\]"),
    (dict(target=torch.tensor([400])), ValueError, "class index out of range"),
    (dict(target=torch.tensor([0, 1])), ValueError, "B = 1 clips"),
    (dict(target=torch.ones(399)), ValueError, "weights on the 400 logits"),
    (dict(target=torch.ones(2, 400)), ValueError, "B = 1 clips"),
    (dict(target=torch.full((400,), float("nan"))), ValueError, "must be finite"),
    (dict(target=torch.ones(400, dtype=torch.bool)), TypeError, "target must be"),
    (dict(target=0, target_dist=0), ValueError, "target_dist needs distilled_type='separated'"),
    (dict(target=0, grad_scale=0), ValueError, "positive power of two"),
    (dict(target=0, grad_scale=3.0), ValueError, "positive power of two"),
    (dict(target=0, grad_scale=True), ValueError, "positive power of two"),
]


@pytest.mark.parametrize("kw,exc,match", SWEEP + ALPHA + TARGET + [(dict(kw, target=0), exc, match) for kw, exc, match in SWEEP])
def test_bad_arguments_are_refused_before_any_device_work(model, kw, exc, match):
    """On a CPU model every launch raises MaestHipError: an argument error that surfaces first was raised before any device work."""
    with pytest.raises(exc, match=match):
        model.attention_heads(torch.rand(1, 96, 625), **kw)


@pytest.mark.parametrize("kw,exc,match", SWEEP + ALPHA)
def test_the_rollout_messages_are_attention_rollouts(model, kw, exc, match):
    with pytest.raises(exc, match=match):
        model.attention_rollout(torch.rand(1, 96, 625), **kw)


@pytest.mark.parametrize("kw,exc,match", TARGET)
def test_the_target_messages_are_attention_relevances(model, kw, exc, match):
    with pytest.raises(exc, match=match):
        model.attention_relevance(torch.rand(1, 96, 625), **kw)


@pytest.mark.parametrize("alpha", [0.25, 0.0, 1.0, 1, 7.0, "0.5", True])
def test_alpha_with_a_target_is_refused(model, alpha):
    """The gradient-weighted walk has no alpha: anything but the default beside a target is an error, before any device work."""
    with pytest.raises(ValueError, match=r"alpha belongs to the rollout walk \(target=None\)"):
        model.attention_heads(torch.rand(1, 96, 625), 0, alpha=alpha)
    with pytest.raises(ValueError, match="alpha belongs to the rollout walk"):
        model.attention_heads(torch.rand(1, 96, 625), target=torch.ones(400), alpha=alpha)


def test_label_arguments_without_a_target_are_refused(model):
    with pytest.raises(ValueError, match="target_dist needs a target"):
        model.attention_heads(torch.rand(1, 96, 625), target_dist=0)
    with pytest.raises(ValueError, match="grad_scale belongs to the walk with a target"):
        model.attention_heads(torch.rand(1, 96, 625), grad_scale=8.0)


def test_target_dist_is_checked_like_target():
    sep = MAEST(depth=2, distilled_type="separated").eval()
    for kw, exc, match in ((dict(target_dist=400), ValueError, "target_dist = 400 out of range"),
                           (dict(target_dist=torch.ones(3)), ValueError, "target_dist: a float tensor"),
                           (dict(target_dist=torch.tensor([0, 1])), ValueError, "target_dist has shape")):
        with pytest.raises(exc, match=match):
            sep.attention_heads(torch.rand(1, 96, 625), 0, **kw)
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        sep.attention_heads(torch.rand(1, 96, 625), 0, target_dist=torch.ones(400))


def test_input_exceptions_are_those_of_forward_and_there_is_no_cpu_fallback(model):
    with pytest.raises(Exception):
        model.attention_heads(torch.empty([]))
    with pytest.raises(AssertionError):
        model.attention_heads(torch.rand(16000), melspectrogram_input=True)
    with pytest.raises(Exception, match="reduce the input duration"):
        model.attention_heads(torch.rand(2, 40 * 16000).float(), 0)
    for kw in (dict(), dict(alpha=0.0), dict(blocks=(0, -1)), dict(target=0), dict(target=torch.tensor([5])), dict(target=torch.ones(400)),
               dict(target=0, alpha=0.5), dict(target=0, grad_scale=1024)):
        with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
            model.attention_heads(torch.rand(1, 96, 625), **kw)
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        ops.attn_apply_heads(torch.zeros(8, 2304), torch.ones(1, 2, 8), 1, 8, 0.125)
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        ops.attn_relevance_heads(torch.zeros(8, 2304), torch.zeros(8, 768), torch.ones(1, 2, 8), 1, 8, 0.125)
    assert all(p.grad is None for p in model.parameters())


def test_heads_mean_is_the_ascending_fp32_sum_times_a_twelfth():
    """Against an independent evaluation in numpy: eleven fp32 adds, heads ascending, one product with fp32(1) / fp32(12)."""
    import numpy as np
    g = torch.Generator().manual_seed(5)
    y = torch.rand((2, 12, 3, 37), generator=g) * torch.logspace(-6, 3, 12).reshape(1, 12, 1, 1)
    a = y.numpy()
    tot = a[:, 0] + a[:, 1]
    for h in range(2, 12):
        tot = (tot + a[:, h]).astype(np.float32)
    want = tot * (np.float32(1.0) / np.float32(12.0))
    got = ops.heads_mean(y)
    assert got.dtype == torch.float32 and got.shape == (2, 3, 37)
    assert np.array_equal(got.numpy().view(np.int32), want.astype(np.float32).view(np.int32))
    assert np.float32(ops._TWELFTH) == np.float32(1.0) / np.float32(12.0)
    desc = a[:, 11]
    for h in range(10, -1, -1):
        desc = (desc + a[:, h]).astype(np.float32)
    assert not np.array_equal(desc.view(np.int32), tot.view(np.int32))      # (the order matters at this data: the check above can fail)
    with pytest.raises(AssertionError):
        ops.heads_mean(y[:, :11])
    with pytest.raises(AssertionError):
        ops.heads_mean(y.double())


def test_result_object_scores_and_grid():
    """A hand-made result on a 2 x 3 grid of which patches (0, 1) and (1, 2) were dropped: N = 2 + 4; two swept blocks."""
    tokens = torch.tensor([[0, 0], [0, 2], [1, 0], [1, 1]], dtype=torch.int32)
    B, R, N = 2, 2, 6
    per_head = {1: torch.arange(B * 12 * R * N, dtype=torch.float32).reshape(B, 12, R, N),
                2: torch.arange(B * 12 * R * N, dtype=torch.float32).reshape(B, 12, R, N).flip(1) * 0.5}
    res = torch.ones(B, R, N)
    from maest_amd.maest import AttentionHeads
    r = AttentionHeads(per_head, res, "rollout", torch.zeros(B, 400), torch.zeros(B, 768), tokens, [2, 3])
    assert r.grid == (2, 3) and r.logits_dist is None and r.result is res and r.kind == "rollout" and r.per_head is per_head
    for row in (0, 1):
        s = r.head_scores(row) if row else r.head_scores()
        assert s.shape == (B, 2, 12)
        for j, blk in enumerate((1, 2)):
            assert torch.equal(s[:, j], per_head[blk][:, :, row, :].sum(-1))
    want_nan = torch.zeros(2, 3, dtype=torch.bool)
    want_nan[0, 1] = want_nan[1, 2] = True
    for blk, head, row in ((1, 0, 0), (2, 11, 1), (1, 5, 1)):
        g = r.to_grid(blk, head, row) if row else r.to_grid(blk, head)
        assert g.shape == (B, 2, 3) and torch.equal(torch.isnan(g), want_nan.expand(B, 2, 3))
        for j, (f, t) in enumerate(tokens.tolist()):
            assert torch.equal(g[:, f, t], per_head[blk][:, head, row, 2 + j])
    with pytest.raises(KeyError):
        r.to_grid(0, 0)
