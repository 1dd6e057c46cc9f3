"""CPU (no kernel launches): the surface of gradient-weighted rollout -- MAEST.attention_relevance's signature, argument validation and
exceptions, the AttentionRelevance result object, and the C ABI the feature must leave as it was (no new entry point, ABI 9, one more flag
declared in the header).  No model-level emulator test, as for the maps: a forward of even a small model is too slow there."""
import inspect
import os
import re

import pytest
import torch

from maest_amd import _lib, ops
from maest_amd.maest import MAEST, AttentionRelevance
from tests import guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty


@pytest.fixture(scope="module")
def model():
    return MAEST(depth=3).eval()


def test_signature_and_defaults():
    sig = inspect.signature(MAEST.attention_relevance)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert pos == [("self", E), ("x", E), ("target", E), ("start", "head"), ("blocks", None), ("melspectrogram_input", False)]
    kwo = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY]
    assert kwo == [("target_dist", None), ("grad_scale", 1.0), ("_patchout", None)]
    sig = inspect.signature(ops.attn_relevance)
    assert list(sig.parameters) == ["qkv", "dout", "w", "B", "N", "scale", "q_rows", "x3", "q_prescaled"]
    assert [sig.parameters[n].default for n in ("q_rows", "x3", "q_prescaled")] == [None, False, False]


def test_attn_apply_keeps_its_signature():
    sig = inspect.signature(ops.attn_apply)
    assert list(sig.parameters) == ["qkv", "w", "B", "N", "scale", "q_rows", "x3", "q_prescaled"]
    assert [sig.parameters[n].default for n in ("q_rows", "x3", "q_prescaled")] == [None, False, False]


def test_abi_is_unchanged_and_the_header_declares_the_flag():
    assert _lib.ABI_VERSION == 9 and len(_lib.SIGNATURES) == 52 and len(_lib.WRITTEN) == 47
    assert len(guard.device_entries()) == 47
    P, I, F = _lib._P, _lib._I, _lib._F
    assert _lib.SIGNATURES["maest_attn_bwd_rows"] == [P, P, P, P, P, P, I, I, I, F, I, P] and _lib.WRITTEN["maest_attn_bwd_rows"] == (4, 5)
    assert _lib.SIGNATURES["maest_attn_bwd"] == [P, P, P, P, P, P, I, I, I, F, P] and _lib.WRITTEN["maest_attn_bwd"] == (4, 5)
    assert not any("relevance" in name or "apply" in name for name in _lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
    assert int(re.search(r"^#define MAEST_ATTN_APPLY_GRAD (\w+)", hdr, flags=re.M).group(1), 0) == _lib.ATTN_APPLY_GRAD == 0x800
    # a bit of its own: above every dtype code, beside the three other flags, below the rows field
    codes = [int(v) for v in re.findall(r"^#define MAEST_(?:F32|BF16|F32X3|F16|BF16_QS|SPLIT3_A|SPLIT3_B|F32X3_A3) (\d+)", hdr, flags=re.M)]
    assert len(codes) == 8 and all(c & _lib.ATTN_APPLY_GRAD == 0 for c in codes)
    flags = [int(v, 0) for v in re.findall(r"^#define MAEST_ATTN_(?:PROBS|PROBS_MEAN|APPLY) (\w+)", hdr, flags=re.M)]
    assert sorted(flags) == [0x100, 0x200, 0x400] == sorted([_lib.ATTN_PROBS, _lib.ATTN_PROBS_MEAN, _lib.ATTN_APPLY])
    assert all(f & _lib.ATTN_APPLY_GRAD == 0 for f in flags)
    assert all(_lib.attn_apply_rows(r) & _lib.ATTN_APPLY_GRAD == 0 for r in range(1, 9)) and _lib.attn_apply_rows(2) > _lib.ATTN_APPLY_GRAD


@pytest.mark.parametrize("kw,exc,match", [
    (dict(target=400), ValueError, "target = 400 out of range for 400 classes"),
    (dict(target=-1), ValueError, "out of range"),
    (dict(target=True), TypeError, "target must be"),
    (dict(target="rock"), TypeError, "target must be"),
    (dict(target=3.0), TypeError, "target must be"),
    (dict(target=torch.tensor([[1, 2]])), ValueError, r"one class index per clip, \[B\]"),
    (dict(target=torch.tensor([400])), ValueError, "class index out of range"),
    (dict(target=torch.tensor([-1])), ValueError, "class index out of range"),
    (dict(target=torch.tensor([0, 1])), ValueError, "B = 1 clips"),
    (dict(target=torch.ones(399)), ValueError, "weights on the 400 logits"),
    (dict(target=torch.ones(1, 1, 400)), ValueError, "weights on the 400 logits"),
    (dict(target=torch.ones(2, 400)), ValueError, "B = 1 clips"),
    (dict(target=torch.full((400,), float("nan"))), ValueError, "must be finite"),
    (dict(target=torch.full((1, 400), float("inf"))), ValueError, "must be finite"),
    (dict(target=torch.ones(400, dtype=torch.bool)), TypeError, "target must be"),
    (dict(target=0, target_dist=0), ValueError, "target_dist needs distilled_type='separated'"),
    (dict(target=0, grad_scale=0), ValueError, "positive power of two"),
    (dict(target=0, grad_scale=3.0), ValueError, "positive power of two"),
    (dict(target=0, grad_scale=-2.0), ValueError, "positive power of two"),
    (dict(target=0, grad_scale=float("inf")), ValueError, "positive power of two"),
    (dict(target=0, grad_scale=float("nan")), ValueError, "positive power of two"),
    (dict(target=0, grad_scale="8"), ValueError, "positive power of two"),
    (dict(target=0, grad_scale=True), ValueError, "positive power of two"),
    # start and blocks: the checks and the texts of attention_rollout
    (dict(target=0, start="cls"), ValueError, "start must be"),
    (dict(target=0, start=torch.ones(9, 10)), ValueError, "R = 9 rows"),
    (dict(target=0, start=torch.ones(10)), ValueError, "start must be"),
    (dict(target=0, start=torch.ones(2, 10, dtype=torch.float64)), ValueError, "float32"),
    (dict(target=0, start=-torch.ones(2, 10)), ValueError, "non-negative"),
    (dict(target=0, start=torch.full((2, 10), float("nan"))), ValueError, "non-negative"),
    (dict(target=0, blocks=(0, 1, 2)), ValueError, "contiguous"),
    (dict(target=0, blocks=(2, 0)), ValueError, "first must not lie above last"),
    (dict(target=0, blocks=(0, 3)), ValueError, "block index 3 out of range"),
    (dict(target=0, blocks=(-4, 2)), ValueError, "block index -4 out of range"),
    (dict(target=0, blocks=1), TypeError, "pair of ints"),
    (dict(target=0, blocks=(0.0, 1)), TypeError, "pair of ints"),
])
def test_bad_arguments_are_refused_before_any_device_work(model, kw, exc, match):
    """On a CPU model every launch raises MaestHipError: an argument error that surfaces first was raised before any device work."""
    with pytest.raises(exc, match=match):
        model.attention_relevance(torch.rand(1, 96, 625), **kw)


def test_target_dist_is_checked_like_target():
    sep = MAEST(depth=2, distilled_type="separated").eval()
    for kw, exc, match in ((dict(target_dist=400), ValueError, "target_dist = 400 out of range"),
                           (dict(target_dist=torch.ones(3)), ValueError, "target_dist: a float tensor"),
                           (dict(target_dist=torch.tensor([0, 1])), ValueError, "target_dist has shape")):
        with pytest.raises(exc, match=match):
            sep.attention_relevance(torch.rand(1, 96, 625), 0, **kw)
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        sep.attention_relevance(torch.rand(1, 96, 625), 0, target_dist=torch.ones(400))


def test_input_exceptions_are_those_of_forward_and_there_is_no_cpu_fallback(model):
    with pytest.raises(Exception):
        model.attention_relevance(torch.empty([]), 0)
    with pytest.raises(AssertionError):
        model.attention_relevance(torch.rand(16000), 0, melspectrogram_input=True)
    with pytest.raises(Exception, match="reduce the input duration"):
        model.attention_relevance(torch.rand(2, 40 * 16000).float(), 0)
    for kw in (dict(target=0), dict(target=torch.tensor([5])), dict(target=torch.ones(400)), dict(target=torch.zeros(1, 400), blocks=(0, -1)),
               dict(target=0, grad_scale=1024), dict(target=0, grad_scale=0.25)):
        with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
            model.attention_relevance(torch.rand(1, 96, 625), **kw)
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        ops.attn_relevance(torch.zeros(8, 2304), torch.zeros(8, 768), torch.ones(1, 2, 8), 1, 8, 0.125)
    assert all(p.grad is None for p in model.parameters())


def test_to_grid_scatters_the_patch_columns_and_marks_dropped_patches():
    """A hand-made result on a 2 x 3 grid of which patches (0, 1) and (1, 2) were dropped: N = 2 + 4."""
    tokens = torch.tensor([[0, 0], [0, 2], [1, 0], [1, 1]], dtype=torch.int32)
    B, R, N = 2, 2, 6
    rel = torch.arange(B * R * N, dtype=torch.float32).reshape(B, R, N)
    r = AttentionRelevance(rel, torch.zeros(B, 400), torch.zeros(B, 768), tokens, [2, 3])
    assert r.grid == (2, 3) and r.logits_dist is None and r.relevance is rel
    want_nan = torch.zeros(2, 3, dtype=torch.bool)
    want_nan[0, 1] = want_nan[1, 2] = True
    for row in (0, 1):
        g = r.to_grid(row) if row else r.to_grid()
        assert g.shape == (B, 2, 3) and torch.equal(torch.isnan(g), want_nan.expand(B, 2, 3))
        for j, (f, t) in enumerate(tokens.tolist()):
            assert torch.equal(g[:, f, t], rel[:, row, 2 + j])
