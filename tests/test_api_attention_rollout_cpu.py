"""CPU (no kernel launches): the surface of attention rollout -- MAEST.attention_rollout's signature, argument validation and exceptions, the
AttentionRollout result object, and the C ABI the feature must leave as it was (no new entry point, ABI 9, one flag and a rows field declared
in the header).  No model-level emulator test, as for the maps: a forward of even a small model is too slow there."""
import inspect
import os
import re

import pytest
import torch

from maest_amd import _lib, ops
from maest_amd.maest import MAEST, AttentionRollout
from tests import guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return MAEST(depth=3).eval()


def test_signature_and_defaults():
    sig = inspect.signature(MAEST.attention_rollout)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert pos == [("self", inspect.Parameter.empty), ("x", inspect.Parameter.empty), ("start", "head"), ("blocks", None), ("alpha", 0.5),
                   ("melspectrogram_input", False)]
    sig = inspect.signature(ops.attn_apply)
    assert list(sig.parameters) == ["qkv", "w", "B", "N", "scale", "q_rows", "x3", "q_prescaled"]
    assert [sig.parameters[n].default for n in ("q_rows", "x3", "q_prescaled")] == [None, False, False]


def test_abi_is_unchanged_and_the_header_declares_the_flag():
    assert _lib.ABI_VERSION == 9 and len(_lib.SIGNATURES) == 52 and len(_lib.WRITTEN) == 47
    assert len(guard.device_entries()) == 47
    P, I, F = _lib._P, _lib._I, _lib._F
    assert _lib.SIGNATURES["maest_attn_bwd_rows"] == [P, P, P, P, P, P, I, I, I, F, I, P] and _lib.WRITTEN["maest_attn_bwd_rows"] == (4, 5)
    assert _lib.SIGNATURES["maest_attn_bwd"] == [P, P, P, P, P, P, I, I, I, F, P] and _lib.WRITTEN["maest_attn_bwd"] == (4, 5)
    assert not any("apply" in name or "rollout" in name for name in _lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
    assert int(re.search(r"^#define MAEST_ATTN_APPLY (\w+)", hdr, flags=re.M).group(1), 0) == _lib.ATTN_APPLY == 0x400
    assert re.search(r"^#define MAEST_ATTN_APPLY_ROWS\(r\) \(\(\(r\) - 1\) << 16\)", hdr, flags=re.M)
    assert [_lib.attn_apply_rows(r) for r in (1, 2, 8)] == [0, 1 << 16, 7 << 16]
    # the flag is a bit of its own above every dtype code and beside the maps' flags; the rows field lies above all of them
    codes = [int(v) for v in re.findall(r"^#define MAEST_(?:F32|BF16|F32X3|F16|BF16_QS|SPLIT3_A|SPLIT3_B|F32X3_A3) (\d+)", hdr, flags=re.M)]
    assert len(codes) == 8 and all(c & _lib.ATTN_APPLY == 0 for c in codes)
    assert _lib.ATTN_APPLY & (_lib.ATTN_PROBS | _lib.ATTN_PROBS_MEAN) == 0 and _lib.attn_apply_rows(2) > _lib.ATTN_APPLY


@pytest.mark.parametrize("kw,exc,match", [
    (dict(alpha=-0.1), ValueError, "alpha must be"),
    (dict(alpha=1.5), ValueError, "alpha must be"),
    (dict(alpha=float("nan")), ValueError, "alpha must be"),
    (dict(alpha="0.5"), ValueError, "alpha must be"),
    (dict(start="cls"), ValueError, "start must be"),
    (dict(start=torch.ones(9, 10)), ValueError, "R = 9 rows"),
    (dict(start=torch.ones(2, 9, 10)), ValueError, "R = 9 rows"),
    (dict(start=torch.ones(10)), ValueError, "start must be"),
    (dict(start=torch.ones(1, 2, 2, 10)), ValueError, "start must be"),
    (dict(start=torch.ones(2, 10, dtype=torch.float64)), ValueError, "float32"),
    (dict(start=-torch.ones(2, 10)), ValueError, "non-negative"),
    (dict(start=torch.full((2, 10), float("nan"))), ValueError, "non-negative"),
    (dict(blocks=(0, 1, 2)), ValueError, "contiguous"),
    (dict(blocks=[0, 2, 4]), ValueError, "contiguous"),
    (dict(blocks=(2, 0)), ValueError, "first must not lie above last"),
    (dict(blocks=(0, 3)), ValueError, "block index 3 out of range"),
    (dict(blocks=(-4, 2)), ValueError, "block index -4 out of range"),
    (dict(blocks=1), TypeError, "pair of ints"),
    (dict(blocks=(0.0, 1)), TypeError, "pair of ints"),
])
def test_bad_arguments_are_refused_before_any_device_work(model, kw, exc, match):
    with pytest.raises(exc, match=match):
        model.attention_rollout(torch.rand(1, 96, 625), **kw)


def test_input_exceptions_are_those_of_forward_and_there_is_no_cpu_fallback(model):
    with pytest.raises(Exception):
        model.attention_rollout(torch.empty([]))
    with pytest.raises(AssertionError):
        model.attention_rollout(torch.rand(16000), melspectrogram_input=True)
    with pytest.raises(Exception, match="reduce the input duration"):
        model.attention_rollout(torch.rand(2, 40 * 16000).float())
    for kw in (dict(), dict(blocks=(0, -1)), dict(alpha=1), dict(alpha=0)):
        with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
            model.attention_rollout(torch.rand(1, 96, 625), **kw)
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        ops.attn_apply(torch.zeros(8, 2304), torch.ones(1, 2, 8), 1, 8, 0.125)


def test_to_grid_scatters_the_patch_columns_and_marks_dropped_patches():
    """A hand-made result on a 2 x 3 grid of which patches (0, 1) and (1, 2) were dropped: N = 2 + 4."""
    tokens = torch.tensor([[0, 0], [0, 2], [1, 0], [1, 1]], dtype=torch.int32)
    B, R, N = 2, 2, 6
    roll = torch.arange(B * R * N, dtype=torch.float32).reshape(B, R, N)
    r = AttentionRollout(roll, torch.zeros(B, 400), torch.zeros(B, 768), tokens, [2, 3])
    assert r.grid == (2, 3) and r.logits_dist is None and r.rollout is roll
    want_nan = torch.zeros(2, 3, dtype=torch.bool)
    want_nan[0, 1] = want_nan[1, 2] = True
    for row in (0, 1):
        g = r.to_grid(row) if row else r.to_grid()
        assert g.shape == (B, 2, 3) and torch.equal(torch.isnan(g), want_nan.expand(B, 2, 3))
        for j, (f, t) in enumerate(tokens.tolist()):
            assert torch.equal(g[:, f, t], roll[:, row, 2 + j])
