"""CPU (no kernel launches): the surface of the attention maps -- MAEST.attention_maps' argument validation and exceptions, the AttentionMaps
result object, and the C ABI the feature must leave as it was (no new entry point, ABI 9, two flag bits declared in the header)."""
import os
import re

import pytest
import torch

from maest_amd import _lib
from maest_amd.maest import MAEST, AttentionMaps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return MAEST(depth=3).eval()


def test_abi_is_unchanged_and_the_header_declares_the_flags():
    assert _lib.ABI_VERSION == 9 and len(_lib.SIGNATURES) == 52 and len(_lib.WRITTEN) == 47
    P, I, F = _lib._P, _lib._I, _lib._F
    assert _lib.SIGNATURES["maest_attn_fwd_rows"] == [P, P, P, I, I, I, F, I, P] and _lib.WRITTEN["maest_attn_fwd_rows"] == (1, 2)
    assert _lib.SIGNATURES["maest_attn_fwd"] == [P, P, P, I, I, I, F, P]
    assert not any("probs" in name for name in _lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
    flags = {n: int(v, 0) for n, v in re.findall(r"^#define (MAEST_ATTN_PROBS\w*) (\w+)", hdr, flags=re.M)}
    assert flags == {"MAEST_ATTN_PROBS": _lib.ATTN_PROBS, "MAEST_ATTN_PROBS_MEAN": _lib.ATTN_PROBS_MEAN}
    # above every dtype code, and two distinct bits
    codes = [int(v) for v in re.findall(r"^#define MAEST_(?:F32|BF16|F32X3|F16|BF16_QS|SPLIT3_A|SPLIT3_B|F32X3_A3) (\d+)", hdr, flags=re.M)]
    assert len(codes) == 8 and max(codes) < _lib.ATTN_PROBS < _lib.ATTN_PROBS_MEAN and _lib.ATTN_PROBS & _lib.ATTN_PROBS_MEAN == 0
    assert all(c & (_lib.ATTN_PROBS | _lib.ATTN_PROBS_MEAN) == 0 for c in codes)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(queries="cls"), ValueError, "queries must be"),
    (dict(heads="sum"), ValueError, "heads must be"),
    (dict(blocks=3), ValueError, "block index 3 out of range"),
    (dict(blocks=-4), ValueError, "block index -4 out of range"),
    (dict(blocks=[0, 7]), ValueError, "block index 7 out of range"),
    (dict(blocks=[0.5]), TypeError, "iterable of ints"),
    (dict(blocks=True), TypeError, "iterable of ints"),
])
def test_bad_arguments_are_refused_before_any_device_work(model, kw, exc, match):
    with pytest.raises(exc, match=match):
        model.attention_maps(torch.rand(1, 96, 625), **kw)


def test_input_exceptions_are_those_of_forward(model):
    with pytest.raises(Exception):
        model.attention_maps(torch.empty([]))
    with pytest.raises(AssertionError):
        model.attention_maps(torch.rand(16000), melspectrogram_input=True)
    with pytest.raises(Exception, match="reduce the input duration"):
        model.attention_maps(torch.rand(2, 40 * 16000).float())
    for blocks in (None, -1, [0, -1], range(3)):
        with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
            model.attention_maps(torch.rand(1, 96, 625), blocks=blocks)


def _result(heads_all=True, B=2):
    """A hand-made result on a 2 x 3 grid of which patches (0, 1) and (1, 2) were dropped: N = 2 + 4."""
    tokens = torch.tensor([[0, 0], [0, 2], [1, 0], [1, 1]], dtype=torch.int32)
    N = 6
    p = torch.arange(B * 12 * 2 * N, dtype=torch.float32).reshape(B, 12, 2, N)
    maps = {1: p if heads_all else p.mean(1)}
    return AttentionMaps(torch.zeros(B, 400), torch.zeros(B, 768), maps, tokens, (2, 3)), p


def test_to_grid_scatters_the_patch_columns_and_marks_dropped_patches():
    r, p = _result()
    assert r.grid == (2, 3) and r.logits_dist is None and list(r.maps) == [1]
    g = r.to_grid(1)
    assert g.shape == (2, 12, 2, 3)
    nan = torch.isnan(g)
    want_nan = torch.zeros(2, 3, dtype=torch.bool)
    want_nan[0, 1] = want_nan[1, 2] = True
    assert torch.equal(nan, want_nan.expand(2, 12, 2, 3))
    for j, (f, t) in enumerate(r.tokens.tolist()):
        assert torch.equal(g[:, :, f, t], p[:, :, 0, 2 + j])
    g1 = r.to_grid(1, query=1, head=5)
    assert g1.shape == (2, 2, 3) and torch.equal(g1[:, 1, 1], p[:, 5, 1, 5]) and torch.equal(torch.isnan(g1), want_nan.expand(2, 2, 3))
    with pytest.raises(KeyError):
        r.to_grid(0)


def test_to_grid_of_head_mean_maps():
    r, p = _result(heads_all=False)
    g = r.to_grid(1, query=1)
    assert g.shape == (2, 2, 3) and torch.equal(g[:, 0, 2], p.mean(1)[:, 1, 3])
    with pytest.raises(ValueError, match="mean over the heads"):
        r.to_grid(1, head=0)
