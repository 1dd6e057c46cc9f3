"""CPU (no kernel launches): the surface of the hidden states -- MAEST.hidden_states' signature, its argument checks (all of them before any
device work), the HiddenStates result object with its NaN scatter, ops.grid_pools' refusal of CPU tensors, and the C ABI the feature must
leave as it was (no new entry point, ABI 9; one flag and the Tk field declared in the header and in _lib)."""
import inspect
import os
import re

import pytest
import torch

from maest_amd import _lib, ops
from maest_amd.hidden import POOLS, kept_axes
from maest_amd.maest import MAEST, HiddenStates
from tests import guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty


@pytest.fixture(scope="module")
def model():
    return MAEST(depth=3).eval()


def test_signature_and_defaults():
    sig = inspect.signature(MAEST.hidden_states)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    kwo = [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY]
    assert pos == [("self", E), ("x", E), ("blocks", None), ("pool", "embedding"), ("melspectrogram_input", False)]
    assert kwo == [("_patchout", None)]
    assert POOLS == ("embedding", "time", "freq", "states")
    assert list(inspect.signature(ops.grid_pools).parameters) == ["x", "Tk", "n_head"]
    for word in ("head_tail = False", "split_add_eval", "no_grad", "before any device work"):
        assert word in MAEST.hidden_states.__doc__


def test_abi_is_unchanged_and_the_header_declares_the_form():
    assert _lib.ABI_VERSION == 9 and len(_lib.SIGNATURES) == 52 and len(_lib.WRITTEN) == 47
    assert len(guard.device_entries()) == 47
    P, I = _lib._P, _lib._I
    assert _lib.SIGNATURES["maest_gather_head_rows"] == [P, I, I, I, I, P, P] and _lib.WRITTEN["maest_gather_head_rows"] == (5,)
    assert not any("pool" in name and name not in ("maest_head_pool_fwd", "maest_head_pool_bwd", "maest_embed_pool", "maest_embed_pool_bwd")
                   for name in _lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
    assert int(re.search(r"^#define MAEST_GATHER_POOLS (\w+)", hdr, flags=re.M).group(1), 0) == _lib.GATHER_POOLS == 0x100
    assert re.search(r"^#define MAEST_GATHER_POOLS_T\(t\) \(\(t\) << 16\)", hdr, flags=re.M)
    assert [_lib.gather_pools_t(t) for t in (1, 25, 187)] == [1 << 16, 25 << 16, 187 << 16]
    # a bit of its own above every dtype code, the Tk field above the flag
    codes = [int(v) for v in re.findall(r"^#define MAEST_(?:F32|BF16|F32X3|F16|BF16_QS|SPLIT3_A|SPLIT3_B|F32X3_A3) (\d+)", hdr, flags=re.M)]
    assert len(codes) == 8 and max(codes) < _lib.GATHER_POOLS < _lib.gather_pools_t(1)
    assert all(c & _lib.GATHER_POOLS == 0 for c in codes)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(blocks=3), ValueError, "block index 3 out of range"),
    (dict(blocks=-4), ValueError, "block index -4 out of range"),
    (dict(blocks=[0, 7]), ValueError, "block index 7 out of range"),
    (dict(blocks=[0.5]), TypeError, "iterable of ints"),
    (dict(blocks=True), TypeError, "iterable of ints"),
    (dict(blocks="1"), TypeError, "iterable of ints"),
    (dict(blocks=[True]), TypeError, "iterable of ints"),
    (dict(pool="mean"), ValueError, "pool must be one of"),
    (dict(pool=("embedding", "cls")), ValueError, "pool must be one of"),
    (dict(pool=None), ValueError, "pool must be one of"),
    (dict(pool=3), ValueError, "pool must be one of"),
    (dict(pool=[1]), ValueError, "pool must be one of"),
    (dict(pool=()), ValueError, "at least one"),
])
def test_bad_arguments_are_refused_before_any_device_work(model, kw, exc, match):
    """On a CPU model every launch raises MaestHipError: an argument error that surfaces first was raised before any device work."""
    with pytest.raises(exc, match=match):
        model.hidden_states(torch.rand(1, 96, 625), **kw)


def test_unstructured_patchout_is_refused_for_the_axis_pools_before_any_device_work():
    net = MAEST(depth=2, u_patchout=50).train()
    for pool in ("time", "freq", ("embedding", "time"), POOLS):
        with pytest.raises(ValueError, match="full frequency x time grid"):
            net.hidden_states(torch.rand(1, 96, 625), pool=pool)
    for pool in ("embedding", "states", ("states", "embedding")):      # these need no grid: the call goes on to the device, which a CPU has not
        with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
            net.hidden_states(torch.rand(1, 96, 625), pool=pool)
    net.eval()                                                          # an evaluation forward keeps every patch
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        net.hidden_states(torch.rand(1, 96, 625), pool="time")


def test_input_exceptions_are_those_of_forward_and_there_is_no_cpu_fallback(model):
    with pytest.raises(Exception):
        model.hidden_states(torch.empty([]))
    with pytest.raises(AssertionError):
        model.hidden_states(torch.rand(16000), melspectrogram_input=True)
    with pytest.raises(Exception, match="reduce the input duration"):
        model.hidden_states(torch.rand(2, 40 * 16000).float())
    for kw in (dict(), dict(blocks=-1), dict(blocks=[0, -1], pool="time"), dict(blocks=range(3), pool=POOLS), dict(pool=iter(["freq"]))):
        with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
            model.hidden_states(torch.rand(1, 96, 625), **kw)
    with pytest.raises(_lib.MaestHipError, match="no CPU fallback"):
        ops.grid_pools(torch.zeros(1, 8, 768), 3)
    assert all(p.grad is None for p in model.parameters())


def test_kept_axes_recognises_a_full_grid():
    f, t = torch.tensor([0, 2, 5]), torch.tensor([1, 3, 4, 9])
    tok = torch.stack(torch.meshgrid(f, t, indexing="ij"), dim=-1).reshape(-1, 2).to(torch.int32)
    got = kept_axes(tok)
    assert torch.equal(got[0], f) and torch.equal(got[1], t)
    assert kept_axes(tok[:-1]) is None and kept_axes(tok[[0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 7]]) is None
    one = kept_axes(torch.tensor([[4, 7]], dtype=torch.int32))
    assert one[0].tolist() == [4] and one[1].tolist() == [7]


def test_result_object_and_the_nan_scatter():
    """A hand-made result on a 3 x 5 grid of which frequency row 1 and time columns 0 and 3 were dropped."""
    f, t = torch.tensor([0, 2]), torch.tensor([1, 2, 4])
    tokens = torch.stack(torch.meshgrid(f, t, indexing="ij"), dim=-1).reshape(-1, 2).to(torch.int32)
    B, C = 2, 768
    time = {0: torch.arange(B * 3 * C, dtype=torch.float32).reshape(B, 3, C), 2: torch.ones(B, 3, C)}
    freq = {0: -torch.arange(B * 2 * C, dtype=torch.float32).reshape(B, 2, C), 2: torch.zeros(B, 2, C)}
    emb = {0: torch.zeros(B, 2304), 2: torch.ones(B, 2304)}
    h = HiddenStates(torch.zeros(B, 400), torch.zeros(B, 768), tokens, [3, 5], embedding=emb, time=time, freq=freq, time_index=t, freq_index=f)
    assert h.grid == (3, 5) and h.logits_dist is None and h.states == {} and h.embedding is emb and list(h.time) == [0, 2]
    for blk in (0, 2):
        a = h.on_time_axis(blk)
        assert a.shape == (B, 5, C) and a.is_contiguous()
        assert bool(torch.isnan(a[:, [0, 3]]).all()) and torch.equal(a[:, t], time[blk])
        g = h.on_freq_axis(blk)
        assert g.shape == (B, 3, C) and bool(torch.isnan(g[:, 1]).all()) and torch.equal(g[:, f], freq[blk])
    with pytest.raises(KeyError):
        h.on_time_axis(1)
    empty = HiddenStates(torch.zeros(B, 400), torch.zeros(B, 768), tokens, (3, 5))
    assert empty.embedding == {} and empty.time == {} and empty.freq == {} and empty.states == {} and empty.time_index is None
