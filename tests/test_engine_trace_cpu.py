"""CPU: relations between the launch sequences of the engine's paths, on traces recorded with no library and no device
(tests/tools/engine_trace.py).  No golden trace: the sequence itself stays free to change; what the docstrings of maest_amd/maest.py claim
about one path in terms of another is pinned.  Shape S of the tool's matrix: input_t = 128, batch 2, N = 2 + 9 * 12 = 110.

One model serves every trace (the weights' values play no part in one); each trace starts from a fresh engine -- cold operand-copy
caches, no training forward counted -- and an empty kept-token cache, as a fresh model would."""
import pytest
import torch

from maest_amd import _lib, ops
from maest_amd.maest import _Engine
from tests.tools import engine_trace as ET

BLOCKS = (3, 11)


@pytest.fixture(scope="module")
def net():
    return ET.build(ET.S, "bf16x3", False)


@pytest.fixture(scope="module")
def mel():
    return ET.mel(ET.S)


def _trace(net, precision, train, fn):
    net.precision = precision
    net.train(train)
    net._engine = _Engine(net)
    net._tok_cache.clear()

    def run():
        torch.manual_seed(7)
        return fn()
    return ET.trace(run)


def _eval(net, mel, precision):
    def fn():
        with torch.no_grad():
            return net(mel)
    return _trace(net, precision, False, fn)


def _train(net, mel, precision):
    def fn():
        outs = net(mel)
        outs[0].sum().backward()
        return outs
    return _trace(net, precision, True, fn)


def _without(entries, taken):
    """The C-ABI calls of a trace without those `taken` selects, the storages numbered again -> (what is left, how many were taken)."""
    calls = ET.calls(entries)
    left = [e for e in calls if not taken(e)]
    return ET.renumbered(left), len(calls) - len(left)


def test_a_trace_repeats(net, mel):
    a, b = _train(net, mel, "bf16"), _train(net, mel, "bf16")
    assert len(ET.calls(a)) > 200 and a == b


def test_auto_evaluates_in_bf16x3(net, mel):
    assert _eval(net, mel, "auto") == _eval(net, mel, "bf16x3")


def test_attention_maps_add_one_launch_per_block(net, mel):
    """"tap None: exactly the launches below" read the other way: the maps are the eager evaluation forward and, per requested block, one
    maest_attn_fwd_rows with MAEST_ATTN_PROBS (the dtype code is its sixth argument)."""
    maps = _trace(net, "bf16x3", False, lambda: net.attention_maps(mel, blocks=BLOCKS))
    left, taken = _without(maps, lambda e: e[0] == "maest_attn_fwd_rows" and e[3][5] & _lib.ATTN_PROBS)
    assert taken == len(BLOCKS) and left == ET.renumbered(ET.calls(_eval(net, mel, "bf16x3")))


def test_hidden_states_below_the_last_block_add_their_pooling_launches(net, mel):
    """... maest_gather_head_rows with MAEST_GATHER_POOLS (its dtype code is the fifth argument), one per requested block."""
    hid = _trace(net, "bf16x3", False, lambda: net.hidden_states(mel, blocks=(2, 7), pool=("time", "freq")))
    left, taken = _without(hid, lambda e: e[0] == "maest_gather_head_rows" and e[3][4] & _lib.GATHER_POOLS)
    assert taken == 2 and left == ET.renumbered(ET.calls(_eval(net, mel, "bf16x3")))


def test_ragged_with_equal_counts_is_the_plain_call(net, mel):
    keep = ET._keep((60, 60))()
    a = _trace(net, "bf16x3", False, lambda: net.forward_tokens(mel, keep, ragged=True))
    b = _trace(net, "bf16x3", False, lambda: net.forward_tokens(mel, keep))
    assert len(ET.calls(a)) > 80 and a == b


def test_no_rate_no_regulariser_launch(net, mel):
    assert net.drop_rate == 0.0 and net.drop_path_rate == 0.0
    names = {e[0] for e in ET.calls(_train(net, mel, "bf16"))}
    assert names and not {n for n in names if n.startswith(("maest_dropout", "maest_drop_", "maest_rng_"))}


def test_fp16_runs_on_the_half_precision_build(net, mel):
    half, bf16 = ET.calls(_eval(net, mel, "fp16")), ET.calls(_eval(net, mel, "bf16"))
    assert half and {e[1] for e in half} == {"f16"}
    assert bf16 and {e[1] for e in bf16} == {"bf16"}


def test_the_recorder_puts_everything_back(net, mel):
    before = (ops.call, ops._p, ops._chk, ops.torch, _lib.call, _lib._host_emulation, dict(_lib._values))
    with pytest.raises(ZeroDivisionError):
        ET.trace(lambda: 1 // 0)
    assert (ops.call, ops._p, ops._chk, ops.torch, _lib.call, _lib._host_emulation, dict(_lib._values)) == before
