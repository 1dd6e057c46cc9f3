"""GPU (`-m gpu`): MAEST.hidden_states on the three-block model of tests/test_attention_heads_gpu.py -- the first three blocks of the
rollout test's state dict, its 256-frame clip: a 9 x 25 patch grid, N = 227 tokens, batch 2 -- in every precision mode.

Bit for bit (torch.equal): logits / features against the plain forward (last block not requested) and against a forward with
_engine.head_tail = False (requested); embedding[k] against forward(x, transformer_block=k) -- every block in the fp32 modes, the last
block in the 16-bit modes, every block there once _engine.split_add_eval = 0 (the truncated forward ends block k with an fp32 fc2 epilogue,
the full one carries that add, from a 16-bit fc2 output, in block k + 1's LayerNorm pass); the pools against ops.embed_pool and the
ascending fp32 loop of tests/hidden_pool_cases.py over the returned states.

Gated: the 16-bit modes' default form within the 3e-2 band tests/test_model_gpu.py gives those modes, against the "fp32" model's embedding;
"fp32" / "auto" states and pools within 1e-3 (that file's gate, its rel_err) of states composed on the CPU from the oracle's patch_embed,
tokens_from_patches and block."""
import functools

import pytest
import torch

from maest_amd import ops
from maest_amd.maest import HiddenStates
from oracle import maest_oracle as O
from tests import hidden_pool_cases as HP
from tests import test_attention_heads_gpu as AH
from tests import test_attention_rollout_gpu as RG
from tests.test_model_gpu import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEPTH, N_TOK, FK, TK = AH.DEPTH, AH.N_TOK, 9, 25
PRECISIONS = AH.PRECISIONS
FP32_MODES, LP_MODES = ["fp32", "auto"], ["bf16", "fp16"]
ALL = ("embedding", "time", "freq", "states")


def _plain(net, x):
    with torch.no_grad():
        return net(x)


def _truncated(net, x, k):
    with torch.no_grad():
        return net(x, transformer_block=k)[1]


def _check(h, B=2, blocks=(0, 1, 2), pools=ALL, Fk=FK, Tk=TK):
    assert isinstance(h, HiddenStates) and h.grid == (9, 25) and h.tokens.shape == (Fk * Tk, 2) and h.logits_dist is None
    N = 2 + Fk * Tk
    shapes = {"embedding": (B, 2304), "time": (B, Tk, 768), "freq": (B, Fk, 768), "states": (B, N, 768)}
    for name, shape in shapes.items():
        d = getattr(h, name)
        assert list(d) == (list(blocks) if name in pools else []), (name, list(d))
        for t in d.values():
            assert t.shape == shape and t.dtype == torch.float32 and t.device.type == "cuda" and not t.requires_grad
            assert bool(torch.isfinite(t).all())
    assert h.time_index.shape == (Tk,) and h.freq_index.shape == (Fk,)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_logits_are_the_forwards_when_the_last_block_is_not_requested(precision):
    net, x = AH.make(precision), AH.mel()
    want = _plain(net, x)
    h = net.hidden_states(x, blocks=(0, 1), pool=ALL)
    _check(h, blocks=(0, 1))
    assert torch.equal(h.logits, want[0]) and torch.equal(h.features, want[1])
    h = net.hidden_states(x, blocks=-2)
    _check(h, blocks=(1,), pools=("embedding",))
    assert torch.equal(h.logits, want[0]) and torch.equal(h.features, want[1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_logits_are_those_of_a_complete_last_block_when_it_is_requested(precision):
    net, x = AH.make(precision), AH.mel()
    h = net.hidden_states(x, pool=ALL)
    _check(h)
    assert net._engine.head_tail is True
    net._engine.head_tail = False
    want = _plain(net, x)
    net._engine.head_tail = True
    assert torch.equal(h.logits, want[0]) and torch.equal(h.features, want[1])
    h2 = net.hidden_states(x, blocks=[2], pool="states")
    assert torch.equal(h2.logits, want[0]) and torch.equal(h2.states[2], h.states[2])


@pytest.mark.parametrize("precision", FP32_MODES)
def test_embeddings_are_the_truncated_forwards_in_the_fp32_modes(precision):
    net, x = AH.make(precision), AH.mel()
    for pool in ("embedding", ALL):      # (ops.embed_pool alone, and the first three rows of the grid pools' launch)
        h = net.hidden_states(x, pool=pool)
        for k in range(DEPTH):
            assert torch.equal(h.embedding[k], _truncated(net, x, k)), f"precision={precision}, pool={pool}: block {k}"


@pytest.mark.parametrize("precision", LP_MODES)
def test_embeddings_in_the_sixteen_bit_modes(precision):
    net, x = AH.make(precision), AH.mel()
    assert net._engine.split_add_eval == 1
    h = net.hidden_states(x, pool=("embedding", "time"))
    assert torch.equal(h.embedding[DEPTH - 1], _truncated(net, x, DEPTH - 1)), "the last block ends both passes with the same launches"
    ref = AH.make("fp32").hidden_states(x).embedding
    for k in range(DEPTH):      # the default form: the band tests/test_model_gpu.py gives this mode
        e = rel_err(h.embedding[k], ref[k])
        print(f"precision={precision}, block {k}: embedding against the fp32 model's: {e:.3e} relative (band 3e-2)")
        assert e < 3e-2
    net._engine.split_add_eval = 0
    h0 = net.hidden_states(x)
    for k in range(DEPTH):
        assert torch.equal(h0.embedding[k], _truncated(net, x, k)), f"precision={precision}, split_add_eval = 0: block {k}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pools_are_pools_of_the_returned_states(precision):
    net, x = AH.make(precision), AH.mel()
    h = net.hidden_states(x, pool=ALL)
    assert torch.equal(h.time_index, torch.arange(TK)) and torch.equal(h.freq_index, torch.arange(FK))
    for k in range(DEPTH):
        assert torch.equal(ops.embed_pool(h.states[k]), h.embedding[k])
        ref = HP.reference(h.states[k].cpu(), FK, TK)
        assert torch.equal(h.time[k].cpu(), ref["time"]) and torch.equal(h.freq[k].cpu(), ref["freq"]), f"block {k}"
        assert torch.equal(h.embedding[k].cpu()[:, 1536:], ref["mean"])
        assert torch.equal(h.on_time_axis(k), h.time[k]) and torch.equal(h.on_freq_axis(k), h.freq[k])      # nothing dropped
    # the states are the caller's: a later forward on the same model leaves them as they are
    kept = {k: h.states[k].clone() for k in h.states}
    net.hidden_states(AH.mel().flip(0), pool=ALL)
    _plain(net, x)
    assert all(torch.equal(kept[k], h.states[k]) for k in kept)


@functools.lru_cache(maxsize=None)
def oracle_states():
    """Per-block fp32 states of the clip, composed on the CPU from the oracle's pieces: computed once, shared, never modified."""
    sd, x = AH.state_dict(), RG.mel()
    with torch.no_grad():
        s = O.tokens_from_patches(O.patch_embed(x, sd), sd)
        out = []
        for i in range(DEPTH):
            s = O.block(s, sd, i)
            out.append(s)
    return out


@pytest.mark.parametrize("precision", FP32_MODES)
def test_states_and_pools_against_the_oracle(precision):
    net, x = AH.make(precision), AH.mel()
    h = net.hidden_states(x, pool=ALL)
    for k, s in enumerate(oracle_states()):
        g = s[:, 2:].reshape(2, FK, TK, 768)
        want = {"states": s, "embedding": torch.cat([s[:, 0], s[:, 1], s[:, 2:].mean(1)], dim=1), "time": g.mean(1), "freq": g.mean(2)}
        for name, w in want.items():
            e = rel_err(getattr(h, name)[k], w)
            print(f"precision={precision}, block {k}: {name} against the oracle: {e:.3e} relative (gate 1e-3)")
            assert e < 1e-3, (name, k, e)


@pytest.mark.parametrize("precision", ["auto", "bf16"])
def test_pinned_patchout_leaves_nan_rows_on_the_time_axis(precision):
    net, x = AH.make(precision), AH.mel()
    keep = RG.KEEP
    h = net.hidden_states(x, pool=("time", "freq", "embedding"), _patchout=(0, torch.tensor(keep)))
    _check(h, pools=("time", "freq", "embedding"), Tk=len(keep))
    assert h.time_index.tolist() == keep and h.freq_index.tolist() == list(range(FK))
    dropped = [t for t in range(TK) if t not in keep]
    for k in range(DEPTH):
        a = h.on_time_axis(k)
        assert a.shape == (2, TK, 768) and bool(torch.isnan(a[:, dropped]).all()) and torch.equal(a[:, keep], h.time[k])
        assert torch.equal(h.on_freq_axis(k), h.freq[k])
    if precision == "auto":
        with torch.no_grad():
            assert torch.equal(h.embedding[1], net(x, transformer_block=1, _patchout=(0, torch.tensor(keep)))[1])


def test_chunks_of_a_long_mel_lie_on_the_batch_axis():
    net, x = AH.make("auto"), AH.mel()
    long = torch.cat([x[0, 0], x[1, 0]], dim=1)      # [96, 512]: two clip lengths
    h = net.hidden_states(long, pool=("embedding", "time"), melspectrogram_input=True)
    _check(h, pools=("embedding", "time"))
    want = net.hidden_states(x, pool=("embedding", "time"))
    assert torch.equal(h.logits, want.logits)
    assert all(torch.equal(h.embedding[k], want.embedding[k]) and torch.equal(h.time[k], want.time[k]) for k in range(DEPTH))


def test_no_side_effects_and_the_unstructured_refusal():
    net, x = AH.make("auto"), AH.mel()
    assert torch.is_grad_enabled() and all(p.requires_grad for p in net.parameters())
    h = net.hidden_states(x, pool=ALL)
    for t in (h.logits, h.features, *h.embedding.values(), *h.time.values(), *h.freq.values(), *h.states.values()):
        assert not t.requires_grad and t.grad_fn is None
    assert all(p.grad is None for p in net.parameters())
    net.train()
    net.u_patchout = 20
    with pytest.raises(ValueError, match="full frequency x time grid"):
        net.hidden_states(x, pool="time")
    torch.manual_seed(3)
    h = net.hidden_states(x, blocks=1)      # the embedding needs no grid
    assert h.embedding[1].shape == (2, 2304) and h.tokens.shape == (FK * TK - 20, 2) and h.time_index is None and h.freq_index is None
    assert not h.embedding[1].requires_grad and all(p.grad is None for p in net.parameters())
