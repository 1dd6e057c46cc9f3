"""GPU (`-m gpu`): MAEST.attention_heads -- the walks of attention_rollout and attention_relevance with every step pooled head by head --
on a three-block model with the first three blocks of the rollout test's state dict and its 256-frame clip: 25 time patches, N = 2 + 9 * 25 =
227 tokens (two key blocks, a ragged last query tile), batch 2.

Equalities, all bit for bit (torch.equal):
  result == attention_rollout(...).rollout for the same arguments, in every precision mode, for start="head", a [B, 8, N] start and
            blocks=(first, last): per head both kernels run the same arithmetic, and ops.heads_mean redoes the mean form's eleven adds and
            one product (include/maest_hip.h, MAEST_ATTN_APPLY_HEADS: the identity);
  result == attention_relevance(...).relevance on a model built with deterministic=True, whose backward repeats bit for bit -- asserted
            first on two attention_relevance calls, so that the equality cannot pass or fail by accident of that precondition;
  heads_mean(per_head[l]) == the step of block l: with alpha = 0 the mix returns the pooled step itself (r * 0 + y * 1, r finite and
            non-negative), so attention_rollout(start=r_l, blocks=(l, l), alpha=0).rollout is the step the mean-form kernel takes from the
            walk's row vectors r_l, which the test rebuilds from per_head by the walk's own two statements (and which must end at `result`);
  head_scores == the sums of per_head over the key tokens.

The derived limit of the float64 chain.  per_head[l][b, h] = r_l . P_h with r_l the walk's fp32 rows, known exactly (above); the model's own
attention_maps(queries="all", heads="all") gives P_h from the same qkv tensor by another kernel.  Both lie inside their bounds of the same
exact probabilities, as in tests/test_attention_rollout_gpu.py ("against the maps"), whose per-block terms are reused per head: with u =
2^-24 and t_max, a_max of the block (over all heads: an upper bound for each),

    E_blk  = ln 2 * 2 (a_max (gamma_66 + u_prod) + 4 u t_max) + (N + 8) u                 one probability of the maps kernel
    E'_blk = E_blk + ln 2 * u (4 log2 N + 2 (t_max + log2 N) + 2 (2 t_max + log2 N))      one probability of the pooling kernel
    gamma_{N + 1}                                                                         the accumulation of ONE head: at most N fmas and
                                                                                          the half-wave add (tests/attn_heads_cases.py)

where the rollout's per-block term has gamma_13 (the maps' head mean), gamma_{N + 14} (eleven head adds, the 1 / 12) and 3 u (the mix):
none of them is made on the way to per_head.  Every term is non-negative, so

    |per_head[l] - r_l . P_h (float64, on the maps)| <= (exp(E_blk + E'_blk + gamma_{N + 1}) - 1) of its own value (+ 2^-100)

with no sum over the blocks: r_l is the kernel's input, not a chained quantity.  "bf16" / "fp16": t_max and a_max are taken 1.1 times the
oracle's, the allowance of the rollout test, for its reason.  The measured shares are kept in profiles/attention_heads.md."""
import functools
import math

import pytest
import torch

from maest_amd import ops
from maest_amd.maest import MAEST, AttentionHeads
from tests import test_attention_rollout_gpu as RG

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEPTH = 3
T_IN, N_TOK = RG.T_IN, RG.N_TOK
U, LN2, FLOOR = RG.U, RG.LN2, RG.FLOOR
CLASS = 7
PRECISIONS = ["fp32", "auto", "bf16", "fp16"]
F16_GRAD_SCALE = 2.0 ** 10      # precision="fp16": keeps the gradient chain above half's subnormals (tests/test_attention_relevance_gpu.py)


@functools.lru_cache(maxsize=None)
def state_dict():
    later = tuple(f"blocks.{i}." for i in range(DEPTH, 12))
    return {k: v for k, v in RG.state_dict().items() if not k.startswith(later)}


def make(precision, **kw):
    net = MAEST(img_size=(96, T_IN), stride=(10, 10), depth=DEPTH, precision=precision, **kw)
    net.load_state_dict(state_dict())
    return net.to(DEV).eval()


def mel():
    return RG.mel().to(DEV)


def dense_start():
    return RG.randn((2, 8, N_TOK), 603).abs()


def _rebuild(h: AttentionHeads, start, alpha=None, grad_scale=1.0):
    """The walk's rows before every swept block, rebuilt from per_head by the walk's own statements -> ({block: r_l}, the end of the walk)."""
    r = start.to(DEV)
    before = {}
    for i in sorted(h.per_head, reverse=True):
        before[i] = r
        y = ops.heads_mean(h.per_head[i])
        r = torch.add(r * float(alpha), y, alpha=1.0 - float(alpha)) if alpha is not None else torch.add(r, y, alpha=1.0 / grad_scale)
    return before, r


def _check_result(h, kind, B, R, blocks):
    assert isinstance(h, AttentionHeads) and h.kind == kind
    assert list(h.per_head) == list(blocks), (list(h.per_head), list(blocks))
    assert h.result.shape == (B, R, N_TOK) and h.result.dtype == torch.float32 and not h.result.requires_grad
    assert h.result.device.type == "cuda" and bool(torch.isfinite(h.result).all())
    for y in h.per_head.values():
        assert y.shape == (B, 12, R, N_TOK) and y.dtype == torch.float32 and not y.requires_grad and y.is_contiguous()
        assert bool(torch.isfinite(y).all()) and bool((y >= 0).all())
    assert h.grid == (9, 25) and h.tokens.shape == (N_TOK - 2, 2)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_result_is_the_rollout_bit_for_bit(precision):
    net, x = make(precision), mel()
    s8 = dense_start().to(DEV)
    for kw, R, blocks in ((dict(), 2, (0, 1, 2)), (dict(alpha=0.9), 2, (0, 1, 2)), (dict(start=s8), 8, (0, 1, 2)),
                          (dict(blocks=(1, 2)), 2, (1, 2)), (dict(start=s8, blocks=(-3, -2), alpha=0.25), 8, (0, 1)),
                          (dict(blocks=(1, 1), alpha=0), 2, (1,))):
        h = net.attention_heads(x, **kw)
        want = net.attention_rollout(x, **kw)
        _check_result(h, "rollout", 2, R, blocks)
        assert torch.equal(h.result, want.rollout), f"precision={precision}, {sorted(kw)}: the end of the per-head walk is not the rollout"
        assert torch.equal(h.logits, want.logits) and torch.equal(h.features, want.features) and h.logits_dist is None
        start = kw["start"] if "start" in kw else RG.head_start(2, N_TOK)
        assert torch.equal(_rebuild(h, start, alpha=kw.get("alpha", 0.5))[1], h.result), "per_head does not rebuild the walk"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_result_is_the_relevance_bit_for_bit(precision):
    net, x = make(precision, deterministic=True), mel()
    gs = dict(grad_scale=F16_GRAD_SCALE) if precision == "fp16" else {}
    s8 = dense_start().to(DEV)
    for kw, R, blocks in ((dict(), 2, (0, 1, 2)), (dict(start=s8), 8, (0, 1, 2)), (dict(blocks=(1, 2)), 2, (1, 2))):
        a = net.attention_relevance(x, CLASS, **kw, **gs)
        b = net.attention_relevance(x, CLASS, **kw, **gs)
        assert torch.equal(a.relevance, b.relevance), "the precondition: deterministic=True makes the relevance walk repeat bit for bit"
        h = net.attention_heads(x, CLASS, **kw, **gs)
        _check_result(h, "relevance", 2, R, blocks)
        assert torch.equal(h.result, a.relevance), f"precision={precision}, {sorted(kw)}: the end of the per-head walk is not the relevance"
        assert torch.equal(h.logits, a.logits) and torch.equal(h.features, a.features)
        start = kw["start"] if "start" in kw else RG.head_start(2, N_TOK)
        assert torch.equal(_rebuild(h, start, grad_scale=gs.get("grad_scale", 1.0))[1], h.result), "per_head does not rebuild the walk"
        assert float((h.result.cpu() - start.cpu()).abs().max()) > 0, "a relevance that never left its start rows shows nothing"
    # a float target [B, C] and the alpha refusal on the device model
    t = torch.zeros(2, 400)
    t[0, 3], t[1, 9] = 1.0, -2.0
    assert torch.equal(net.attention_heads(x, t, **gs).result, net.attention_relevance(x, t, **gs).relevance)
    with pytest.raises(ValueError, match="alpha belongs to the rollout walk"):
        net.attention_heads(x, CLASS, alpha=0.9)
    assert all(p.grad is None for p in net.parameters())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mean_recovery_and_head_scores(precision):
    net, x = make(precision), mel()
    s8 = dense_start()
    h = net.attention_heads(x, start=s8.to(DEV), alpha=0.25)
    before, end = _rebuild(h, s8, alpha=0.25)
    assert torch.equal(end, h.result)
    for i in (2, 1, 0):
        step = net.attention_rollout(x, start=before[i], blocks=(i, i), alpha=0).rollout       # alpha = 0: the pooled step itself
        assert torch.equal(ops.heads_mean(h.per_head[i]), step), f"block {i}: the mean of per_head is not the step of the rollout"
    for row in (0, 5):
        s = h.head_scores(row)
        assert s.shape == (2, DEPTH, 12) and s.dtype == torch.float32
        for j in range(DEPTH):
            assert torch.equal(s[:, j], h.per_head[j][:, :, row, :].sum(-1))
    g = h.to_grid(1, 4, row=5)
    assert g.shape == (2, 9, 25) and not bool(torch.isnan(g).any()) and torch.equal(g.reshape(2, -1), h.per_head[1][:, 4, 5, 2:])
    # every head's attention rows sum to one: a head passes on exactly the mass of the walk's row, inside the limit of the rollout test's row
    # sums for one block (which holds the mean form's larger rounding count: an upper bound here)
    lim = math.expm1(RG.block_bounds(precision, N_TOK, 2, 2)[0])
    want = before[2].double().sum(-1)[:, None, :].cpu()
    d = float(((h.per_head[2].double().sum(-1).cpu() - want).abs() / want).max())
    print(f"precision={precision}: every head of block 2 passes on its row's mass within {d:.2e} relative (limit {lim:.2e})")
    assert d <= lim


def head_bound(precision, N, i):
    """exp(E_blk + E'_blk + gamma_{N + 1}) - 1 of block i: the module docstring (the terms of test_attention_rollout_gpu.block_bounds)."""
    t_max, a_max = RG.expected()[2][i]
    wide = 1.0 if precision in ("fp32", "auto") else 1.1
    t_max, a_max = wide * t_max, wide * a_max
    route = U * (4 * math.log2(N) + 2 * (t_max + math.log2(N)) + 2 * (2 * t_max + math.log2(N)))
    e_maps = LN2 * 2 * (a_max * (RG.gamma(66) + RG.U_PROD[precision]) + 4 * U * t_max) + (N + 8) * U
    return math.expm1(e_maps + (e_maps + LN2 * route) + RG.gamma(N + 1))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_head_against_a_float64_chain_over_the_models_own_maps(precision):
    """Two kernels on the same qkv tensors: r_l . P_h in float64 on the per-head maps against the pooled per-head step."""
    net, x = make(precision), mel()
    maps = net.attention_maps(x, queries="all", heads="all").maps
    for start, alpha in ((RG.head_start(2, N_TOK), 0.5), (dense_start(), 0.25)):
        h = net.attention_heads(x, start=start.to(DEV), alpha=alpha)
        before, _ = _rebuild(h, start, alpha=alpha)
        for i in (2, 1, 0):
            want = torch.einsum("brq,bhqk->bhrk", before[i].cpu().double(), maps[i].cpu().double())
            lim = head_bound(precision, N_TOK, i)
            e = float(((h.per_head[i].cpu().double() - want).abs() / (want + FLOOR / lim)).max())
            print(f"precision={precision}, R = {start.shape[1]}, block {i}: per_head against r . P_h over attention_maps: {e:.3e} relative "
                  f"(limit {lim:.3e}, share {e / lim:.3f})")
            assert e <= lim, f"block {i}: per_head differs from the chain over the model's own maps by {e:.3e} relative; the limit is {lim:.3e}"


def test_separated_heads_and_the_launches():
    """distilled_type="separated": target_dist is served and logits_dist returned; the per-head bucket appears once per swept block and the
    mean-form buckets not at all."""
    net, x = make("auto", distilled_type="separated", deterministic=True), mel()
    w = RG.randn((400,), 605)
    with ops.KernelTimer(kinds=None) as t:
        h = net.attention_heads(x, 3, target_dist=w, blocks=(1, 2))
    torch.cuda.synchronize()
    names = [r[0] for r in t.records]
    assert names.count("maest_attn_relevance_heads") == 2 and "maest_attn_relevance" not in names and "maest_attn_apply" not in names
    a = net.attention_relevance(x, 3, target_dist=w, blocks=(1, 2))
    assert torch.equal(h.result, a.relevance) and torch.equal(h.logits_dist, a.logits_dist) and h.logits_dist is not None
    with ops.KernelTimer(kinds=None) as t:
        net.attention_heads(x)
    torch.cuda.synchronize()
    names = [r[0] for r in t.records]
    assert names.count("maest_attn_apply_heads") == DEPTH and "maest_attn_apply" not in names
