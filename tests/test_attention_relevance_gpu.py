"""GPU (`-m gpu`): MAEST.attention_relevance (gradient-weighted rollout: Chefer, Gur & Wolf 2021, the self-attention rule) against autograd
on the oracle, and what the call must leave alone.  The 256-frame clip of the rollout test: 25 time patches, N = 2 + 9 * 25 = 227, batch 2.

    s = sum(target * logits),   dP_h = ds / dP_h,   A_l = mean_h max(P_h * dP_h, 0),   r_last = start,   r_{l-1} = r_l + r_l . A_l

Expected: a test-local restatement of the oracle's block loop on its state dict and tokens (LayerNorm -> qkv -> softmax with retain_grad() on
P -> attn @ v -> proj -> MLP, the statements of oracle.block / oracle.attention), first shown to give oracle.forward's logits bit for bit,
then differentiated by torch on the host -- once in float64 (R64) and once in fp32 (R32) -- and chained by the definition.
Gates, on R and separately on (R - start)[:, :, 2:] (the patch columns lie orders of magnitude below the head columns and must not hide
behind them):
  precision="fp32":  |R - R64| <= 4 max |R32 - R64| + 2^-100: four times torch's own fp32 error, the project's yardstick
  precision="auto":  (bf16x3) within 1e-3 (north_star) of the fp32-mode result, relative to each row's maximum
  "bf16" / "fp16":   the deviation from the fp32-mode result is printed, not gated (fp16 with grad_scale = 2^10)
  every mode:        R finite and >= start elementwise; a zero target returns start bit for bit
The measured figures are kept in profiles/attention_relevance.md."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maest_amd import get_maest, ops
from oracle import maest_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = "passt_s_swa_p16_128_ap476"
T_IN = 256
N_TOK = 2 + 9 * 25
FLOOR = 2.0 ** -100
CLASS = 7                    # the target of the "mean" cases: one class index for every clip
CLASS_SEP = 3                # separated heads: a class index on logits ...
F16_GRAD_SCALE = 2.0 ** 10   # precision="fp16": the seed gradient is 1 / 768-th parts of 1e-2 weights; 2^10 keeps the chain above half's subnormals
KEEP = sorted(np.random.Generator(np.random.PCG64(604)).permutation(25)[:15].tolist())      # the pinned time columns of the train() case


def randn(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def dist_weights():
    """... and float weights [C] on logits_dist."""
    return randn((400,), 605)


@functools.lru_cache(maxsize=None)
def state_dict():
    return O.make_state_dict(T_IN, seed=601)


@functools.lru_cache(maxsize=None)
def mel():
    return randn((2, 1, 96, T_IN), 602)


def make(precision, train=False, **kw):
    net = get_maest(ARCH, pretrained=False, input_t=T_IN, precision=precision, **kw)
    net.load_state_dict(state_dict())
    return net.to(DEV).train(train)


def _restated(dtype, t_keep):
    """The oracle's forward with the attention probabilities of every block in hand -> (logits of the "mean" head, (logits, logits_dist)
    of the separated heads, [P_l])."""
    sd = {k: v.to(dtype) for k, v in state_dict().items()}
    x4 = mel().to(dtype)
    D, H = O.EMBED_DIM, O.NUM_HEADS
    x = O.tokens_from_patches(O.patch_embed(x4, sd), sd, 0, t_keep).detach().requires_grad_(True)
    B, N, _ = x.shape
    probs = []
    for i in range(O.DEPTH):
        p = f"blocks.{i}."
        h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
        qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * ((D // H) ** -0.5)).softmax(dim=-1)
        attn.retain_grad()
        probs.append(attn)
        y = (attn @ qkv[2]).transpose(1, 2).reshape(B, N, D)
        x = x + F.linear(y, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        h = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
        x = x + O.mlp(h, sd, p + "mlp.")
    x = F.layer_norm(x, (D,), sd["norm.weight"], sd["norm.bias"], 1e-6)
    cls, dist = x[:, 0], x[:, 1]

    def head(z):
        return F.linear(F.layer_norm(z, (D,), sd["head.0.weight"], sd["head.0.bias"], 1e-5), sd["head.1.weight"], sd["head.1.bias"])

    return head((cls + dist) / 2), (head(cls), F.linear(dist, sd["head_dist.weight"], sd["head_dist.bias"])), probs


def _rectified_means(s, probs):
    """A_l = mean_h max(P_h * ds / dP_h, 0) of every block, [B, N, N]."""
    for p in probs:
        p.grad = None
    s.backward(retain_graph=True)
    return [(p.detach() * p.grad).clamp_min(0).mean(1) for p in probs]


@functools.lru_cache(maxsize=None)
def expected(train=False):
    """-> {dtype: {"mean": [A_l], "separated": [A_l]}} for float64 and float32, after showing that the restatement is the oracle.  Computed
    once per case, shared, never modified."""
    t_keep = KEEP if train else None
    out = {}
    for dtype in (torch.float64, torch.float32):
        lg, (lg_cls, lg_dist), probs = _restated(dtype, t_keep)
        sd = {k: v.to(dtype) for k, v in state_dict().items()}
        with torch.no_grad():
            want = O.forward(mel().to(dtype), sd, (96, T_IN), t_keep=t_keep)
            want_sep = O.forward(mel().to(dtype), sd, (96, T_IN), t_keep=t_keep, distilled_type="separated")
        assert torch.equal(lg.detach(), want[0]), "the restated block loop does not give oracle.forward's logits"
        assert torch.equal(lg_cls.detach(), want_sep[0]) and torch.equal(lg_dist.detach(), want_sep[1])
        out[dtype] = {"mean": _rectified_means(lg[:, CLASS].sum(), probs),
                      "separated": _rectified_means(lg_cls[:, CLASS_SEP].sum() + (lg_dist * dist_weights().to(dtype)).sum(), probs)}
        for p in probs:
            p.grad = None
    return out


def chain(mats, start, first=0, last=11):
    """The recurrence of the definition on [B, N, N] matrices, in their dtype."""
    r = start.to(mats[0].dtype)
    for i in range(last, first - 1, -1):
        r = r + r @ mats[i]
    return r


def head_start(B, N):
    r = torch.zeros(B, 2, N)
    r[:, 0, 0] = 1.0
    r[:, 1, 1] = 1.0
    return r


def _views(r, start):
    return (("R", r), ("(R - start)[:, :, 2:]", (r - start.double())[:, :, 2:]))


def _gate_fp32(what, r, start, kind="mean", train=False, **kw):
    e = expected(train)
    r64 = chain(e[torch.float64][kind], start, **kw)
    r32 = chain(e[torch.float32][kind], start, **kw).double()
    r = r.detach().cpu().double()
    for (name, got), (_, w64), (_, w32) in zip(_views(r, start), _views(r64, start), _views(r32, start)):
        yard = float((w32 - w64).abs().max())
        err = float((got - w64).abs().max())
        print(f"  {what}, {name}: max |. - R64| {err:.3e} = {err / max(yard, 1e-300):.2f} x torch's own fp32 error ({yard:.3e}); "
              f"largest value {float(w64.abs().max()):.3e}")
        assert err <= 4 * yard + FLOOR, (f"{what}, {name}: {err:.3e} is {err / max(yard, 1e-300):.2f} x torch's own fp32 error ({yard:.3e}); "
                                         "the gate is 4 x")


def _check_basics(what, r, start):
    r = r.detach().cpu()
    assert bool(torch.isfinite(r).all()), f"{what}: non-finite values"
    assert bool((r >= start).all()), f"{what}: {int((r < start).sum())} values below their start values"


@functools.lru_cache(maxsize=None)
def fp32_mode_relevance():
    return make("fp32").attention_relevance(mel().to(DEV), CLASS).relevance.cpu()


def _deviation(what, r, start):
    ref = fp32_mode_relevance().double()
    out = []
    for (name, got), (_, want) in zip(_views(r.detach().cpu().double(), start), _views(ref, start)):
        e = float(((got - want).abs() / want.amax(-1, keepdim=True)).max())
        print(f"  {what} against the fp32-mode result, {name}, relative to each row's maximum: {e:.3e}")
        out.append(e)
    return out


def test_fp32_relevance_against_the_oracle():
    net, x = make("fp32"), mel().to(DEV)
    print(f"precision=fp32, [2, 96, {T_IN}] eval, N = {N_TOK}, target = class {CLASS}")
    r = net.attention_relevance(x, CLASS)
    assert r.relevance.shape == (2, 2, N_TOK) and r.relevance.dtype == torch.float32 and not r.relevance.requires_grad
    assert r.relevance.device.type == "cuda" and r.grid == (9, 25) and r.tokens.shape == (N_TOK - 2, 2) and r.logits_dist is None
    hs = head_start(2, N_TOK)
    _gate_fp32("start='head', all blocks", r.relevance, hs)
    _check_basics("start='head'", r.relevance, hs)
    g = r.to_grid(1)
    assert g.shape == (2, 9, 25) and not bool(torch.isnan(g).any()) and torch.equal(g.reshape(2, -1), r.relevance[:, 1, 2:])
    # the other forms of the same target: an index per clip, weights on the logits shared by the clips, weights per clip
    onehot = torch.zeros(400)
    onehot[CLASS] = 1.0
    for form in (torch.tensor([CLASS, CLASS]), torch.tensor([CLASS, CLASS], dtype=torch.int32, device=DEV), onehot, onehot.expand(2, -1).to(DEV)):
        assert torch.equal(net.attention_relevance(x, form).relevance, r.relevance)
    # a different class per clip: each clip is the single-class result of its own class
    other = net.attention_relevance(x, CLASS + 1).relevance
    mixed = net.attention_relevance(x, torch.tensor([CLASS, CLASS + 1])).relevance
    assert torch.equal(mixed[0], r.relevance[0]) and torch.equal(mixed[1], other[1]) and not torch.equal(other[1], r.relevance[1])
    for bad, match in ((dict(target=CLASS, start=torch.ones(2, 10)), "N = 227"), (dict(target=torch.tensor([1, 2, 3])), "B = 2 clips")):
        with pytest.raises(ValueError, match=match):
            net.attention_relevance(x, **bad)


def test_options_against_the_oracle():
    net, x = make("fp32"), mel().to(DEV)
    hs = head_start(2, N_TOK)
    r = net.attention_relevance(x, CLASS, blocks=(4, 9))
    _gate_fp32("blocks=(4, 9)", r.relevance, hs, first=4, last=9)
    _check_basics("blocks=(4, 9)", r.relevance, hs)
    r = net.attention_relevance(x, CLASS, blocks=(-1, -1))
    _gate_fp32("blocks=(-1, -1)", r.relevance, hs, first=11, last=11)
    # a tensor start [R, N], R = 3: uniform over the patch tokens, the head tokens, one patch
    s3 = torch.zeros(3, N_TOK)
    s3[0, 2:] = 1.0 / (N_TOK - 2)
    s3[1, :2] = 0.5
    s3[2, 100] = 3.0
    r = net.attention_relevance(x, CLASS, start=s3)
    assert r.relevance.shape == (2, 3, N_TOK)
    _gate_fp32("start [R, N], R = 3", r.relevance, s3.expand(2, -1, -1))
    _check_basics("start [R, N]", r.relevance, s3.expand(2, -1, -1))
    _gate_fp32("start [R, N], blocks=(4, 9)", net.attention_relevance(x, CLASS, start=s3, blocks=(4, 9)).relevance, s3.expand(2, -1, -1),
               first=4, last=9)
    # ... and [B, R, N], R = 8, on the device already
    s8 = randn((2, 8, N_TOK), 603).abs()
    r = net.attention_relevance(x, CLASS, start=s8.to(DEV))
    assert r.relevance.shape == (2, 8, N_TOK)
    _gate_fp32("start [B, R, N], R = 8", r.relevance, s8)
    _check_basics("start [B, R, N]", r.relevance, s8)


def test_auto_relevance_within_north_star_of_the_fp32_mode():
    hs = head_start(2, N_TOK)
    r = make("auto").attention_relevance(mel().to(DEV), CLASS).relevance
    for e in _deviation("precision=auto (bf16x3)", r, hs):
        assert e <= 1e-3, f"{e:.3e} of the row maximum from the fp32-mode result"
    _check_basics("auto", r, hs)


@pytest.mark.parametrize("precision,grad_scale", [("bf16", 1.0), ("fp16", F16_GRAD_SCALE)])
def test_sixteen_bit_relevance(precision, grad_scale):
    """Recorded, not gated: the deviation from the fp32-mode result.  Gated: finite, >= start."""
    hs = head_start(2, N_TOK)
    r = make(precision).attention_relevance(mel().to(DEV), CLASS, grad_scale=grad_scale).relevance
    _deviation(f"precision={precision}, grad_scale = {grad_scale:g} (recorded, not gated)", r, hs)
    _check_basics(precision, r, hs)
    assert bool((r[:, :, 2:] > 0).any()), "every patch column is zero: the gradients underflowed"


@pytest.mark.parametrize("precision", ["fp32", "auto", "bf16", "fp16"])
def test_a_zero_target_returns_the_start(precision):
    net, x = make(precision), mel().to(DEV)
    r = net.attention_relevance(x, torch.zeros(400))
    assert torch.equal(r.relevance.cpu(), head_start(2, N_TOK)), "a zero target must return the start rows bit for bit"
    s8 = randn((2, 8, N_TOK), 603).abs()
    assert torch.equal(net.attention_relevance(x, torch.zeros(2, 400), start=s8, blocks=(3, 10)).relevance.cpu(), s8)


def test_grad_scale_is_exact_in_fp32():
    net, x = make("fp32", deterministic=True), mel().to(DEV)
    a = net.attention_relevance(x, CLASS, grad_scale=1.0).relevance
    b = net.attention_relevance(x, CLASS, grad_scale=8).relevance
    c = net.attention_relevance(x, CLASS, grad_scale=0.25).relevance
    assert torch.equal(a, b) and torch.equal(a, c), "grad_scale must not change an fp32 result"
    assert torch.equal(a.cpu(), fp32_mode_relevance()), "deterministic=True must not change the relevance"


@pytest.mark.parametrize("precision,train", [("fp32", False), ("auto", False), ("bf16", False), ("auto", True), ("fp32", True)])
def test_outputs_are_those_of_a_recording_forward(precision, train):
    net, x = make(precision, train=train), mel().to(DEV)
    lg, ft = net(x)      # grad mode on, parameters require grad: a recording forward
    assert lg.requires_grad
    r = net.attention_relevance(x, CLASS, blocks=(10, 11))
    assert torch.equal(r.logits, lg.detach()) and torch.equal(r.features, ft.detach()) and r.logits_dist is None
    assert not r.logits.requires_grad and not r.features.requires_grad and not r.relevance.requires_grad and r.relevance.grad_fn is None


def _run(fn):
    with ops.KernelTimer(kinds=None) as t:
        out = fn()
    torch.cuda.synchronize()
    return out, [r[0] for r in t.records]


@pytest.mark.parametrize("precision", ["fp32", "auto", "bf16", "fp16"])
def test_off_means_off(precision):
    """No gradient is left anywhere; a plain forward, attention_maps and attention_rollout after the call launch what they launched before
    it and give bit-identical results; the call launches no weight-gradient GEMM, the pooling kernel once per swept block and the attention
    backward once per block the chain passes through."""
    net = make(precision)
    x = mel().to(DEV).requires_grad_(True)
    gs = F16_GRAD_SCALE if precision == "fp16" else 1.0

    def plain():
        with torch.no_grad():
            return net(x)

    plain()      # (the operand copies of the weights are made by the first forward)
    (lg0, ft0), names0 = _run(plain)
    m0, names_m0 = _run(lambda: net.attention_maps(x, blocks=[2, -1], heads="mean"))
    o0, names_o0 = _run(lambda: net.attention_rollout(x, blocks=(3, 9)))
    r, names_r = _run(lambda: net.attention_relevance(x, CLASS, grad_scale=gs))
    r2, names_r2 = _run(lambda: net.attention_relevance(x, CLASS, blocks=(4, 9), grad_scale=gs))
    (lg1, ft1), names1 = _run(plain)
    m1, names_m1 = _run(lambda: net.attention_maps(x, blocks=[2, -1], heads="mean"))
    o1, names_o1 = _run(lambda: net.attention_rollout(x, blocks=(3, 9)))
    assert x.grad is None and all(p.grad is None for p in net.parameters()), "the call left a gradient behind"
    assert "maest_attn_relevance" not in names0 + names_m0 + names_o0
    assert names1 == names0 and names_m1 == names_m0 and names_o1 == names_o0
    assert torch.equal(lg1, lg0) and torch.equal(ft1, ft0)
    assert all(torch.equal(m1.maps[i], m0.maps[i]) for i in (2, 11)) and torch.equal(o1.rollout, o0.rollout)
    assert "maest_gemm_tn" not in names_r + names_r2 and "maest_attn_apply" not in names_r + names_r2
    first, last = 0, 11
    assert names_r.count("maest_attn_relevance") == last - first + 1 and names_r.count("maest_attn_bwd") == last - first
    # blocks=(4, 9): six steps; the chain passes through blocks 11 .. 5 on its way to block 4, where it stops
    assert names_r2.count("maest_attn_relevance") == 6 and names_r2.count("maest_attn_bwd") == 11 - 4
    assert names_r2[-1] == "maest_attn_relevance", "the walk must end behind the step of block `first`"


def test_dropout_and_drop_path_are_not_applied():
    """A train() model with drop_rate = 0.1 and drop_path_rate = 0.1 gives the relevance of the same model with rates 0, bit for bit, and
    its mask step counter does not move (no regulariser state is even created)."""
    x, po = mel().to(DEV), (0, torch.tensor(KEEP))
    a = make("fp32", train=True, s_patchout_t=10, deterministic=True)
    b = make("fp32", train=True, s_patchout_t=10, deterministic=True, drop_rate=0.1, drop_path_rate=0.1)
    ra = a.attention_relevance(x, CLASS, _patchout=po)
    rb = b.attention_relevance(x, CLASS, _patchout=po)
    assert torch.equal(ra.relevance, rb.relevance) and torch.equal(ra.logits, rb.logits)
    assert b._reg_state == {}, "the call drew regulariser masks"
    c = make("auto", train=True, s_patchout_t=10, deterministic=True, drop_rate=0.1)
    d = make("auto", train=True, s_patchout_t=10, deterministic=True)
    assert torch.equal(c.attention_relevance(x, CLASS, _patchout=po).relevance, d.attention_relevance(x, CLASS, _patchout=po).relevance)


def test_train_mode_relevance_follows_the_patchout_draws():
    """train(): the kept patches are the pinned columns, `tokens` says so, the relevance is the oracle's on the same columns, and to_grid
    puts NaN exactly at the dropped patches."""
    net = make("fp32", train=True, s_patchout_t=10)
    r = net.attention_relevance(mel().to(DEV), CLASS, _patchout=(0, torch.tensor(KEEP)))
    N = 2 + 9 * len(KEEP)
    f, t = torch.meshgrid(torch.arange(9), torch.tensor(KEEP), indexing="ij")
    assert r.tokens.dtype == torch.int32 and torch.equal(r.tokens.cpu(), torch.stack([f, t], -1).reshape(-1, 2).int())
    assert r.grid == (9, 25) and r.relevance.shape == (2, 2, N)
    print(f"precision=fp32, train() with {len(KEEP)} of 25 time columns kept, N = {N}")
    _gate_fp32("train()", r.relevance, head_start(2, N), train=True)
    _check_basics("train()", r.relevance, head_start(2, N))
    g = r.to_grid(row=1)
    dropped = torch.ones(25, dtype=torch.bool)
    dropped[KEEP] = False
    assert g.shape == (2, 9, 25) and torch.equal(torch.isnan(g).cpu(), dropped.expand(2, 9, 25))
    assert torch.equal(g[:, :, KEEP].reshape(2, -1), r.relevance[:, 1, 2:])


def test_separated_heads():
    net = make("fp32", distilled_type="separated")
    x = mel().to(DEV)
    r = net.attention_relevance(x, CLASS_SEP, target_dist=dist_weights())
    lg, lgd, ft = net(x)
    assert torch.equal(r.logits, lg.detach()) and torch.equal(r.logits_dist, lgd.detach()) and torch.equal(r.features, ft.detach())
    hs = head_start(2, N_TOK)
    _gate_fp32("separated heads, target and target_dist", r.relevance, hs, kind="separated")
    _check_basics("separated", r.relevance, hs)
    # target alone seeds logits only: the dist token's row then gathers relevance through the blocks' attention alone
    only = net.attention_relevance(x, CLASS_SEP).relevance
    _check_basics("separated, target alone", only, hs)
    assert not torch.equal(only, r.relevance)
    with pytest.raises(ValueError, match="target_dist needs distilled_type='separated'"):
        make("fp32").attention_relevance(x, CLASS, target_dist=0)
