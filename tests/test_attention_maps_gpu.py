"""GPU (`-m gpu`): MAEST.attention_maps against the oracle's softmax(q k^T * scale) of every block, and what the call must leave alone.

Expected maps: the oracle's block inputs (tokens_from_patches for block 0, forward_features(probes=) for the others), then F.layer_norm ->
F.linear(qkv) -> softmax as oracle.attention computes it -- once in float64 (P64) and once in fp32 (P32) on the same state dict.
  precision="fp32":  |P - P64| <= 4 max |P32 - P64| + 2^-100 per block: four times torch's own fp32 error, the yardstick of
                     tests/augment_mel_grad_cases.py (the complete maps of blocks 0, 6 and 11, and the head rows of every block)
  precision="auto":  (bf16x3) within 1e-3 (north_star) of the fp32-mode maps, relative to each row's maximum
  "bf16" / "fp16":   the deviation from the fp32-mode maps is printed, not gated (as the project treats its bf16 logits)
  every mode:        rows sum to 1 inside 2 (N + 8) 2^-24
The measured figures are kept in profiles/attention_maps.md."""
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
U = 2.0 ** -24
FLOOR = 2.0 ** -100
FULL_BLOCKS = (0, 6, 11)      # blocks whose complete [B, 12, N, N] maps are compared (the head rows: every block)
KEEP = sorted(np.random.Generator(np.random.PCG64(504)).permutation(62)[:32].tolist())      # the pinned time columns of the train() case


def randn(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def state_dict():
    return O.make_state_dict(625, seed=501)


@functools.lru_cache(maxsize=None)
def mel():
    return randn((2, 1, 96, 626), 502)


def make(precision, train=False, **kw):
    net = get_maest(ARCH, pretrained=False, input_t=625, precision=precision, **kw)
    net.load_state_dict(state_dict())
    return net.to(DEV).train(train)


def _block_inputs(dtype, t_keep):
    sd = {k: v.to(dtype) for k, v in state_dict().items()}
    x4 = mel().to(dtype)
    probes = []
    O.forward_features(x4, sd, toffset=0, t_keep=t_keep, probes=probes)
    return sd, [O.tokens_from_patches(O.patch_embed(x4, sd), sd, 0, t_keep)] + probes[:-1]


def _probabilities(x, sd, i):
    """softmax(q k^T * scale) of block i on its input x, as oracle.attention computes it."""
    pre = f"blocks.{i}."
    B, N, C = x.shape
    h = F.layer_norm(x, (C,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-6)
    qkv = F.linear(h, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]).reshape(B, N, 3, O.NUM_HEADS, C // O.NUM_HEADS).permute(2, 0, 3, 1, 4)
    return ((qkv[0] @ qkv[1].transpose(-2, -1)) * ((C // O.NUM_HEADS) ** -0.5)).softmax(dim=-1)


@functools.lru_cache(maxsize=None)
def expected(train=False):
    """-> {block: dict(head=P64 [B, 12, 2, N], yard_head, full=P64 [B, 12, N, N] or None, yard_full)}; yard = max |P32 - P64| over the
    same elements.  Computed once per case, shared, never modified."""
    t_keep = KEEP if train else None
    with torch.no_grad():
        sd64, in64 = _block_inputs(torch.float64, t_keep)
        sd32, in32 = _block_inputs(torch.float32, t_keep)
        out = {}
        for i in range(O.DEPTH):
            p64, p32 = _probabilities(in64[i], sd64, i), _probabilities(in32[i], sd32, i).double()
            d = (p32 - p64).abs()
            out[i] = dict(head=p64[:, :, :2].clone(), yard_head=float(d[:, :, :2].max()), yard_full=float(d.max()),
                          full=p64 if i in FULL_BLOCKS else None)
    return out


@functools.lru_cache(maxsize=None)
def fp32_mode_maps():
    """The maps of the precision="fp32" model: what the other modes are compared with."""
    r = make("fp32").attention_maps(mel().to(DEV), queries="all")
    return {i: p.cpu() for i, p in r.maps.items()}


def _rows_sum_to_one(p, what):
    N = p.shape[-1]
    d = float((p.double().sum(-1) - 1).abs().max())
    assert d <= 2 * (N + 8) * U, f"{what}: a row sums to 1 +- {d:.3e} (limit {2 * (N + 8) * U:.1e})"
    return d


def _gate_fp32(what, p, p64, yard):
    err = float((p.double().cpu() - p64).abs().max())
    print(f"  {what}: max |P - P64| {err:.3e} = {err / yard:.2f} x torch's own fp32 error ({yard:.3e})")
    assert err <= 4 * yard + FLOOR, f"{what}: {err:.3e} is {err / yard:.2f} x torch's own fp32 error ({yard:.3e}); the gate is 4 x"
    return err / yard


def test_fp32_maps_against_the_oracle():
    net, exp = make("fp32"), expected()
    x = mel().to(DEV)
    print("precision=fp32, [2, 96, 626] eval, N = 560: max |P - P64| / max |P32 - P64| per block")
    r = net.attention_maps(x, blocks=FULL_BLOCKS, queries="all")
    assert sorted(r.maps) == list(FULL_BLOCKS)
    for i in FULL_BLOCKS:
        assert r.maps[i].shape == (2, 12, 560, 560) and r.maps[i].dtype == torch.float32 and not r.maps[i].requires_grad
        _gate_fp32(f"block {i}, every row", r.maps[i], exp[i]["full"], exp[i]["yard_full"])
        _rows_sum_to_one(r.maps[i], f"block {i}")
    r = net.attention_maps(x)
    assert sorted(r.maps) == list(range(12))
    for i in range(12):
        assert r.maps[i].shape == (2, 12, 2, 560)
        _gate_fp32(f"block {i}, head rows", r.maps[i], exp[i]["head"], exp[i]["yard_head"])
        _rows_sum_to_one(r.maps[i], f"block {i} head rows")


def test_train_mode_maps_follow_the_patchout_draws():
    """train(): the kept patches are the pinned columns, `tokens` says so, the maps are those of the oracle on the same columns, and
    to_grid puts NaN exactly at the dropped patches."""
    net, exp = make("fp32", train=True, s_patchout_t=30), expected(train=True)
    r = net.attention_maps(mel().to(DEV), blocks=[0, 6, 11], _patchout=(0, torch.tensor(KEEP)))
    N = 2 + 9 * len(KEEP)
    f, t = torch.meshgrid(torch.arange(9), torch.tensor(KEEP), indexing="ij")
    assert r.tokens.dtype == torch.int32 and torch.equal(r.tokens.cpu(), torch.stack([f, t], -1).reshape(-1, 2).int())
    assert r.grid == (9, 62)
    print("precision=fp32, train() with 32 of 62 time columns kept, N = 290")
    for i in (0, 6, 11):
        assert r.maps[i].shape == (2, 12, 2, N)
        _gate_fp32(f"block {i}, head rows", r.maps[i], exp[i]["head"], exp[i]["yard_head"])
        _rows_sum_to_one(r.maps[i], f"block {i}")
    g = r.to_grid(11, query=1)
    assert g.shape == (2, 12, 9, 62)
    dropped = torch.ones(62, dtype=torch.bool)
    dropped[KEEP] = False
    assert torch.equal(torch.isnan(g).cpu(), dropped.expand(2, 12, 9, 62))
    assert torch.equal(g[:, :, :, KEEP].reshape(2, 12, -1), r.maps[11][:, :, 1, 2:])
    with torch.no_grad():
        lg, ft = net(mel().to(DEV), _patchout=(0, torch.tensor(KEEP)))
    assert torch.equal(lg, r.logits) and torch.equal(ft, r.features)


def test_auto_maps_within_north_star_of_the_fp32_mode():
    ref = fp32_mode_maps()
    r = make("auto").attention_maps(mel().to(DEV), queries="all")
    print("precision=auto (bf16x3) against the fp32-mode maps, relative to each row's maximum")
    for i in range(12):
        p, q = r.maps[i].cpu().double(), ref[i].double()
        e = float(((p - q).abs() / q.amax(-1, keepdim=True)).max())
        print(f"  block {i}: {e:.3e}")
        assert e <= 1e-3, f"block {i}: {e:.3e} of the row maximum from the fp32-mode map"
        _rows_sum_to_one(r.maps[i], f"block {i}")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_sixteen_bit_maps_sum_to_one(precision):
    """Recorded, not gated: the deviation from the fp32-mode maps.  Gated: rows sum to 1."""
    ref = fp32_mode_maps()
    r = make(precision).attention_maps(mel().to(DEV), queries="all")
    print(f"precision={precision} against the fp32-mode maps, relative to each row's maximum (recorded, not gated)")
    for i in range(12):
        p, q = r.maps[i].cpu().double(), ref[i].double()
        assert bool(torch.isfinite(p).all())
        print(f"  block {i}: {float(((p - q).abs() / q.amax(-1, keepdim=True)).max()):.3e}")
        _rows_sum_to_one(r.maps[i], f"block {i}")


@pytest.mark.parametrize("precision", ["fp32", "auto", "bf16", "fp16"])
def test_outputs_are_those_of_forward(precision):
    net, x = make(precision), mel().to(DEV)
    with torch.no_grad():
        lg, ft = net(x)
    r = net.attention_maps(x, blocks=-1)
    assert torch.equal(r.logits, lg) and torch.equal(r.features, ft) and r.logits_dist is None
    assert not r.logits.requires_grad and list(r.maps) == [11]


def test_off_means_off():
    """A plain forward after an attention_maps call launches what it launched before it and gives bit-identical logits; the map kernel's
    timing bucket appears in the maps call only, once per requested block."""
    net, x = make("auto"), mel().to(DEV)

    def run(fn):
        with ops.KernelTimer(kinds=None) as t:
            with torch.no_grad():
                out = fn()
        torch.cuda.synchronize()
        return out, [r[0] for r in t.records]

    with torch.no_grad():
        net(x)      # (the operand copies of the weights are made by the first forward)
    (lg0, ft0), names0 = run(lambda: net(x))
    r, names_m = run(lambda: net.attention_maps(x, blocks=[2, 5, -1]))
    (lg1, ft1), names1 = run(lambda: net(x))
    assert "maest_attn_probs" not in names0 and names1 == names0
    assert torch.equal(lg1, lg0) and torch.equal(ft1, ft0) and torch.equal(r.logits, lg0)
    assert names_m.count("maest_attn_probs") == 3 and [n for n in names_m if n != "maest_attn_probs"] == names0


@pytest.mark.parametrize("queries,heads,shape", [("head", "all", (2, 12, 2, 560)), ("head", "mean", (2, 2, 560)),
                                                 ("all", "all", (2, 12, 560, 560)), ("all", "mean", (2, 560, 560))])
def test_shapes_and_the_head_mean(queries, heads, shape):
    net, x = make("fp32"), mel().to(DEV)
    r = net.attention_maps(x, blocks=3, queries=queries, heads=heads)
    assert list(r.maps) == [3] and r.maps[3].shape == shape and r.maps[3].device.type == "cuda"
    full = fp32_mode_maps()[3]
    rows = full if queries == "all" else full[:, :, :2]
    if heads == "all":
        assert torch.equal(r.maps[3].cpu(), rows)          # the head rows are the first two rows of the complete map, bit for bit
    else:
        acc = rows[:, 0].clone()
        for h in range(1, 12):
            acc = acc + rows[:, h]
        assert torch.equal(r.maps[3].cpu(), acc * torch.tensor(1.0 / 12.0, dtype=torch.float32))
    g = r.to_grid(3)
    assert g.shape == ((2, 12, 9, 62) if heads == "all" else (2, 9, 62)) and not bool(torch.isnan(g).any())
    assert r.grid == (9, 62) and r.tokens.shape == (558, 2)


def test_block_selections():
    net, x = make("auto"), mel().to(DEV)
    for blocks, want in ((None, list(range(12))), (4, [4]), (-1, [11]), ([7, -12, 3], [0, 3, 7]), (range(2), [0, 1]), ((5, 5), [5])):
        assert list(net.attention_maps(x, blocks=blocks, heads="mean").maps) == want
    for bad in (12, -13, [0, 12]):
        with pytest.raises(ValueError, match="out of range"):
            net.attention_maps(x, blocks=bad)


def test_audio_input_gives_chunk_batches():
    net = make("auto")
    wave = randn((16000 * 21,), 503).to(DEV) * 0.1      # 21 s: two complete chunks of 625 frames = 61 time patches, N = 2 + 9 * 61
    r = net.attention_maps(wave, blocks=[0], heads="mean")
    with torch.no_grad():
        lg, ft = net(wave)
    assert r.maps[0].shape == (2, 2, 551) and r.grid == (9, 61) and torch.equal(r.logits, lg) and torch.equal(r.features, ft)
    _rows_sum_to_one(r.maps[0], "audio input")


def test_separated_heads():
    net = make("auto", distilled_type="separated")
    x = mel().to(DEV)
    r = net.attention_maps(x, blocks=-1)
    with torch.no_grad():
        lg, lgd, ft = net(x)
    assert torch.equal(r.logits, lg) and torch.equal(r.logits_dist, lgd) and torch.equal(r.features, ft)
    assert r.maps[11].shape == (2, 12, 2, 560)
