"""Shared by the regulariser tests (not collected by pytest): the mask generator of include/maest_hip.h restated in numpy, a plain-torch
restatement of the regularised MAEST blocks that takes those masks, and the case list of the GPU tests.

The reference draws its masks from torch's generator stream, which nothing else can reproduce: parity is defined with INJECTED masks.
tests/tools/gen_golden_regularisers.py drives the imported reference with the masks below in place of F.dropout / drop_path and records
its outputs (tests/golden/g13_regularisers.npz); tests/test_regularisers_golden_cpu.py checks `forward` below against that fixture, which
is what lets it stand in for the reference where the reference cannot travel."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import maest_oracle as O

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)

# (counter, key, output) known answers of Philox4x32-10 (Random123's kat vectors)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (broadcast together) -> uint32 [..., 4]."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & U32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0 = (k0 + np.uint64(W0)) & U32
        k1 = (k1 + np.uint64(W1)) & U32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def threshold(p):
    return int(p * 4294967296.0)


def scale(p):
    """1 / (1 - p) in fp32, the factor of a kept element."""
    return np.float32(1.0) / np.float32(1.0 - p)


def elem_keep(seed, step, site, p, B, N, C, tokens=None):
    """bool [B, len(tokens), C]: element (b, t, c) of a site of width C is kept; N = the clip's full token count, tokens = the token
    indices present (default all N)."""
    t = np.arange(N, dtype=np.uint64) if tokens is None else np.asarray(tokens, dtype=np.uint64)
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    c4 = (np.arange(C // 4, dtype=np.uint64) * np.uint64(4))[None, None, :]
    e = ((b * np.uint64(N) + t[None, :, None]) * np.uint64(C) + c4) >> np.uint64(2)
    w = philox4x32_10(e & U32, e >> np.uint64(32), site, step, *key(seed))          # [B, T, C / 4, 4]: word = c & 3
    return w.reshape(B, t.size, C) >= np.uint32(threshold(p))


def path_keep(seed, step, site, p, B):
    """bool [B]: clip b's branch is kept at a drop-path site."""
    b = np.arange(B, dtype=np.uint64)
    w = philox4x32_10(b >> np.uint64(2), 0, site, step, *key(seed))                 # [B, 4]
    return w[np.arange(B), np.arange(B) & 3] >= np.uint32(threshold(p))


class Masks:
    """The multipliers (keep * scale, fp32 torch tensors) of one forward: seed, step, batch size and full token count fixed."""

    def __init__(self, seed, step, B, N):
        self.seed, self.step, self.B, self.N = seed, step, B, N

    def elem(self, site, p, C, tokens=None):
        k = elem_keep(self.seed, self.step, site, p, self.B, self.N, C, tokens)
        return torch.from_numpy(k.astype(np.float32) * scale(p))

    def path(self, site, p):
        k = path_keep(self.seed, self.step, site, p, self.B)
        return torch.from_numpy(k.astype(np.float32) * scale(p)).reshape(self.B, 1, 1)


def block_rates(drop_path_rate, depth=O.DEPTH):
    return [float(v) for v in torch.linspace(0, drop_path_rate, depth)]


def forward(x, sd, *, drop_rate=0.0, drop_path_rate=0.0, seed=0, step=0, toffset=0, t_keep=None, transformer_block=-1,
            return_self_attention=False, distilled_type="mean", depth=O.DEPTH):
    """The oracle's train-mode forward (oracle.maest_oracle.forward) with the regularisers of models/maest.py:800, 200-207, 354-377,
    404-419 applied through the masks above.  x: [B, 1, F, T]."""
    D, p = O.EMBED_DIM, float(drop_rate)
    dpr = block_rates(drop_path_rate, depth)
    x = O.tokens_from_patches(O.patch_embed(x, sd), sd, toffset, t_keep)
    B, N, _ = x.shape
    mk = Masks(seed, step, B, N)
    if p > 0:
        x = x * mk.elem(8 * depth, p, D)                                             # pos_drop
    for i in range(depth):
        pre = f"blocks.{i}."
        a = O.attention(F.layer_norm(x, (D,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-6), sd, pre + "attn.")
        if p > 0:
            a = a * mk.elem(8 * i, p, D)                                             # proj_drop
        if i == transformer_block and return_self_attention:
            x = a
            break
        if dpr[i] > 0:
            a = a * mk.path(8 * i + 1, dpr[i])
        x = x + a
        h = F.layer_norm(x, (D,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], 1e-6)
        h = F.gelu(F.linear(h, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"]))
        if p > 0:
            h = h * mk.elem(8 * i + 2, p, O.MLP_HIDDEN)
        h = F.linear(h, sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"])
        if p > 0:
            h = h * mk.elem(8 * i + 3, p, D)
        if dpr[i] > 0:
            h = h * mk.path(8 * i + 4, dpr[i])
        x = x + h
        if i == transformer_block:
            break
    if transformer_block != -1:
        return None, torch.cat([x[:, 0, :], x[:, 1, :], torch.mean(x[:, 2:, :], dim=1)], dim=1)
    x = F.layer_norm(x, (D,), sd["norm.weight"], sd["norm.bias"], 1e-6)
    cls, dist = x[:, 0], x[:, 1]
    features = (cls + dist) / 2

    def head(z):
        z = F.layer_norm(z, (D,), sd["head.0.weight"], sd["head.0.bias"], 1e-5)
        return F.linear(z, sd["head.1.weight"], sd["head.1.bias"])
    if distilled_type == "mean":
        return head(features), features
    return head(cls), F.linear(dist, sd["head_dist.weight"], sd["head_dist.bias"]), features


# ---------------------------------------------------------------------------------------------- the G13 configuration
# (shared by the generator, the CPU check of the restatement and the GPU test through the C ABI)
G13 = dict(arch="passt_s_swa_p16_128_ap476", B=4, T=625, classes=400, s_patchout_t=30, drop_rate=0.1, drop_path_rate=0.3, seed=2, step=0,
           sd_seed=1313, x_seed=131, y_seed=132, torch_seed=1300)


def g13_inputs():
    """-> (x [B, 1, 96, T], y [B, classes]) of the G13 step, from PCG64 streams (nothing but outputs is stored)."""
    c = G13
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(c["x_seed"])).standard_normal((c["B"], 1, 96, c["T"]), dtype=np.float32))
    y = torch.from_numpy((np.random.Generator(np.random.PCG64(c["y_seed"])).random((c["B"], c["classes"])) < 0.02).astype(np.float32))
    return x, y


def g13_drop_path_outcomes():
    """{site: bool [B]} of every drop-path site of the G13 step."""
    c = G13
    out = {}
    for i, r in enumerate(block_rates(c["drop_path_rate"])):
        if r > 0:
            for s in (8 * i + 1, 8 * i + 4):
                out[s] = path_keep(c["seed"], c["step"], s, r, c["B"])
    return out


# ---------------------------------------------------------------------------------------------- GPU cases against the restatement
# name -> model / call options; every case runs in fp32, bf16 and fp16 (scaled loss)
CASES = {
    "drop_path_only": dict(drop_path_rate=0.3),
    "dropout_only": dict(drop_rate=0.1),
    "both": dict(drop_rate=0.1, drop_path_rate=0.3),
    "separated_head": dict(drop_rate=0.1, drop_path_rate=0.3, distilled_type="separated"),
    "frozen_input_grad": dict(drop_rate=0.1, drop_path_rate=0.3, frozen=True),
    "block5": dict(drop_rate=0.1, drop_path_rate=0.3, transformer_block=5),
    "block3_self_attention": dict(drop_rate=0.1, drop_path_rate=0.3, transformer_block=3, return_self_attention=True),
}
