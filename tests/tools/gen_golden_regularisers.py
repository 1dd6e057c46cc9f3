#!/usr/bin/env python
"""Generate tests/golden/g13_regularisers.npz from the IMPORTED reference (run in the authoring container only).

TEST INFRASTRUCTURE.  Drives the reference MAEST in train mode with drop_rate and drop_path_rate > 0 and pinned patchout draws (as G4 /
G5 pin theirs).  The reference's masks come from torch's generator stream and cannot be reproduced, so F.dropout and
vit_helpers.drop_path are replaced, at capture time only, by versions that apply the numpy masks of tests/regulariser_cases.py for
(seed, step 0); the reference's call order maps calls to sites: pos_drop, then for every block proj_drop, drop-path, Mlp.drop x 2,
drop-path.  Recorded: logits, features, the BCE loss, and for every parameter and the input the gradient norm and an 8-element probe
(G5's layout).  Only outputs are stored.

    python tests/tools/gen_golden_regularisers.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from oracle import maest_oracle as O  # noqa: E402
from oracle.gen_golden import import_reference  # noqa: E402
from tests import regulariser_cases as RC  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g13_regularisers.npz")


def main():
    torch.set_num_threads(8)
    c = RC.G13
    rm = import_reference()
    import models.helpers.vit_helpers as vh
    depth = O.DEPTH
    m = getattr(rm, c["arch"])(pretrained=False, num_classes=c["classes"], in_chans=1, img_size=(96, c["T"]), stride=(10, 10),
                               s_patchout_t=c["s_patchout_t"], drop_rate=c["drop_rate"], drop_path_rate=c["drop_path_rate"],
                               distilled_type="mean")
    sd = O.make_state_dict(c["T"], n_classes=c["classes"], seed=c["sd_seed"])
    m.load_state_dict(sd, strict=True)
    m.train()
    dpr = RC.block_rates(c["drop_path_rate"])
    assert isinstance(m.blocks[0].drop_path, torch.nn.Identity)
    assert all(abs(m.blocks[i].drop_path.drop_prob - dpr[i]) < 1e-12 for i in range(1, depth))
    out = RC.g13_drop_path_outcomes()
    n_mixed = sum(1 for v in out.values() if v.any() and not v.all())
    assert any(not v.all() for v in out.values()) and any(v.any() for v in out.values())
    print(f"drop-path sites: {len(out)}, of which {n_mixed} both drop and keep a clip")
    assert n_mixed >= 3

    x, y = RC.g13_inputs()
    Tp = (c["T"] - 16) // 10 + 1
    torch.manual_seed(c["torch_seed"])      # the reference's own patchout draws (models/maest.py:648-650, 684-686), replayed to pin them
    toff = torch.randint(1 + 62 - Tp, (1,)).item()
    keep = torch.randperm(Tp)[: Tp - c["s_patchout_t"]].sort().values

    # the sites in the reference's call order
    drop_sites, path_sites = [8 * depth], []
    for i in range(depth):
        drop_sites += [8 * i, 8 * i + 2, 8 * i + 3]
        if dpr[i] > 0:
            path_sites += [8 * i + 1, 8 * i + 4]
    calls = {"drop": 0, "path": 0}
    mk = {}

    def dropout(inp, p=0.5, training=True, inplace=False):
        if p == 0.0:        # Attention.attn_drop (attn_drop_rate = 0) on the probabilities [B, heads, N, N]: not a site
            assert inp.dim() == 4
            return inp
        site = drop_sites[calls["drop"]]
        calls["drop"] += 1
        assert training and abs(p - c["drop_rate"]) < 1e-12 and inp.dim() == 3
        B, N, C = inp.shape
        mk.setdefault("m", RC.Masks(c["seed"], c["step"], B, N))
        assert C == (O.MLP_HIDDEN if site % 8 == 2 and site != 8 * depth else O.EMBED_DIM), (site, C)
        return inp * mk["m"].elem(site, p, C)

    def drop_path(inp, drop_prob=0.0, training=False):
        site = path_sites[calls["path"]]
        calls["path"] += 1
        assert training and abs(drop_prob - dpr[site // 8]) < 1e-12
        keep_b = torch.from_numpy(RC.path_keep(c["seed"], c["step"], site, drop_prob, inp.shape[0]).astype(np.float32))
        return inp / (1 - drop_prob) * keep_b.reshape(-1, 1, 1)         # x / keep_prob * keep[b], the injected draw in place of torch.rand

    xg = x.clone().requires_grad_(True)
    saved = (F.dropout, vh.drop_path)
    F.dropout, vh.drop_path = dropout, drop_path
    try:
        torch.manual_seed(c["torch_seed"])
        logits, feats = m(xg)
    finally:
        F.dropout, vh.drop_path = saved
    assert calls["drop"] == len(drop_sites) == 1 + 3 * depth and calls["path"] == len(path_sites) == 2 * (depth - 1), calls
    loss = F.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    ref = {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None}

    # the restatement reproduces the reference (this is what the committed CPU test re-checks against the fixture)
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    ol, of = RC.forward(xo, sdo, drop_rate=c["drop_rate"], drop_path_rate=c["drop_path_rate"], seed=c["seed"], step=c["step"],
                        toffset=toff, t_keep=keep.tolist())
    oloss = F.binary_cross_entropy_with_logits(ol, y)
    oloss.backward()
    print(f"restatement vs reference: logits {(ol - logits).abs().max().item():.2e}, loss {abs(oloss.item() - loss.item()):.2e}, "
          f"x.grad {(xo.grad - xg.grad).abs().max().item() / xg.grad.abs().max().item():.2e}")
    names = [n for n, _ in O.state_dict_spec(c["T"], c["classes"])] + ["_input"]
    ref["_input"] = xg.grad.detach()
    gnorm, gprobe, has = [], [], []
    for n in names:
        if n in ref:
            g = ref[n]
            gnorm.append(g.norm().item())
            gprobe.append(g.flatten()[:8].numpy())
            has.append(1)
        else:
            gnorm.append(0.0)
            gprobe.append(np.zeros(8, np.float32))
            has.append(0)
    np.savez(OUT, loss=loss.detach().numpy(), logits=logits.detach().numpy(), features=feats.detach().numpy(), toffset=np.int64(toff),
             t_keep=keep.numpy(), grad_norm=np.array(gnorm, np.float32), grad_probe=np.stack(gprobe).astype(np.float32),
             grad_present=np.array(has, np.int8), grad_qkv5=ref["blocks.5.attn.qkv.weight"][:16, :16].numpy(),
             grad_fc2_11=ref["blocks.11.mlp.fc2.weight"][:8, :16].numpy(), grad_input=xg.grad[:, 0, 40:44, 100:116].numpy())
    print(OUT, os.path.getsize(OUT), "B")


if __name__ == "__main__":
    main()
