"""CPU: the plain-torch restatement of the regularised blocks (tests/regulariser_cases.py: forward) against fixture G13 -- outputs the
IMPORTED reference gave in train mode with drop_rate = 0.1 and drop_path_rate = 0.3, its F.dropout / drop_path replaced by the numpy
masks of (seed 2, step 0) (tests/tools/gen_golden_regularisers.py).  Tolerances are those test_oracle_golden.py holds the oracle to on
G5.  This is what lets the restatement stand in for the reference in tests/test_regularisers_gpu.py."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import maest_oracle as O
from tests import regulariser_cases as RC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_regularisers.npz")


def test_g13_draws_drop_and_keep_clips():
    """The fixture's masks exercise both outcomes: some drop-path site drops a clip, some keeps one, several do both."""
    out = RC.g13_drop_path_outcomes()
    assert len(out) == 2 * (O.DEPTH - 1)            # block 0 has rate 0: no site
    assert any(not v.all() for v in out.values()) and any(v.any() for v in out.values())
    assert sum(1 for v in out.values() if v.any() and not v.all()) >= 3


def test_g13_restatement_matches_the_reference_fixture():
    g = np.load(GOLD)
    c = RC.G13
    x, y = RC.g13_inputs()
    sd = {k: v.requires_grad_(True) for k, v in O.make_state_dict(c["T"], n_classes=c["classes"], seed=c["sd_seed"]).items()}
    xo = x.clone().requires_grad_(True)
    logits, feats = RC.forward(xo, sd, drop_rate=c["drop_rate"], drop_path_rate=c["drop_path_rate"], seed=c["seed"], step=c["step"],
                               toffset=int(g["toffset"]), t_keep=g["t_keep"].tolist())
    loss = F.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) < 1e-6
    assert float((logits.detach() - torch.from_numpy(g["logits"])).abs().max()) < 1e-4
    assert float((feats.detach() - torch.from_numpy(g["features"])).abs().max()) < 1e-4
    grads = {n: p.grad for n, p in sd.items()}
    grads["_input"] = xo.grad
    names = [n for n, _ in O.state_dict_spec(c["T"], c["classes"])] + ["_input"]
    for i, n in enumerate(names):
        if g["grad_present"][i]:
            gn = float(grads[n].norm())
            assert abs(gn - float(g["grad_norm"][i])) <= 1e-4 * float(g["grad_norm"][i]) + 1e-9, n
            probe = grads[n].flatten()[:8].numpy()
            assert np.abs(probe - g["grad_probe"][i]).max() <= 1e-4 * float(np.abs(g["grad_probe"][i]).max()) + 1e-9, n
        else:
            assert grads[n] is None, n             # head_dist is unused in "mean" mode
    # the regularisers are in the numbers: the unregularised oracle is far from the fixture
    with torch.no_grad():
        plain = O.forward(x, {k: v.detach() for k, v in sd.items()}, (96, c["T"]), toffset=int(g["toffset"]), t_keep=g["t_keep"].tolist())[0]
    assert float((plain - torch.from_numpy(g["logits"])).abs().max()) > 1e-2
