"""GPU (`-m gpu`): dropout and stochastic depth in the training step.

  * fixture G13 (the imported reference in train mode with injected masks) through the C ABI in precision="fp32" at the project's gate;
  * fresh seeded cases against the plain-torch restatement (tests/regulariser_cases.py, pinned to the reference by
    tests/test_regularisers_golden_cpu.py) in fp32 / bf16 / fp16 under a scaled loss, at the bands of
    test_grad_paths_gpu.py::test_input_gradient_other_precisions;
  * the same masks whatever the engine's layout (head_tail, split_add), eager and replayed from a captured graph;
  * mask statistics at the headline shape; and: off means off."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maest_amd import get_maest, ops
from oracle import maest_oracle as O
from tests import regulariser_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = "passt_s_swa_p16_128_ap476"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_regularisers.npz")
NEW_ENTRIES = {"maest_rng_advance", "maest_dropout", "maest_drop_add_layernorm_fwd", "maest_drop_add", "maest_drop_cast"}


def randn(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=np.float32))


def rel_err(a, b):
    a = a.detach().float().cpu()
    b = torch.as_tensor(b).detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def make(sd, precision="fp32", **kw):
    net = get_maest(ARCH, pretrained=False, input_t=625, precision=precision, **kw)
    net.load_state_dict(sd)
    return net.to(DEV).train()


# ------------------------------------------------------------------------------------------------ 1. G13 through the C ABI
def test_g13_reference_fixture_fp32():
    g, c = np.load(GOLD), RC.G13
    sd = O.make_state_dict(c["T"], n_classes=c["classes"], seed=c["sd_seed"])
    net = make(sd, s_patchout_t=c["s_patchout_t"], drop_rate=c["drop_rate"], drop_path_rate=c["drop_path_rate"])
    net.set_regulariser_seed(c["seed"])
    x, y = RC.g13_inputs()
    xd = x.to(DEV).requires_grad_(True)
    logits, feats = net(xd, _patchout=(int(g["toffset"]), torch.from_numpy(g["t_keep"])))
    loss = F.binary_cross_entropy_with_logits(logits, y.to(DEV))
    loss.backward()
    le = abs(loss.item() - float(g["loss"])) / float(g["loss"])
    print(f"G13 fp32: loss rel {le:.2e}, logits {rel_err(logits, g['logits']):.2e}, features {rel_err(feats, g['features']):.2e}")
    assert le < 1e-3 and rel_err(logits, g["logits"]) < 1e-3 and rel_err(feats, g["features"]) < 1e-3
    grads = {n: p.grad for n, p in net.named_parameters()}
    grads["_input"] = xd.grad
    names = [n for n, _ in O.state_dict_spec(c["T"], c["classes"])] + ["_input"]
    worst = 0.0
    for i, n in enumerate(names):
        if not g["grad_present"][i]:
            assert grads[n] is None or float(grads[n].abs().max()) == 0.0, n
            continue
        gn, ref_n = float(grads[n].norm()), float(g["grad_norm"][i])
        e = abs(gn - ref_n) / max(ref_n, 1e-12)
        pe = (grads[n].flatten()[:8].cpu() - torch.from_numpy(g["grad_probe"][i])).abs().max().item()
        scale = max(float(np.abs(g["grad_probe"][i]).max()), ref_n / np.sqrt(grads[n].numel()))
        worst = max(worst, e, pe / max(scale, 1e-12))
        assert e < 1e-3, f"{n}: grad norm {gn:.4e} vs {ref_n:.4e}"
        assert pe <= 1e-3 * scale + 1e-9, f"{n}: grad probe err {pe:.3e} (scale {scale:.3e})"
    print(f"G13 fp32: worst relative gradient deviation {worst:.2e}")
    assert rel_err(grads["blocks.5.attn.qkv.weight"][:16, :16], g["grad_qkv5"]) < 1e-3
    assert rel_err(grads["blocks.11.mlp.fc2.weight"][:8, :16], g["grad_fc2_11"]) < 1e-3
    assert rel_err(xd.grad[:, 0, 40:44, 100:116], g["grad_input"]) < 1e-3


# ------------------------------------------------------------------------------------------------ 2. fresh seeded cases
def _case_inputs(B=4, T=626):
    x = randn((B, 1, 96, T), 201)
    y = (torch.from_numpy(np.random.Generator(np.random.PCG64(202)).random((B, 400))) < 0.02).float()
    yt = (torch.from_numpy(np.random.Generator(np.random.PCG64(203)).random((B, 400))) < 0.03).float()
    keep = sorted(np.random.Generator(np.random.PCG64(204)).permutation(62)[:32].tolist())
    w = randn((B, 2304), 205)
    return x, y, yt, keep, w


def _loss(outs, y, yt, w, opts):
    """The scalar a case differentiates: BCE (mean over the two heads of a separated model), or a fixed projection of the embedding."""
    if opts.get("transformer_block") is not None:
        return (outs[1] * w.to(outs[1].device)).sum() / 64.0
    if opts.get("distilled_type") == "separated":
        return (F.binary_cross_entropy_with_logits(outs[0].float(), y.to(outs[0].device))
                + F.binary_cross_entropy_with_logits(outs[1].float(), yt.to(outs[1].device))) / 2
    return F.binary_cross_entropy_with_logits(outs[0].float(), y.to(outs[0].device))


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 1e-2), ("fp16", 1e-3)])
@pytest.mark.parametrize("name", list(RC.CASES))
def test_seeded_cases_match_the_restatement(name, precision, tol):
    opts = dict(RC.CASES[name])
    frozen = opts.pop("frozen", False)
    rates = {k: opts[k] for k in ("drop_rate", "drop_path_rate") if k in opts}
    fwd = {k: opts[k] for k in ("transformer_block", "return_self_attention") if k in opts}
    dtype_kw = {"distilled_type": opts["distilled_type"]} if "distilled_type" in opts else {}
    seed, steps_before = 1000 + len(name), 2          # the compared forward is the model's THIRD: step counter 2
    sd = O.make_state_dict(625, seed=210)
    net = make(sd, precision=precision, s_patchout_t=30, **rates, **dtype_kw)
    net.set_regulariser_seed(seed)
    if frozen:
        net.requires_grad_(False)
    x, y, yt, keep, w = _case_inputs()
    po = dict(_patchout=(0, torch.tensor(keep)))
    S = 2.0 ** 14 if precision == "fp16" and not fwd else 1.0
    for _ in range(steps_before):                     # two recorded forwards advance the device step counter
        net(x.to(DEV).requires_grad_(True), **po, **fwd)
    xd = x.to(DEV).requires_grad_(True)
    outs = net(xd, **po, **fwd)
    (_loss(outs, y, yt, w, opts) * S).backward()
    # the restatement on the CPU, masks of (seed, step 2)
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    ref = RC.forward(xo, sdo, seed=seed, step=steps_before, toffset=0, t_keep=keep, **rates, **fwd, **dtype_kw)
    _loss(ref, y, yt, w, opts).backward()
    # outputs: the fp32 gate; bf16 at the 2e-2 of test_model_gpu.py's bf16 comparisons; fp16 at the 2e-3 smoke() holds its fp16 logits to
    out_tol = {"fp32": 1e-3, "bf16": 2e-2, "fp16": 2e-3}[precision]
    for a, b in zip(outs, ref):
        if a is not None:
            e = rel_err(a, b)
            print(f"{name} {precision}: output {e:.2e}")
            assert e < out_tol
    gx = xd.grad.float().cpu() / S
    assert bool(torch.isfinite(gx).all())
    e_max = rel_err(gx, xo.grad)
    e_norm = abs(float(gx.norm()) - float(xo.grad.norm())) / float(xo.grad.norm())
    print(f"{name} {precision}: x.grad worst element {e_max:.2e} of the largest, norm {e_norm:.2e}")
    if precision == "fp32":
        assert e_max < tol
    else:          # the norm within 3 tol, every element within 10 tol of the largest
        assert e_norm < 3 * tol and e_max < 10 * tol
    worst = ("", 0.0)
    for n, p in net.named_parameters():
        if frozen or sdo[n].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, n
        gp, gr = p.grad.float().cpu() / S, sdo[n].grad
        en = abs(float(gp.norm()) - float(gr.norm())) / max(float(gr.norm()), 1e-30)
        em = rel_err(gp, gr)
        worst = max(worst, (n, max(en / 3, em / 10) if precision != "fp32" else em), key=lambda t: t[1])
        if precision == "fp32":
            assert em < tol, (n, em)
        else:
            assert en < 3 * tol and em < 10 * tol, (n, en, em)
    print(f"{name} {precision}: worst parameter gradient {worst[0]} {worst[1]:.2e} (of tol {tol})")


# ------------------------------------------------------------------------------------------------ 3. layout invariance
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_masks_do_not_depend_on_the_engine_layout(precision):
    """head_tail on / off and split_add 0 / 1 / 2 with the same seed and step: outputs and every gradient agree in the band of
    test_model_gpu.py::test_last_block_on_head_tokens_equals_the_complete_evaluation (fp32: 1e-5; bf16: 2e-2, loss 3e-4) -- a mask
    that followed a buffer's rows instead of (clip, token, column) would be off by O(1)."""
    sd = O.make_state_dict(625, seed=220)
    x, y, _, keep, _ = _case_inputs(B=6)
    res = {}
    for tail, sa in ((True, 1), (False, 1), (True, 0), (True, 2), (False, 0)):
        net = make(sd, precision=precision, s_patchout_t=30, drop_rate=0.1, drop_path_rate=0.3)
        net._engine.head_tail, net._engine.split_add = tail, sa
        net.set_regulariser_seed(31)
        logits, feats = net(x.to(DEV), _patchout=(0, torch.tensor(keep)))
        loss = F.binary_cross_entropy_with_logits(logits.float(), y.to(DEV))
        loss.backward()
        res[(tail, sa)] = (loss.item(), logits.float().clone(), feats.float().clone(),
                           {n: p.grad.detach().float().clone() for n, p in net.named_parameters() if p.grad is not None})
        del net
    l0, z0, f0, g0 = res[(True, 1)]
    tol = 1e-5 if precision != "bf16" else 2e-2
    for k, (l1, z1, f1, g1) in res.items():
        assert abs(l1 - l0) <= (1e-6 if precision != "bf16" else 3e-4) * abs(l0), (k, l0, l1)
        assert rel_err(z1, z0) < tol and rel_err(f1, f0) < tol, k
        assert set(g0) == set(g1)
        worst = max(((g1[n] - g0[n]).norm().item() / max(g0[n].norm().item(), 1e-30), n) for n in g0)
        print(f"layout {k} vs (head_tail, split_add 1), {precision}: loss {l1:.7f} vs {l0:.7f}, worst gradient deviation {worst[0]:.2e} at {worst[1]}")
        assert worst[0] < tol, (k, worst)


# ------------------------------------------------------------------------------------------------ 4. graph replay
def test_graph_replay_draws_fresh_masks_and_equals_eager():
    sd = O.make_state_dict(625, seed=230)
    x, y, _, keep, _ = _case_inputs()
    xd, yd, po = x.to(DEV), y.to(DEV), (0, torch.tensor(keep))

    def three_steps(graph):
        net = make(sd, precision="bf16", s_patchout_t=30, drop_rate=0.1, drop_path_rate=0.3)
        net.set_regulariser_seed(41)
        if graph:
            net.enable_hip_graph()
        opt = torch.optim.SGD(net.parameters(), lr=1e-3)
        zs = []
        for _ in range(3):                       # graph: eager, capture, replay
            opt.zero_grad(set_to_none=True)
            logits, _ = net(xd, _patchout=po)
            F.binary_cross_entropy_with_logits(logits.float(), yd).backward()
            zs.append(logits.detach().float().clone())
            grads = {n: p.grad.detach().float().clone() for n, p in net.named_parameters() if p.grad is not None}
            opt.step()
        if graph:
            assert any(st.get("graph") is not None for k, st in net._graphs.items() if k[0] == "train"), "nothing was captured"
            # the state and the snapshot are static buffers of the graph: the step counter has moved three times, on the device
            assert net._regulariser_state(torch.device(DEV, torch.cuda.current_device())).cpu().numpy().view(np.uint32)[2] == 3
        return zs, grads

    ze, ge = three_steps(False)
    zg, gg = three_steps(True)
    for i in range(3):
        e = rel_err(zg[i], ze[i])
        print(f"step {i}: graph-mode logits vs eager {e:.2e}")
        assert e < 1e-4
    worst = max((rel_err(gg[n], ge[n]), n) for n in ge)
    print(f"third step: worst gradient deviation {worst[0]:.2e} at {worst[1]}")
    assert worst[0] < 1e-4
    # the replayed step drew other masks than the captured one (lr 1e-3 SGD moves the logits by far less)
    assert rel_err(zg[2], zg[1]) > 1e-2 and rel_err(ze[2], ze[1]) > 1e-2


# ------------------------------------------------------------------------------------------------ 5. statistics at a real size
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics_at_the_headline_shape(p):
    """[B * N, 768] of the headline training step (256 clips x 290 tokens): the kept fraction within 5 sigma of 1 - p, the agreement
    rate of two sites' masks and of two steps' masks within 5 sigma of p^2 + (1 - p)^2 (independent masks)."""
    B, N, C = 256, 290, 768
    n = B * N * C
    seed = 0x1234ABCD5678EF01

    def keep(site, step):
        x = torch.ones((B * N, C), device=DEV)
        ops.dropout_(x, None, B, N, N, site, p, ops.rng_state(seed, DEV, step=step))
        return x != 0
    k0, k1, k2 = keep(3, 0), keep(11, 0), keep(3, 1)
    sig = np.sqrt(p * (1 - p) / n)
    for k in (k0, k1, k2):
        frac = float(k.double().mean())
        print(f"p = {p}: kept fraction {frac:.6f} ({(frac - (1 - p)) / sig:+.2f} sigma)")
        assert abs(frac - (1 - p)) < 5 * sig
    q = p * p + (1 - p) * (1 - p)
    sq = np.sqrt(q * (1 - q) / n)
    for what, other in (("sites", k1), ("steps", k2)):
        agree = float((k0 == other).double().mean())
        print(f"p = {p}: agreement between two {what} {agree:.6f} ({(agree - q) / sq:+.2f} sigma)")
        assert abs(agree - q) < 5 * sq
    # and the device masks ARE the numpy masks (first clip)
    assert np.array_equal(k0[:N].cpu().numpy(), RC.elem_keep(seed, 0, 3, p, 1, N, C)[0])


# ------------------------------------------------------------------------------------------------ 6. off means off
def test_off_means_off():
    sd = O.make_state_dict(625, seed=240)
    x, y, _, keep, _ = _case_inputs()
    xd, po = x.to(DEV), dict(_patchout=(0, torch.tensor(keep)))

    def run(net, train):
        net.train(train)
        with ops.KernelTimer(kinds=None) as t:
            logits, feats = net(xd, **(po if train else {}))
            if train:
                F.binary_cross_entropy_with_logits(logits.float(), y.to(DEV)).backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), feats.detach().clone(), [r[0] for r in t.records]

    plain = make(sd, precision="bf16", s_patchout_t=30)
    zero = make(sd, precision="bf16", s_patchout_t=30, drop_rate=0.0, drop_path_rate=0.0)
    on = make(sd, precision="bf16", s_patchout_t=30, drop_rate=0.1, drop_path_rate=0.3)
    zp, fp, names_p = run(plain, True)
    zz, fz, names_z = run(zero, True)
    assert names_z == names_p and not NEW_ENTRIES & set(names_z)
    assert torch.equal(zz, zp) and torch.equal(fz, fp)
    assert not zero._reg_state, "a model with all rates 0 allocated a generator state"
    ep, efp, enames_p = run(plain, False)
    eo, efo, enames_o = run(on, False)
    assert enames_o == enames_p and not NEW_ENTRIES & set(enames_o)
    assert torch.equal(eo, ep) and torch.equal(efo, efp)
    assert not on._reg_state
    # ... and on means on: the same model in train() launches the new entry points
    _, _, names_on = run(on, True)
    assert NEW_ENTRIES <= set(names_on)
