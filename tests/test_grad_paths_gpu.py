"""GPU (`-m gpu`): gradients through the calls the reference differentiates beyond the training step -- the input mel
(x.grad: saliency, input attribution), the embedding of an intermediate block (model(x, transformer_block=k)) and its
self-attention variant -- against the oracle's torch autograd on the CPU."""

import numpy as np
import pytest
import torch

from maest_amd import get_maest
from maest_amd.module import Module
from oracle import maest_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = "passt_s_swa_p16_128_ap476"


def randn(shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32))


def rel_err(a, b):
    a = a.detach().float().cpu()
    b = torch.as_tensor(b).detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def make(sd, precision="fp32", **kw):
    net = get_maest(ARCH, pretrained=False, input_t=625, precision=precision, **kw)
    net.load_state_dict(sd)
    return net.to(DEV)


def oracle_params(sd):
    return {k: v.clone().requires_grad_(True) for k, v in sd.items()}


def _reached(name, k, self_attention=False):
    if not name.startswith("blocks."):
        return name.startswith(("patch_embed.", "cls_token", "dist_token", "new_pos_embed", "freq_new_pos_embed", "time_new_pos_embed"))
    i, rest = name.split(".", 2)[1:]
    return int(i) < k or (int(i) == k and (not self_attention or rest.startswith(("norm1.", "attn."))))


# ---------------------------------------------------------------------------------------------------- 1. input gradient
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_input_gradient_fp32_matches_the_oracle(mode):
    sd = O.make_state_dict(625, seed=11)
    net = make(sd, s_patchout_t=20)
    net.train(mode == "train")
    B, T = 2, 626
    x = randn((B, 1, 96, T), 12)
    w = randn((B, 400), 13)
    keep = sorted(np.random.Generator(np.random.PCG64(14)).permutation(62)[:42].tolist())
    po = dict(_patchout=(0, torch.tensor(keep))) if mode == "train" else {}
    xd = x.to(DEV).requires_grad_(True)
    logits, _ = net(xd, **po)
    (logits * w.to(DEV)).sum().backward()
    assert xd.grad is not None and xd.grad.shape == x.shape
    xo = x.clone().requires_grad_(True)
    tk = dict(toffset=0, t_keep=keep) if mode == "train" else {}
    (O.forward(xo, oracle_params(sd), (96, 625), **tk)[0] * w).sum().backward()
    e = rel_err(xd.grad, xo.grad)
    print(f"x.grad fp32 {mode}: {e:.2e}")
    assert e < 1e-3
    # a frozen model: the same x.grad, and no parameter gradient at all
    g_full = xd.grad.clone()
    net.requires_grad_(False)
    net.zero_grad(set_to_none=True)
    xd2 = x.to(DEV).requires_grad_(True)
    logits, _ = net(xd2, **po)
    (logits * w.to(DEV)).sum().backward()
    assert rel_err(xd2.grad, g_full) < 1e-6
    assert all(p.grad is None for p in net.parameters())


def test_input_gradient_other_stride_fp32():
    stride = (16, 13)
    sd = O.make_state_dict(625, seed=15, stride=stride)
    with pytest.warns(UserWarning):
        net = get_maest("discogs-maest-10s-pw-129e", pretrained=False, stride_f=16, stride_t=13, precision="fp32")
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    x = randn((2, 1, 96, 500), 16)
    xd = x.to(DEV).requires_grad_(True)
    net(xd)[0].square().sum().backward()
    xo = x.clone().requires_grad_(True)
    O.forward(xo, oracle_params(sd), (96, 625), stride=stride)[0].square().sum().backward()
    assert rel_err(xd.grad, xo.grad) < 1e-3


@pytest.mark.parametrize("B,T", [(1, 16), (3, 37), (2, 333)])
def test_input_gradient_ragged_sizes_fp32(B, T):
    sd = O.make_state_dict(625, seed=17)
    net = make(sd).eval()
    x = randn((B, 1, 96, T), 18 + T)
    xd = x.to(DEV).requires_grad_(True)
    net(xd)[0].sum().backward()
    xo = x.clone().requires_grad_(True)
    O.forward(xo, oracle_params(sd), (96, 625))[0].sum().backward()
    assert rel_err(xd.grad, xo.grad) < 1e-3


# ---------------------------------------------------------------------------------------------------- 2. block-k gradients
@pytest.mark.parametrize("k,sa", [(0, False), (5, False), (11, False), (3, True)])
def test_block_embedding_gradients_fp32(k, sa):
    sd = O.make_state_dict(625, seed=20)
    net = make(sd, s_patchout_t=20).train()
    B, T = 2, 626
    x = randn((B, 1, 96, T), 21)
    w = randn((B, 2304), 22)
    keep = sorted(np.random.Generator(np.random.PCG64(23)).permutation(62)[:42].tolist())
    xd = x.to(DEV).requires_grad_(True)
    _, emb = net(xd, transformer_block=k, return_self_attention=sa, _patchout=(0, torch.tensor(keep)))
    assert emb.requires_grad and emb.shape == (B, 2304)
    (emb * w.to(DEV)).sum().backward()
    sdo = oracle_params(sd)
    xo = x.clone().requires_grad_(True)
    _, eo = O.forward(xo, sdo, (96, 625), transformer_block=k, return_self_attention=sa, toffset=0, t_keep=keep)
    assert rel_err(emb, eo) < 1e-3
    (eo * w).sum().backward()
    worst = rel_err(xd.grad, xo.grad)
    assert worst < 1e-3, worst
    for n, p in net.named_parameters():
        if _reached(n, k, sa):
            assert p.grad is not None, n
            e = rel_err(p.grad, sdo[n].grad)
            worst = max(worst, e)
            assert e < 1e-3, (n, e)
        else:
            assert p.grad is None, n
            assert sdo[n].grad is None, n
    print(f"block {k} (self-attention {sa}) fp32: worst relative gradient deviation {worst:.2e}")


# ---------------------------------------------------------------------------------------------------- 3. mixup + SpecMasking
def test_input_gradient_through_mixup_and_spec_masking_fp32():
    rng = np.random.Generator(np.random.PCG64(30))
    sd = O.make_state_dict(625, seed=30)
    net = make(sd, s_patchout_t=30).train()
    mod = Module(net=net, mixup_alpha=0.3)
    B, T = 3, 626
    x = torch.from_numpy(rng.standard_normal((B, 1, 96, T), dtype=np.float32))
    y = torch.from_numpy((rng.random((B, 400)) < 0.02).astype(np.float32))
    perm = torch.tensor([2, 0, 1])
    lam = torch.tensor([0.8, 0.6, 0.95])
    keep = sorted(rng.permutation(62)[:32].tolist())
    t_str = torch.tensor([[[10, 8], [300, 5]], [[0, 3], [620, 8]], [[100, 7], [101, 2]]], dtype=torch.int32)
    f_str = torch.tensor([[[5, 4]], [[90, 5]], [[40, 0]]], dtype=torch.int32)
    xd = x.to(DEV).requires_grad_(True)
    loss = mod.training_step((xd, None, y.to(DEV)), 0, _mixup=(perm, lam), _patchout=(0, torch.tensor(keep)),
                             _specmask=(t_str, f_str))
    loss.backward()
    xo = x.clone().requires_grad_(True)
    xm = torch.stack([O.spec_masking(xo[b], [tuple(v) for v in t_str[b].tolist()], [tuple(v) for v in f_str[b].tolist()])
                      for b in range(B)])
    want, _ = O.training_loss(xm, y, oracle_params(sd), perm, lam, toffset=0, t_keep=keep)
    want.backward()
    assert abs(loss.item() - want.item()) < 1e-5 * abs(want.item())
    e = rel_err(xd.grad, xo.grad)
    print(f"x.grad through mixup + SpecMasking fp32: {e:.2e}")
    assert e < 1e-3
    assert float(xd.grad[0, 0, :, 10:18].abs().max()) == 0.0 and float(xd.grad[1, 0, 90:95, :].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- 4. other precisions
@pytest.mark.parametrize("precision,mode,tol", [("auto", "eval", 1e-3), ("bf16", "train", 1e-2), ("fp16", "train", 1e-3)])
def test_input_gradient_other_precisions(precision, mode, tol):
    """The default mode of a grad-enabled eval() forward (bf16x3) at the fp32 gate on the largest element; the 16-bit training modes
    in the band the training-step tests (G5) give their gradients -- bf16 at tol 1e-2, fp16 (mean BCE loss scaled by 2^14, as under
    GradScaler) at tol 1e-3."""
    sd = O.make_state_dict(625, seed=40)
    net = make(sd, precision=precision, s_patchout_t=20)
    net.train(mode == "train")
    B, T = 2, 626
    x = randn((B, 1, 96, T), 41)
    y = (torch.from_numpy(np.random.Generator(np.random.PCG64(42)).random((B, 400))) < 0.02).float()
    keep = sorted(np.random.Generator(np.random.PCG64(43)).permutation(62)[:42].tolist())
    po = dict(_patchout=(0, torch.tensor(keep))) if mode == "train" else {}
    S = 2.0 ** 14 if precision == "fp16" else 1.0
    xd = x.to(DEV).requires_grad_(True)
    logits, _ = net(xd, **po)
    (torch.nn.functional.binary_cross_entropy_with_logits(logits.float(), y.to(DEV)) * S).backward()
    xo = x.clone().requires_grad_(True)
    tk = dict(toffset=0, t_keep=keep) if mode == "train" else {}
    torch.nn.functional.binary_cross_entropy_with_logits(O.forward(xo, oracle_params(sd), (96, 625), **tk)[0], y).backward()
    g = xd.grad.float().cpu() / S
    assert bool(torch.isfinite(g).all())
    e_max = rel_err(g, xo.grad)
    e_norm = abs(float(g.norm()) - float(xo.grad.norm())) / float(xo.grad.norm())
    print(f"x.grad {precision} {mode}: worst element {e_max:.2e} of the largest, norm {e_norm:.2e}")
    if precision == "auto":
        assert e_max < tol
    else:          # G5's band: the norm within 3 tol, every element within 10 tol of the largest
        assert e_norm < 3 * tol and e_max < 10 * tol


# ---------------------------------------------------------------------------------------------------- 5. long sequence
def test_block6_gradients_at_the_30s_training_shape_fp32():
    """BASELINE configs[3]'s per-clip shape: 1876 frames with s_patchout_t = 90 -> 9 x 97 patches, N = 875."""
    sd = O.make_state_dict(1875, seed=50)
    net = get_maest("discogs-maest-30s-pw-129e", pretrained=False, s_patchout_t=90, precision="fp32")
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    x = randn((1, 1, 96, 1876), 51)
    keep = sorted(np.random.Generator(np.random.PCG64(52)).permutation(187)[:97].tolist())
    w = randn((1, 2304), 53)
    xd = x.to(DEV).requires_grad_(True)
    _, emb = net(xd, transformer_block=6, _patchout=(0, torch.tensor(keep)))
    (emb * w.to(DEV)).sum().backward()
    sdo = oracle_params(sd)
    xo = x.clone().requires_grad_(True)
    _, eo = O.forward(xo, sdo, (96, 1875), transformer_block=6, toffset=0, t_keep=keep)
    (eo * w).sum().backward()
    assert rel_err(xd.grad, xo.grad) < 1e-3
    params = dict(net.named_parameters())
    for n in ("patch_embed.proj.weight", "blocks.0.attn.qkv.weight", "blocks.6.mlp.fc2.weight", "time_new_pos_embed", "blocks.6.norm2.bias"):
        assert rel_err(params[n].grad, sdo[n].grad) < 1e-3, n
    assert params["blocks.7.attn.qkv.weight"].grad is None and params["head.1.weight"].grad is None


# ---------------------------------------------------------------------------------------------------- 6. repeatability, graphs, sink
def _block_step(net, x, k=5, w=None):
    xd = x.to(DEV).requires_grad_(True)
    _, emb = net(xd, transformer_block=k)
    (emb * (w if w is not None else 1.0)).sum().backward()
    return xd.grad


def test_repeated_backward_is_bit_identical_and_graph_mode_equals_eager():
    sd = O.make_state_dict(625, seed=60)
    net = make(sd).eval()
    x = randn((2, 1, 96, 626), 61)
    w = randn((2, 2304), 62).to(DEV)
    g1 = _block_step(net, x, w=w)
    p1 = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    net.zero_grad(set_to_none=True)
    g2 = _block_step(net, x, w=w)
    assert torch.equal(g1, g2), "x.grad differs between two identical backward passes"
    for n, p in net.named_parameters():
        if n in p1:
            # (weight gradients accumulate split-K partial sums with atomics: order-only noise)
            assert rel_err(p.grad, p1[n]) < 1e-5, n
    # the saliency of a frozen model: the dgrad chain alone, bit for bit the same x.grad
    net.requires_grad_(False)
    assert torch.equal(_block_step(net, x, w=w), g1)
    net.requires_grad_(True)
    # captured graphs on: a forward whose input needs a gradient (or a truncated one) runs eagerly -- same gradients
    net.enable_hip_graph()
    for _ in range(3):
        net.zero_grad(set_to_none=True)
        assert torch.equal(_block_step(net, x, w=w), g1)
        xf = x.to(DEV).requires_grad_(True)
        net(xf)[0].sum().backward()
    net.enable_hip_graph(False)
    # a second backward through the same output raises, as for the full forward
    xd = x.to(DEV).requires_grad_(True)
    _, emb = net(xd, transformer_block=2)
    loss = emb.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward called twice"):
        loss.backward()


def test_truncated_backward_completes_with_a_gradient_sink():
    from maest_amd.dist import GradReducer
    sd = O.make_state_dict(625, seed=70)
    net = make(sd).train()
    x = randn((2, 1, 96, 626), 71)
    keep = list(range(0, 62, 2))
    w = randn((2, 2304), 72).to(DEV)

    def step():
        _, emb = net(x.to(DEV), transformer_block=4, _patchout=(0, torch.tensor(keep)))
        (emb * w).sum().backward()
    step()
    ref = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    assert "blocks.4.mlp.fc1.weight" in ref and "blocks.5.attn.qkv.weight" not in ref
    net.zero_grad(set_to_none=True)
    red = GradReducer(net.named_parameters(), bucket_mb=32)
    assert len(red.buckets) > 3
    net._grad_sink = red
    red.reset()
    step()
    red.finish()
    net._grad_sink = None
    for n, p in net.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == red.grad_buffer(n).data_ptr(), n
        if n in ref:
            d = (p.grad - ref[n]).abs().max().item()
            assert d <= 1e-5 * max(ref[n].abs().max().item(), 1e-6) + 1e-7, (n, d)
        else:
            assert float(p.grad.abs().max()) == 0.0, n
