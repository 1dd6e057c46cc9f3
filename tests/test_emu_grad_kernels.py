"""CPU (`-m "not gpu"`): the backward kernels of the input path -- maest_patch_im2col_bwd (col2im) and maest_embed_pool_bwd -- run
from the SAME sources under the host SIMT emulator (tests/emu) at tiny shapes, against torch autograd of a restatement of their
forwards."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maest_amd import ops
from oracle import maest_oracle as O
from tests.kernel_cases import close, rnd


def _case(B, Fdim, T, stride, seed):
    """A kept-token list that drops whole frequency rows, whole time columns and single patches, in a shuffled sequence order."""
    Fp, Tp = (Fdim - 16) // stride[0] + 1, (T - 16) // stride[1] + 1
    rng = np.random.Generator(np.random.PCG64(seed))
    f_keep = [f for f in range(Fp) if f != 1] if Fp > 2 else list(range(Fp))
    t_keep = [t for t in range(Tp) if t != Tp - 2] if Tp > 2 else list(range(Tp))
    tok = [(f, t) for f in f_keep for t in t_keep]
    tok = [tok[i] for i in sorted(rng.permutation(len(tok))[: max(1, len(tok) - 2)].tolist())]
    tok = [tok[i] for i in rng.permutation(len(tok)).tolist()]
    return torch.tensor(tok, dtype=torch.int32), Fp, Tp


def _stripes(B, Fdim, T, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t_str = torch.from_numpy(np.stack([rng.integers(0, T - 4, (B, 2)), rng.integers(0, 7, (B, 2))], -1).astype(np.int32))
    f_str = torch.from_numpy(np.stack([rng.integers(0, Fdim - 4, (B, 2)), rng.integers(0, 6, (B, 2))], -1).astype(np.int32))
    t_str[0, 0] = torch.tensor([T - 3, 8])          # runs past the right edge
    return t_str, f_str


def _im2col_ref(x, tok, stride, perm, lam, t_str, f_str):
    """The forward of maest_patch_im2col_strided restated in torch: per-clip SpecMasking, mixup, unfold, kept tokens."""
    B, Fdim, T = x.shape
    xm = x
    if t_str is not None:
        xm = torch.stack([O.spec_masking(x[b], [tuple(v) for v in t_str[b].tolist()], [tuple(v) for v in f_str[b].tolist()])
                          for b in range(B)])
    if perm is not None:
        xm = O.mixup(xm, perm.long(), lam)
    Fp, Tp = (Fdim - 16) // stride[0] + 1, (T - 16) // stride[1] + 1
    cols = F.unfold(xm.unsqueeze(1), kernel_size=16, stride=stride).reshape(B, 256, Fp, Tp)
    cols = cols[:, :, tok[:, 0].long(), tok[:, 1].long()]                  # [B, 256, P]
    return cols.permute(0, 2, 1).reshape(-1, 256)


@pytest.mark.parametrize("stride", [(10, 10), (16, 13)])
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_emu_patch_im2col_bwd(emu, stride, mix, masked):
    B, Fdim = 3, 42
    T = 46 if stride == (10, 10) else 55
    tok, Fp, Tp = _case(B, Fdim, T, stride, seed=7)
    P = tok.shape[0]
    perm = torch.tensor([2, 0, 1], dtype=torch.int32) if mix else None
    lam = torch.tensor([0.7, 0.35, 0.9]) if mix else None
    t_str, f_str = _stripes(B, Fdim, T, 9) if masked else (None, None)
    for dtype, x_dtype in ((torch.float32, torch.float32), (torch.bfloat16, torch.float16)):
        dcols = rnd((B * P, 256), 11).to(dtype)
        x = torch.zeros((B, Fdim, T), requires_grad=True)
        (_im2col_ref(x, tok, stride, perm, lam, t_str, f_str) * dcols.float()).sum().backward()
        want = x.grad
        kw = dict(perm=perm, lam=lam, t_stripes=t_str, f_stripes=f_str, stride=stride)
        got = ops.patch_im2col_bwd(dcols, (B, Fdim, T), x_dtype, tok, **kw)
        assert got.dtype == x_dtype and got.shape == (B, Fdim, T)
        close(got, want.to(x_dtype), 1e-5 if x_dtype == torch.float32 else 1e-3, 1e-5, f"col2im {dtype} -> {x_dtype}")
        # exact zeros where the forward read nothing: samples no kept patch covers, and masked samples
        ones = torch.ones((B, Fdim, T), requires_grad=True)
        _im2col_ref(ones, tok, stride, None, None, t_str, f_str).sum().backward()
        assert bool((got[ones.grad == 0] == 0).all())
        again = ops.patch_im2col_bwd(dcols, (B, Fdim, T), x_dtype, tok, **kw)
        assert torch.equal(got, again), "col2im is not bit-identical on a rerun"


def test_emu_patch_im2col_bwd_repeated_partner(emu):
    """perm need not be a permutation: a clip that two others mix in receives both partners' gradients; one that nobody picks only
    its own."""
    B, Fdim, T, stride = 3, 26, 36, (10, 10)
    Fp, Tp = (Fdim - 16) // 10 + 1, (T - 16) // 10 + 1
    tok = torch.stack(torch.meshgrid(torch.arange(Fp), torch.arange(Tp), indexing="ij"), -1).reshape(-1, 2).to(torch.int32)
    perm = torch.tensor([1, 1, 1], dtype=torch.int32)
    lam = torch.tensor([0.25, 0.5, 0.8])
    dcols = rnd((B * tok.shape[0], 256), 12)
    x = torch.zeros((B, Fdim, T), requires_grad=True)
    (_im2col_ref(x, tok, stride, perm, lam, None, None) * dcols).sum().backward()
    got = ops.patch_im2col_bwd(dcols, (B, Fdim, T), torch.float32, tok, perm=perm, lam=lam, stride=stride)
    close(got, x.grad, 1e-5, 1e-5, "col2im, repeated partner")


def test_emu_patch_im2col_bwd_single_patch_clip(emu):
    """The shortest input the model takes (16 frames: one time patch) with a frequency row dropped."""
    B, Fdim, T, stride = 2, 36, 16, (10, 10)
    tok = torch.tensor([[0, 0], [2, 0]], dtype=torch.int32)
    dcols = rnd((B * 2, 256), 13)
    x = torch.zeros((B, Fdim, T), requires_grad=True)
    (_im2col_ref(x, tok, stride, None, None, None, None) * dcols).sum().backward()
    got = ops.patch_im2col_bwd(dcols, (B, Fdim, T), torch.float32, tok, stride=stride)
    close(got, x.grad, 1e-6, 1e-6, "col2im, one time patch")
    assert bool((got[:, 16:20] == 0).all())       # rows 16..19 lie in no kept patch (row 1 of patches dropped)


@pytest.mark.parametrize("N", [3, 7])
def test_emu_embed_pool_bwd(emu, N):
    B = 2
    x = rnd((B, N, 768), 20).requires_grad_(True)
    d = rnd((B, 3 * 768), 21)
    emb = torch.cat([x[:, 0], x[:, 1], x[:, 2:].mean(dim=1)], dim=1)
    assert torch.allclose(emb, ops.embed_pool(x.detach()), rtol=1e-6, atol=1e-6)
    (emb * d).sum().backward()
    want = x.grad.reshape(B * N, 768)
    got = ops.embed_pool_bwd(d, N)
    close(got, want, 1e-6, 1e-7, "embed_pool_bwd")
    got2, lp = ops.embed_pool_bwd(d, N, lp_dtype=torch.bfloat16)
    assert torch.equal(got2, got) and torch.equal(lp, got.to(torch.bfloat16))
