"""GPU (`-m gpu`): the input-gradient chain is ONE chain.  MAEST.attention_relevance differentiates the network with the launches of the
backward that trains it: the C-ABI calls of its walk -- entry names and every argument that is not a pointer -- are, call for call, the
first calls of a real backward of the same forward, down to the proj dgrad of block 0 (the pooling steps it adds in between aside).

The one stated difference: where the walk stops, at block 0, no attention backward follows to read `delta`, so its proj dgrad is the plain
maest_gemm_nt where the backward launches maest_gemm_nt_rowdot.

The 256-frame clip of the rollout and relevance tests: batch 2, N = 2 + 9 * 25 = 227; precision "bf16", eval(), every parameter frozen, the
mel input requiring grad (a backward that, like the walk, launches no weight-gradient GEMM)."""
import ctypes

import numpy as np
import pytest
import torch

from maest_amd import _lib, get_maest, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_IN = 256
CLASS = 7
DEPTH = 12


def _recorded(net, fn):
    """-> (the C-ABI calls `fn` makes as [(entry, (non-pointer arguments))], how many of them the engine's forward made): the name `call`
    inside maest_amd.ops is replaced for the duration, the mechanism of tests/guard.py."""
    calls, forward_end = [], []
    real_call, real_forward = ops.call, net._engine.forward

    def call(name, *args):
        sig = _lib.SIGNATURES[name]
        assert len(args) == len(sig), (name, len(args), len(sig))
        calls.append((name, tuple(getattr(a, "value", a) for a, ty in zip(args, sig) if ty is not ctypes.c_void_p)))
        return real_call(name, *args)

    def forward(*a, **kw):
        out = real_forward(*a, **kw)
        forward_end.append(len(calls))
        return out

    ops.call, net._engine.forward = call, forward
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.call = real_call
        del net._engine.forward
    assert len(forward_end) == 1, "one engine forward per recorded case"
    return calls, forward_end[0]


def test_the_relevance_walk_is_a_prefix_of_the_backward():
    torch.manual_seed(11)
    net = get_maest("passt_s_swa_p16_128_ap476", pretrained=False, input_t=T_IN, precision="bf16").to(DEV).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    mel = torch.from_numpy(np.random.Generator(np.random.PCG64(602)).standard_normal((2, 1, 96, T_IN), dtype=np.float32)).to(DEV)
    x = mel.clone().requires_grad_(True)

    def backward():
        logits, _ = net(x)
        logits[:, CLASS].sum().backward()

    a, fwd_a = _recorded(net, backward)
    b, fwd_b = _recorded(net, lambda: net.attention_relevance(mel, CLASS))
    assert x.grad is not None and fwd_a > 0 and fwd_b > 0
    a, b = a[fwd_a:], b[fwd_b:]
    # maest_attn_bwd_rows(qkv, out, dout, lse, delta, dqkv, B, N, code, scale, q_rows, stream): the code is the third non-pointer argument
    pooling = [c for c in b if c[0] == "maest_attn_bwd_rows" and c[1][2] & _lib.ATTN_APPLY]
    b = [c for c in b if c not in pooling]
    assert len(pooling) == DEPTH, "one pooling step per block"
    n = len(b)
    print(f"backward: {len(a)} calls; walk: {n} calls + {len(pooling)} pooling steps")
    assert n >= DEPTH * 6 and len(a) > n
    for k, (got, want) in enumerate(zip(b[:-1], a[:n - 1])):
        assert got == want, f"call {k} of the chain: the walk launches {got}, the backward {want}"
    # ... which ends at block 0's proj dgrad: blocks 10 .. 0 of the backward produce delta there (the last block runs on the head rows),
    # and one attention backward, block 0's, is still to come
    assert b[-1][0] == "maest_gemm_nt" and a[n - 1][0] == "maest_gemm_nt_rowdot", (b[-1], a[n - 1])
    assert sum(c[0] == "maest_gemm_nt_rowdot" for c in a[:n]) == DEPTH - 1
    assert sum(c[0] == "maest_attn_bwd_rows" for c in a[n:]) == 1
