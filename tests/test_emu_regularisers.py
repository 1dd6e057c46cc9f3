"""CPU (`-m "not gpu"`): the regulariser kernels (csrc/regularise.hip) under the SIMT lockstep emulator at tiny shapes, in the bf16 build
and the half build.  Masks are compared with the numpy generator of tests/regulariser_cases.py as integers (keep / drop: no tolerance);
values against the one-line torch definition of each kernel: fp32 bit-exact where no sum reorders, 1e-6 behind the LayerNorm's
reductions (as the neighbouring emulator tests); 16-bit results within one ulp of the operand type."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maest_amd import _lib, ops
from tests import kernel_cases as KC
from tests import regulariser_cases as RC

BF = torch.bfloat16
SEED = 0x9E3779B97F4A7C15


@pytest.fixture
def emu16():
    from tests.emu import build_emu
    if not build_emu.available():
        pytest.skip("host clang for the emulator build is not available")
    _lib._testing_override(build_emu.build(), build_emu.build(f16=True))
    yield "cpu"
    _lib._testing_restore()


def _snap(step):
    """A snapshot tensor of (SEED, step), as maest_rng_advance writes it."""
    return ops.rng_state(SEED, "cpu", step=step)


def _ulp16(ref):
    """One unit in the last place of the calling thread's 16-bit operand type at |ref| (bf16: 8 significand bits, half: 11)."""
    bits = 11 if KC.f16_build() else 8
    return torch.maximum(torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - (bits - 1)), torch.tensor(2.0 ** -24))


def _close16(got, ref, what, atol=0.0):
    """Within one ulp of the operand type (+ `atol`: the fp32 band of a reference whose sums reorder, as in the fp32 tests)."""
    err = (KC.f32(got) - ref).abs()
    assert bool((err <= _ulp16(ref) + atol).all()), (what, float(err.max()))


def test_emu_rng_advance_snapshots_then_steps(emu):
    st = ops.rng_state(SEED, "cpu", step=0xFFFFFFFE)
    a = ops.rng_advance(st)
    b = ops.rng_advance(st)
    c = ops.rng_advance(st)
    u = lambda t: t.numpy().view(np.uint32).tolist()
    lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
    assert u(a) == [lo, hi, 0xFFFFFFFE, 0] and u(b) == [lo, hi, 0xFFFFFFFF, 0] and u(c) == [lo, hi, 0, 0]      # consecutive, wrapping
    assert u(st) == [lo, hi, 1, 0]


@pytest.mark.parametrize("C", [768, 3072])
@pytest.mark.parametrize("rpc", [7, 2])          # dense (N = 7 rows per clip) and the head-token layout (tokens 0, 1 of every clip)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_emu_dropout_mask_is_the_numpy_mask(emu, C, rpc, p):
    B, N = 3, 7
    for site, step in ((8 * 11 + 2, 0), (96, 0), (96, 1)):       # two sites, two steps
        want = RC.elem_keep(SEED, step, site, p, B, N, C, tokens=range(rpc)).reshape(B * rpc, C)
        x = torch.ones(B * rpc, C)
        aux = torch.full((B * rpc, C), 2.0)
        ops.dropout_(x, aux, B, N, rpc, site, p, _snap(step))
        assert np.array_equal(x.numpy() != 0, want), (site, step)
        assert np.array_equal(x.numpy(), want.astype(np.float32) * RC.scale(p))          # keep / (1 - p), bit for bit
        assert np.array_equal(aux.numpy(), 2 * want.astype(np.float32) * RC.scale(p))
        if p == 0.0:
            assert want.all()
    # the two sites and the two steps drew different masks
    if p > 0:
        k = [RC.elem_keep(SEED, st, s, p, B, N, C) for s, st in ((90, 0), (96, 0), (96, 1))]
        assert not np.array_equal(k[0], k[1]) and not np.array_equal(k[1], k[2])


@pytest.mark.parametrize("f16", [False, True])
def test_emu_dropout_16bit(emu16, f16):
    B, N, C, p, site = 2, 5, 3072, 0.1, 42
    m = RC.Masks(SEED, 3, B, N).elem(site, p, C).reshape(B * N, C)
    with _lib.flavour("f16" if f16 else "bf16"):
        x0 = KC.rnd((B * N, C), 1)
        x = KC.lp(x0)
        ref = KC.f32(x) * m
        ones = KC.lp(torch.ones(B * N, C))
        ops.dropout_(x, ones, B, N, N, site, p, _snap(3))
        _close16(x, ref, "dropout 16-bit")
        assert np.array_equal(KC.f32(ones).numpy() != 0, m.numpy() != 0)
        _close16(ones, m, "dropout 16-bit aux")


def _branch_mult(B, N, rpc, elem, path, step):
    mk = RC.Masks(SEED, step, B, N)
    me = mk.elem(*elem, 768, tokens=range(rpc)) if elem is not None else None
    mp = mk.path(*path) if path is not None else None
    return me, mp


def _apply(d, me, mp):
    """(d * keep_e * scale_e) * keep_p * scale_p in the kernel's order."""
    if me is not None:
        d = d * me
    if mp is not None:
        d = d * mp
    return d


PARTS = [((16, 0.1), (17, 0.5)), ((16, 0.5), None), (None, (20, 0.5))]


@pytest.mark.parametrize("elem,path", PARTS)
@pytest.mark.parametrize("rpc", [6, 2])
def test_emu_drop_add_and_layernorm_fp32(emu, elem, path, rpc):
    B, N, step = 5, 6, 2
    rows = B * rpc
    me, mp = _branch_mult(B, N, rpc, elem, path, step)
    if path is not None:
        k = RC.path_keep(SEED, step, path[0], path[1], B)
        assert k.any() and not k.all()          # the case drops a clip and keeps one
    x, d = KC.rnd((rows, 768), 1), KC.rnd((rows, 768), 2)
    g, b = 1 + 0.1 * KC.rnd((768,), 3), 0.1 * KC.rnd((768,), 4)
    want = (x.reshape(B, rpc, 768) + _apply(d.reshape(B, rpc, 768), me, mp)).reshape(rows, 768)
    got = ops.drop_add(x, d, B, N, rpc, elem, path, _snap(step))
    assert torch.equal(got, want)                # no sum reorders: bit-exact
    x_new, y, mean, rstd = ops.drop_add_layernorm_fwd(x, d, g, b, 1e-6, torch.float32, B, N, rpc, elem, path, _snap(step), save_stats=True)
    assert torch.equal(x_new, want)
    KC.close(y, F.layer_norm(want, (768,), g, b, 1e-6), 1e-6, 2e-6, "drop_add_layernorm_fwd y")
    KC.close(mean, want.mean(1), 1e-6, 1e-6, "mean")
    KC.close(rstd, 1 / torch.sqrt(want.var(1, unbiased=False) + 1e-6), 1e-6, 1e-6, "rstd")
    # the gradient entering the branch: dst = src * multiplier, src untouched
    src = KC.rnd((rows, 768), 5)
    keep = src.clone()
    dst = ops.drop_cast(src, torch.float32, B, N, rpc, elem, path, _snap(step))
    assert torch.equal(src, keep) and dst.data_ptr() != src.data_ptr()
    assert torch.equal(dst, _apply(src.reshape(B, rpc, 768), me, mp).reshape(rows, 768))


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("rpc", [6, 2])
def test_emu_drop_kernels_16bit(emu16, f16, rpc):
    B, N, step = 5, 6, 1
    elem, path = (24, 0.1), (25, 0.5)
    rows = B * rpc
    me, mp = _branch_mult(B, N, rpc, elem, path, step)
    with _lib.flavour("f16" if f16 else "bf16"):
        x, d = KC.rnd((rows, 768), 1), KC.lp(KC.rnd((rows, 768), 2))
        g, b = 1 + 0.1 * KC.rnd((768,), 3), 0.1 * KC.rnd((768,), 4)
        want = (x.reshape(B, rpc, 768) + _apply(KC.f32(d).reshape(B, rpc, 768), me, mp)).reshape(rows, 768)
        assert torch.equal(ops.drop_add(x, d, B, N, rpc, elem, path, _snap(step)), want)      # 16-bit delta, fp32 stream: exact
        x_new, y = ops.drop_add_layernorm_fwd(x, d, g, b, 1e-6, BF, B, N, rpc, elem, path, _snap(step))
        assert torch.equal(x_new, want)
        ref = F.layer_norm(want, (768,), g, b, 1e-6)
        _close16(y, ref, "drop_add_layernorm_fwd 16-bit y", atol=2e-6)
        src = KC.rnd((rows, 768), 5)
        dst = ops.drop_cast(src, BF, B, N, rpc, elem, path, _snap(step))
        _close16(dst, _apply(src.reshape(B, rpc, 768), me, mp).reshape(rows, 768), "drop_cast 16-bit")
