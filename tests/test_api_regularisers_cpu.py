"""CPU: the public contract of the training-time regularisers -- MAEST(drop_rate=, attn_drop_rate=, drop_path_rate=), the mask seed, the
Philox known answers -- and the argument validation of the new entry points (csrc/regularise.hip): invalid arguments come back as
MAEST_ERR_INVALID with a message, before any device work.  Runs against the gfx950 build when it is present and against the
host-emulator build of the same sources."""
import inspect
import os

import numpy as np
import pytest
import torch

from maest_amd import _lib, get_maest
from maest_amd.maest import MAEST, regulariser_seed
from tests import regulariser_cases as RC

F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
P1, P2 = 256, 512        # non-null "pointers": never dereferenced, every call below fails its checks first


# ------------------------------------------------------------------------------------------------ constructor contract
def test_constructor_names_and_defaults_are_the_references():
    sig = inspect.signature(MAEST.__init__).parameters
    for name in ("drop_rate", "attn_drop_rate", "drop_path_rate"):       # models/maest.py:452-454
        assert sig[name].default == 0.0, name
    gm = inspect.signature(get_maest).parameters
    for name in ("drop_rate", "drop_path_rate"):
        assert gm[name].default == 0.0 and gm[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    m = MAEST(depth=2)
    assert (m.drop_rate, m.attn_drop_rate, m.drop_path_rate) == (0.0, 0.0, 0.0)
    m = get_maest("discogs-maest-10s-pw-129e", pretrained=False, drop_rate=0.1, drop_path_rate=0.2)
    assert (m.drop_rate, m.drop_path_rate) == (0.1, 0.2) and m.training


def test_attention_dropout_is_not_built():
    with pytest.raises(NotImplementedError, match="fused attention kernels"):
        MAEST(depth=2, attn_drop_rate=0.1)


@pytest.mark.parametrize("kw", [dict(drop_rate=1.0), dict(drop_rate=-0.1), dict(drop_path_rate=1.5), dict(attn_drop_rate=-1.0),
                                dict(drop_path_rate=float("nan"))])
def test_rates_outside_the_unit_interval_raise(kw):
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        MAEST(depth=2, **kw)


def test_rates_are_plain_attributes_checked_again_at_use():
    m = MAEST(depth=3, drop_path_rate=0.2)
    assert m._regulariser_plan() == (0.0, m.drop_path_rates)
    m.drop_rate = 0.25                      # takes effect at the next forward
    assert m._regulariser_plan()[0] == 0.25
    m.eval()
    assert m._regulariser_plan() is None    # eval(): nothing is applied
    m.train()
    m.drop_rate = m.drop_path_rate = 0.0
    assert m._regulariser_plan() is None
    m.attn_drop_rate = 0.1
    with pytest.raises(NotImplementedError):
        m._regulariser_plan()
    m.attn_drop_rate, m.drop_rate = 0.0, 1.0
    with pytest.raises(ValueError):
        m._regulariser_plan()


def test_no_new_state():
    plain, reg = MAEST(depth=2), MAEST(depth=2, drop_rate=0.1, drop_path_rate=0.1)
    a, b = plain.state_dict(), reg.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert [n for n, _ in plain.named_buffers()] == [n for n, _ in reg.named_buffers()]
    assert len(list(reg.parameters())) == len(list(plain.parameters()))


def test_clone_and_deepcopy_carry_the_rates():
    import copy
    m = MAEST(depth=2, drop_rate=0.1, drop_path_rate=0.2)
    assert m._init_kwargs["drop_rate"] == 0.1 and m._init_kwargs["drop_path_rate"] == 0.2 and m._init_kwargs["attn_drop_rate"] == 0.0
    m.drop_rate = 0.3                       # changed after construction: travels too
    m.set_regulariser_seed(77)
    for twin in (m.clone_weights(), copy.deepcopy(m)):
        assert (twin.drop_rate, twin.attn_drop_rate, twin.drop_path_rate) == (0.3, 0.0, 0.2)
        assert twin._reg_seed == 77


@pytest.mark.parametrize("depth,rate", [(12, 0.1), (3, 0.3), (1, 0.5), (5, 0.0)])
def test_block_rates_are_linspace(depth, rate):
    m = MAEST(depth=depth, drop_path_rate=rate)
    want = [float(torch.linspace(0, rate, depth)[i]) for i in range(depth)]
    assert m.drop_path_rates == want and m.drop_path_rates[0] == 0.0
    assert RC.block_rates(rate, depth) == want


# ------------------------------------------------------------------------------------------------ seed
def test_seed_derivation_is_a_pure_function_that_separates_ranks():
    s = [regulariser_seed(1234, r) for r in range(16)]
    assert s == [regulariser_seed(1234, r) for r in range(16)]
    assert len(set(s)) == 16 and all(0 <= v < 2 ** 64 for v in s)
    assert regulariser_seed(1234, 0) != regulariser_seed(1235, 0)
    # neighbouring ranks do not get neighbouring keys: both 32-bit key words differ
    for a, b in zip(s, s[1:]):
        assert (a & 0xFFFFFFFF) != (b & 0xFFFFFFFF) and (a >> 32) != (b >> 32)


def test_set_regulariser_seed():
    m = MAEST(depth=2, drop_rate=0.1)
    assert m._reg_seed is None
    assert m.set_regulariser_seed(2 ** 64 + 5) is m and m._reg_seed == 5
    st = m._regulariser_state(torch.device("cpu"))
    assert st.dtype == torch.int32 and st.numpy().view(np.uint32).tolist() == [5, 0, 0, 0]
    st[2] = 9                                # steps taken
    m.set_regulariser_seed((7 << 32) | 3)    # in place (a captured graph holds the buffer), the step restarts
    assert m._regulariser_state(torch.device("cpu")) is st and st.numpy().view(np.uint32).tolist() == [3, 7, 0, 0]
    # without a call: derived once from torch.initial_seed() (rank 0 outside a process group)
    m2 = MAEST(depth=2, drop_rate=0.1)
    m2._regulariser_state(torch.device("cpu"))
    assert m2._reg_seed == regulariser_seed(torch.initial_seed(), 0)


# ------------------------------------------------------------------------------------------------ generator
def test_philox_known_answers():
    for ctr, key, want in RC.KNOWN_ANSWERS:
        assert tuple(int(v) for v in RC.philox4x32_10(*ctr, *key)) == want


def test_mask_definition_basics():
    assert RC.threshold(0.0) == 0 and RC.threshold(0.5) == 2 ** 31 and RC.threshold(0.1) == int(0.1 * 4294967296.0)
    assert RC.elem_keep(1, 0, 3, 0.0, 2, 5, 768).all()
    k = RC.elem_keep(1, 0, 3, 0.5, 2, 5, 768)
    # coordinates, not layout: the head-token rows of a clip draw the masks of tokens 0 and 1
    assert np.array_equal(RC.elem_keep(1, 0, 3, 0.5, 2, 5, 768, tokens=[0, 1]), k[:, :2])
    assert not np.array_equal(k, RC.elem_keep(1, 1, 3, 0.5, 2, 5, 768)) and not np.array_equal(k, RC.elem_keep(1, 0, 4, 0.5, 2, 5, 768))
    assert not np.array_equal(k, RC.elem_keep(1 << 32, 0, 3, 0.5, 2, 5, 768))


# ------------------------------------------------------------------------------------------------ argument validation
def _libs():
    out = []
    if os.path.exists(_lib.LIB_PATH):
        out.append("gfx950")
    from tests.emu import build_emu
    if build_emu.available():
        out.append("emu")
    return out


@pytest.fixture(params=_libs())
def lib(request):
    if request.param == "emu":
        from tests.emu import build_emu
        _lib._testing_override(build_emu.build())
        yield _lib.load()
        _lib._testing_restore()
    else:
        yield _lib.load()


def test_new_entries_are_additive():
    names = list(_lib.SIGNATURES)
    for n in ("maest_rng_advance", "maest_dropout", "maest_drop_add_layernorm_fwd", "maest_drop_add", "maest_drop_cast"):
        assert n in names
    assert _lib.ABI_VERSION == 9
    from maest_amd import build
    assert "regularise.hip" in build.SOURCES


@pytest.mark.parametrize("args, msg", [((None, P1), b"null pointer"), ((P1, None), b"null pointer"), ((P1, P1), b"alias")])
def test_rng_advance_rejects(lib, args, msg):
    assert lib.maest_rng_advance(*args, None) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def _dropout(lib, **kw):
    a = dict(x=P1, aux=None, dtype=F32, B=2, N=10, rpc=10, C=768, thr=1 << 30, scale=1.25, site=3, snap=P2)
    a.update(kw)
    return lib.maest_dropout(a["x"], a["aux"], a["dtype"], a["B"], a["N"], a["rpc"], a["C"], a["thr"], a["scale"], a["site"], a["snap"], None)


@pytest.mark.parametrize("kw, msg", [
    (dict(x=None), b"null pointer"),
    (dict(snap=None), b"null pointer"),
    (dict(dtype=F16), b"bad dtype"),
    (dict(B=0), b"bad shape"),
    (dict(rpc=0), b"bad shape"),
    (dict(rpc=11), b"bad shape"),           # more rows than the clip has tokens
    (dict(C=772), b"multiple of 8"),
    (dict(C=0), b"multiple of 8"),
    (dict(site=-1), b"site"),
    (dict(aux=P1), b"alias"),
])
def test_dropout_rejects(lib, kw, msg):
    assert _dropout(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def _mask_args(a):
    return (a["site_e"], a["thr_e"], a["scale_e"], a["site_p"], a["thr_p"], a["scale_p"], a["snap"], None)


_MASK = dict(B=2, N=10, rpc=10, cols=768, site_e=0, thr_e=1 << 30, scale_e=1.25, site_p=1, thr_p=1 << 29, scale_p=1.1, snap=P2)
_SHAPE_CASES = [
    (dict(snap=None), b"null pointer"),
    (dict(cols=3072), b"cols must be 768"),
    (dict(B=0), b"bad shape"),
    (dict(N=0), b"bad shape"),
    (dict(rpc=12), b"bad shape"),
    (dict(site_e=-1, site_p=-1), b"both off"),
]


def _add_ln(lib, **kw):
    a = dict(_MASK, x=P1, delta=P1, ddt=BF16, xo=P1, g=P1, b=P1, y=P1, ydt=BF16, eps=1e-6)
    a.update(kw)
    return lib.maest_drop_add_layernorm_fwd(a["x"], a["delta"], a["ddt"], a["xo"], a["g"], a["b"], a["y"], a["ydt"], None, None, a["B"], a["N"],
                                            a["rpc"], a["cols"], a["eps"], *_mask_args(a))


@pytest.mark.parametrize("kw, msg", [(dict(x=None), b"null pointer"), (dict(delta=None), b"null pointer"), (dict(y=None), b"null pointer"),
                                     (dict(g=None), b"null pointer"), (dict(ddt=F16), b"bad dtype"), (dict(ydt=_lib.SPLIT3_A), b"bad dtype")]
                         + _SHAPE_CASES)
def test_drop_add_layernorm_fwd_rejects(lib, kw, msg):
    assert _add_ln(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def _add(lib, **kw):
    a = dict(_MASK, x=P1, delta=P1, ddt=F32, xo=P1)
    a.update(kw)
    return lib.maest_drop_add(a["x"], a["delta"], a["ddt"], a["xo"], a["B"], a["N"], a["rpc"], a["cols"], *_mask_args(a))


@pytest.mark.parametrize("kw, msg", [(dict(x=None), b"null pointer"), (dict(xo=None), b"null pointer"), (dict(ddt=7), b"bad dtype")] + _SHAPE_CASES)
def test_drop_add_rejects(lib, kw, msg):
    assert _add(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def _cast(lib, **kw):
    a = dict(_MASK, src=P1, dst=P2, dt=BF16, snap=1024)
    a.update(kw)
    return lib.maest_drop_cast(a["src"], a["dst"], a["dt"], a["B"], a["N"], a["rpc"], a["cols"], *_mask_args(a))


@pytest.mark.parametrize("kw, msg", [(dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer"), (dict(dt=F16), b"bad dtype"),
                                     (dict(dst=P1, dt=F32), b"alias")] + _SHAPE_CASES)
def test_drop_cast_rejects(lib, kw, msg):
    assert _cast(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()
