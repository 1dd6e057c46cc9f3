"""CPU: argument validation of the input-path backward entries (maest_patch_im2col_bwd, maest_embed_pool_bwd): null or invalid
arguments come back as MAEST_ERR_INVALID with a message, before any device work.  Runs against the gfx950 build when it is present
and against the host-emulator build of the same sources."""
import os

import pytest

from maest_amd import _lib

F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
P1 = 256                 # a non-null "pointer": never dereferenced, every call below fails its checks first


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


def _col2im(lib, **kw):
    a = dict(dcols=P1, dtype=F32, B=2, F=96, T=626, sf=10, st=10, perm=None, lam=None, tok=P1, P=558, ts=None, nt=0, fs=None, nf=0,
             work=P1, nwork=9 * 62, dx=P1, xdt=F32)
    a.update(kw)
    return lib.maest_patch_im2col_bwd(a["dcols"], a["dtype"], a["B"], a["F"], a["T"], a["sf"], a["st"], a["perm"], a["lam"], a["tok"],
                                      a["P"], a["ts"], a["nt"], a["fs"], a["nf"], a["work"], a["nwork"], a["dx"], a["xdt"], None)


@pytest.mark.parametrize("kw, msg", [
    (dict(dcols=None), b"null pointer"),
    (dict(dx=None), b"null pointer"),
    (dict(tok=None), b"null pointer"),
    (dict(work=None), b"null pointer"),
    (dict(B=0), b"bad shape"),
    (dict(P=0), b"bad shape"),
    (dict(T=15), b"smaller than a patch"),
    (dict(sf=0), b"stride"),
    (dict(perm=P1), b"perm and lam"),
    (dict(dtype=F16), b"bad dtype"),
    (dict(xdt=BF16), b"fp32 or fp16"),
    (dict(nt=2), b"stripe"),
    (dict(nwork=9 * 62 - 1), b"workspace"),
    (dict(perm=P1, lam=P1), b"workspace"),          # mixup needs 2 B + 1 more
])
def test_patch_im2col_bwd_rejects(lib, kw, msg):
    assert _col2im(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


@pytest.mark.parametrize("args, msg", [
    ((None, 2, 10, P1, None, BF16), b"null pointer"),
    ((P1, 2, 10, None, None, BF16), b"null pointer"),
    ((P1, 0, 10, P1, None, BF16), b"bad shape"),
    ((P1, 2, 2, P1, None, BF16), b"bad shape"),
    ((P1, 2, 10, P1, P1, F32), b"MAEST_BF16"),
])
def test_embed_pool_bwd_rejects(lib, args, msg):
    assert lib.maest_embed_pool_bwd(*args, None) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def test_abi_version():
    assert _lib.ABI_VERSION == 9
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maest_hip.h")).read()
    assert "#define MAEST_ABI_VERSION 9" in hdr
