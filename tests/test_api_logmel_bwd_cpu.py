"""CPU: argument validation of maest_logmel_bwd: null or invalid arguments come back as MAEST_ERR_INVALID with a message, before any
device work.  Runs against the gfx950 build when it is present and against the host-emulator build of the same sources."""
import os

import pytest

from maest_amd import _lib

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


def _bwd(lib, **kw):
    a = dict(wave=P1, grad=P1, B=2, S=160000, window=P1, twiddle=P1, fb_start=P1, fb_len=P1, fb_w=P1, fb_stride=16, bin_band=P1,
             bin_w=P1, work=P1, nwork=2 * 626 * 512, dwave=P1)
    a.update(kw)
    return lib.maest_logmel_bwd(a["wave"], a["grad"], a["B"], a["S"], a["window"], a["twiddle"], a["fb_start"], a["fb_len"], a["fb_w"],
                                a["fb_stride"], a["bin_band"], a["bin_w"], 1e4, 2.0, 2.5, a["work"], a["nwork"], a["dwave"], None)


@pytest.mark.parametrize("kw, msg", [
    (dict(wave=None), b"null pointer"),
    (dict(grad=None), b"null pointer"),
    (dict(window=None), b"null pointer"),
    (dict(twiddle=None), b"null pointer"),
    (dict(fb_start=None), b"null pointer"),
    (dict(fb_len=None), b"null pointer"),
    (dict(fb_w=None), b"null pointer"),
    (dict(bin_band=None), b"null pointer"),
    (dict(bin_w=None), b"null pointer"),
    (dict(work=None), b"null pointer"),
    (dict(dwave=None), b"null pointer"),
    (dict(B=0), b"bad shape"),
    (dict(S=256), b"bad shape"),
    (dict(fb_stride=0), b"bad fb_stride"),
    (dict(nwork=2 * 626 * 512 - 1), b"workspace"),
])
def test_logmel_bwd_rejects(lib, kw, msg):
    assert _bwd(lib, **kw) == 1
    assert msg in lib.maest_last_error(), lib.maest_last_error()


def test_logmel_bwd_signature_follows_the_forward():
    """The new entry sits right behind maest_logmel in the binding table, as in the header, and the ABI version is unchanged."""
    names = list(_lib.SIGNATURES)
    assert names[names.index("maest_logmel") + 1] == "maest_logmel_bwd"
    assert _lib.ABI_VERSION == 9
