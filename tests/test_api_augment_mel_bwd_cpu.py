"""CPU: argument validation of maest_augment_mel_bwd: null or invalid arguments come back as MAEST_ERR_INVALID with a message, before any
device work.  Runs against the gfx950 build when it is present and against the host-emulator build of the same sources."""
import os

import pytest

from maest_amd import _lib

P1 = 256                 # a non-null "pointer": never dereferenced, every call below fails its checks first
NWORK = 2 * 1000 * 1024  # B * T * 1024 for B = 2, S = 320000 (T = 1000)


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
    a = dict(wave=P1, grad=P1, B=2, S=320000, window=P1, twiddle=P1, fb_start=P1, fb_len=P1, fb_w=P1, fb_stride=16, n_mels=128,
             bin_band=P1, bin_w=P1, work=P1, nwork=NWORK, dwave=P1)
    a.update(kw)
    return lib.maest_augment_mel_bwd(a["wave"], a["grad"], a["B"], a["S"], a["window"], a["twiddle"], a["fb_start"], a["fb_len"],
                                     a["fb_w"], a["fb_stride"], a["n_mels"], a["bin_band"], a["bin_w"], -0.97, 1.0, 1e-5, 5.0,
                                     a["work"], a["nwork"], a["dwave"], None)


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
    (dict(S=513, nwork=2 * 2 * 1024), b"bad shape"),
    (dict(n_mels=0), b"bad filterbank"),
    (dict(n_mels=129), b"bad filterbank"),
    (dict(fb_stride=0), b"bad filterbank"),
    (dict(nwork=NWORK - 1), b"workspace"),
])
def test_augment_mel_bwd_rejects(lib, kw, msg):
    assert _bwd(lib, **kw) == 1
    err = lib.maest_last_error()
    assert msg in err and b"maest_augment_mel_bwd" in err, err


def test_augment_mel_bwd_signature_follows_the_forward():
    """The new entry sits right behind maest_augment_mel in the binding table, as in the header, and the ABI version is unchanged."""
    names = list(_lib.SIGNATURES)
    assert names[names.index("maest_augment_mel") + 1] == "maest_augment_mel_bwd"
    assert _lib.ABI_VERSION == 9
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maest_hip.h")).read()
    assert hdr.index("int maest_augment_mel(") < hdr.index("int maest_augment_mel_bwd(") < hdr.index("int maest_scale_f32(")
