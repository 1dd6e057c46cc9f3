"""CPU: the library switches (ops.set_option / get_option / options / thread_options over maest_set_option, maest_get_option,
maest_set_option_thread).  Host logic only: runs against the host-emulator build of the sources and against the gfx950 builds when they
are present."""
import ctypes
import os
import subprocess
import sys
import threading

import pytest
import torch

from maest_amd import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _c(lib, name):
    """What the library itself reports for the calling thread."""
    c = ctypes.c_int(0)
    assert lib.maest_get_option(_lib.OPTIONS[name], ctypes.byref(c)) == 0
    return c.value


def _in_thread(fn):
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    assert out, "the thread raised"
    return out[0]


def test_thread_options_nest(lib):
    base = ops.get_option("gemm_wgs")
    with ops.thread_options(gemm_wgs=7):
        assert ops.get_option("gemm_wgs") == _c(lib, "gemm_wgs") == 7
        with ops.thread_options(gemm_wgs=3, gemm_tail=0):
            assert ops.get_option("gemm_wgs") == _c(lib, "gemm_wgs") == 3
            assert ops.get_option("gemm_tail") == _c(lib, "gemm_tail") == 0
        assert ops.get_option("gemm_wgs") == _c(lib, "gemm_wgs") == 7
        with ops.thread_options(gemm_wgs=3):
            pass
        assert ops.get_option("gemm_wgs") == _c(lib, "gemm_wgs") == 7
    assert ops.get_option("gemm_wgs") == _c(lib, "gemm_wgs") == base


def test_first_query_inside_an_override_block_is_not_cached(lib):
    with ops.options(gemm_panel=-1):          # a new process-wide value: nothing of it is cached yet
        with ops.thread_options(gemm_panel=5):
            assert ops.get_option("gemm_panel") == 5
        assert ops.get_option("gemm_panel") == _c(lib, "gemm_panel") == -1
        assert _in_thread(lambda: (ops.get_option("gemm_panel"), _c(lib, "gemm_panel"))) == (-1, -1)


def test_other_threads_never_see_an_override(lib):
    base = ops.get_option("gemm_wgs")
    seen = lambda: (ops.get_option("gemm_wgs"), _c(lib, "gemm_wgs"))  # noqa: E731
    with ops.thread_options(gemm_wgs=9):
        assert _in_thread(seen) == (base, base)
    assert _in_thread(seen) == (base, base)
    # and the other way round: a block on another thread leaves this one alone
    entered, leave = threading.Event(), threading.Event()

    def other():
        with ops.thread_options(gemm_wgs=11):
            entered.set()
            leave.wait(30)
    t = threading.Thread(target=other)
    t.start()
    try:
        assert entered.wait(30)
        assert seen() == (base, base)
    finally:
        leave.set()
        t.join()
    assert seen() == (base, base)


def test_attn_bwd_2_is_taken_as_0(lib):
    with ops.options(attn_bwd=2):
        assert ops.get_option("attn_bwd") == _c(lib, "attn_bwd") == 0
        assert ops.attn_bwd_rows_supported(torch.bfloat16, 290)
    with ops.thread_options(attn_bwd=2):
        assert ops.get_option("attn_bwd") == _c(lib, "attn_bwd") == 0
        assert ops.attn_bwd_rows_supported(torch.bfloat16, 290)
    with ops.options(attn_bwd=1):
        assert not ops.attn_bwd_rows_supported(torch.bfloat16, 290)


def test_switches_reach_both_builds():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.LIB_PATH_F16)):
        pytest.skip("libmaest_hip.so / libmaest_hip_f16.so not built here (run __graft_entry__.build())")
    lib = _lib.load()
    with _lib.flavour("f16"):
        lib16 = _lib.load()
    base = _c(lib, "gemm_min_m")
    assert _c(lib16, "gemm_min_m") == base
    with ops.options(gemm_min_m=base + 512):
        with _lib.flavour("f16"):
            assert ops.get_option("gemm_min_m") == base + 512
        assert _c(lib, "gemm_min_m") == _c(lib16, "gemm_min_m") == base + 512
        ops.set_option("gemm_min_m", base + 1024)
        with _lib.flavour("f16"):
            assert ops.get_option("gemm_min_m") == base + 1024
        assert _c(lib, "gemm_min_m") == _c(lib16, "gemm_min_m") == base + 1024
    assert _c(lib, "gemm_min_m") == _c(lib16, "gemm_min_m") == base
    # a thread override holds in both builds: a flavour switch inside the block keeps it
    with ops.thread_options(gemm_wgs=5):
        with _lib.flavour("f16"):
            assert ops.get_option("gemm_wgs") == 5
        assert _c(lib, "gemm_wgs") == _c(lib16, "gemm_wgs") == 5
    assert _c(lib16, "gemm_wgs") == _c(lib, "gemm_wgs") == ops.get_option("gemm_wgs")


_CHILD = r"""
import sys
sys.path.insert(0, {repo!r})
from maest_amd import _lib, ops
ops.set_option("gemm_min_m", 768)
if {emu!r}:
    _lib._testing_override({emu!r}, {emu16!r})
with ops.thread_options(gemm_wgs=6):          # (binds the bf16 build here, the f16 one below)
    for f in ["bf16"] + (["f16"] if {f16!r} else []):
        with _lib.flavour(f):
            print(f, *(_lib._out_int("maest_get_option", _lib.OPTIONS[k]) for k in ("gemm_min_m", "gemm_wgs", "attn_bwd")))
"""


def test_a_build_bound_later_starts_from_the_values_set(lib):
    """Each build is bound once per process, so this runs in a fresh interpreter: set_option (and a thread override) before the build is
    bound, then what the build itself reports; MAEST_ATTN_BWD=2 from the environment reads back as 0.  Under emulation the child binds
    both emulator builds, the half one for flavour("f16")."""
    from tests.emu import build_emu
    emu = build_emu.LIB if _lib.host_emulation() else ""
    emu16 = build_emu.build(f16=True) if emu else ""
    f16 = bool(emu) or os.path.exists(_lib.LIB_PATH_F16)
    env = dict(os.environ, MAEST_ATTN_BWD="2")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, emu=emu, emu16=emu16, f16=f16)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    want = ["bf16 768 6 0"] + (["f16 768 6 0"] if f16 else [])
    assert r.stdout.split("\n")[:-1] == want
