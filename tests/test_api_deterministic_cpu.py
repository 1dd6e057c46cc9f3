"""CPU: the public contract of the deterministic mode -- MAEST(deterministic=) / get_maest(deterministic=), the library switch
MAEST_OPT_DETERMINISTIC ("deterministic", process-wide and per thread), the workspace sizes maest_gemm_tn_workspace_bytes reports under
it, and the refusal of the split-K NT GEMM.  Host logic only: no device work.  Runs against the gfx950 build when it is present and
against the host-emulator build of the same sources."""
import copy
import ctypes
import inspect
import os
import threading

import pytest
import torch

from maest_amd import _lib, get_maest, ops
from maest_amd.maest import MAEST

BF = torch.bfloat16
TILE = 256 * 256 * 4


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


def _c(lib, name="deterministic"):
    c = ctypes.c_int(-7)
    assert lib.maest_get_option(_lib.OPTIONS[name], ctypes.byref(c)) == 0, lib.maest_last_error()
    return c.value


# ------------------------------------------------------------------------------------------------ constructor contract
def test_argument_is_keyword_only_and_defaults_to_none():
    for fn in (MAEST.__init__, get_maest):
        p = inspect.signature(fn).parameters["deterministic"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert MAEST(depth=2).deterministic is None
    assert MAEST(depth=2, deterministic=True).deterministic is True
    m = get_maest("discogs-maest-10s-pw-129e", pretrained=False, deterministic=False)
    assert m.deterministic is False and m._init_kwargs["deterministic"] is False


@pytest.mark.parametrize("bad", [1, 0, "yes", 1.0])
def test_argument_is_validated_like_the_rates(bad):
    with pytest.raises(ValueError, match="deterministic"):
        MAEST(depth=2, deterministic=bad)
    m = MAEST(depth=2)
    m.deterministic = bad                     # a plain attribute: checked again at use
    with pytest.raises(ValueError, match="deterministic"):
        m.deterministic_mode()


def test_none_follows_torch_and_the_library_switch(lib):
    m = MAEST(depth=2)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert m.deterministic_mode() is None and not m.is_deterministic        # nothing is set: the library switch as it stands (0)
        with ops.options(deterministic=1):
            assert m.deterministic_mode() is None and m.is_deterministic
            m.deterministic = False                                             # False overrides the process-wide switch ...
            assert m.deterministic_mode() == 0 and not m.is_deterministic
        m.deterministic = None
        torch.use_deterministic_algorithms(True)
        assert m.deterministic_mode() == 1 and m.is_deterministic
        m.deterministic = False                                                 # ... and torch's flag
        assert m.deterministic_mode() == 0 and not m.is_deterministic
        torch.use_deterministic_algorithms(False)
        m.deterministic = True
        assert m.deterministic_mode() == 1 and m.is_deterministic
    finally:
        torch.use_deterministic_algorithms(was)


def test_the_pass_sets_a_thread_override_and_removes_it(lib):
    """_Engine.backward wraps the pass in this block: the switch is 1 inside, for this thread only, and back afterwards"""
    on, off, follow = MAEST(depth=2, deterministic=True), MAEST(depth=2, deterministic=False), MAEST(depth=2)
    seen = []
    t = None
    with on._engine._deterministic_form():
        assert _c(lib) == 1 and ops.get_option("deterministic") == 1
        t = threading.Thread(target=lambda: seen.append((_c(lib), ops.get_option("deterministic"))))
        t.start()
        t.join()
        with off._engine._deterministic_form():          # another model's pass nested in this thread: its own value, then ours again
            assert _c(lib) == 0
        assert _c(lib) == 1
    assert seen == [(0, 0)] and _c(lib) == 0
    with ops.options(deterministic=1):
        with follow._engine._deterministic_form():
            assert _c(lib) == 1
        with off._engine._deterministic_form():
            assert _c(lib) == 0


def test_clone_and_deepcopy_carry_it_and_state_dict_is_unchanged():
    plain, det = MAEST(depth=2), MAEST(depth=2, deterministic=True)
    a, b = plain.state_dict(), det.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert [n for n, _ in plain.named_buffers()] == [n for n, _ in det.named_buffers()]
    for twin in (det.clone_weights(), copy.deepcopy(det)):
        assert twin.deterministic is True
    det.deterministic = False                 # changed after construction: travels too
    assert det.clone_weights().deterministic is False and copy.deepcopy(det).deterministic is False


# ------------------------------------------------------------------------------------------------ the switch
def test_option_exists_and_reads_back(lib):
    assert _lib.OPTIONS["deterministic"] == 11 and _lib.ABI_VERSION == 9
    assert _c(lib) == 0                                        # default (MAEST_DETERMINISTIC unset)
    with ops.options(deterministic=1):
        assert _c(lib) == 1 and ops.get_option("deterministic") == 1
    assert _c(lib) == 0


def test_thread_override_does_not_leak(lib):
    seen = []
    with ops.thread_options(deterministic=1):
        assert _c(lib) == 1
        t = threading.Thread(target=lambda: seen.append(_c(lib)))
        t.start()
        t.join()
    assert seen == [0] and _c(lib) == 0


def test_environment_default_is_read():
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from tests.emu import build_emu
    if os.path.exists(_lib.LIB_PATH):
        bind = ""
    elif build_emu.available():
        bind = f"_lib._testing_override({build_emu.build()!r})\n"
    else:
        pytest.skip("no build of the library here")
    code = f"import sys\nsys.path.insert(0, {repo!r})\nfrom maest_amd import _lib, ops\n{bind}print(ops.get_option('deterministic'))"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MAEST_DETERMINISTIC="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "1", r.stderr


# ------------------------------------------------------------------------------------------------ workspace sizes
def test_workspace_sizes(lib):
    wb = ops.gemm_tn_workspace_bytes
    K = 74240
    shapes = {(2304, 768): 9, (768, 768): 28, (3072, 768): 7}                    # qkv / proj / fc1 wgrads: splits of the one-round plan
    off = {mn: wb(BF, *mn, K) for mn in list(shapes) + [(400, 768), (519, 768), (768, 256)]}
    assert all(v == 0 for v in off.values())                                      # default: atomics, no workspace
    with ops.options(tn_reduce=1):
        red = {mn: wb(BF, *mn, K) for mn in off}
    for (M, N), splits in shapes.items():
        assert red[(M, N)] == splits * (M // 256) * (N // 256) * TILE
    with ops.options(deterministic=1):
        for (M, N), splits in shapes.items():
            got = wb(BF, M, N, K)
            # C partials plus one row of column-sum partials per (split, j-tile)
            assert got == red[(M, N)] + splits * (N // 256) * M * 4 and got > red[(M, N)]
            assert wb(torch.float32, M, N, K) > 0 and wb(torch.float32, M, N, K, x3=True) > 0
        # the shapes the 256-tile kernels refuse: gemm_tn_kernel's own workspace form
        for M, N in ((400, 768), (519, 768), (768, 256)):
            assert red[(M, N)] == 0
            tiles = -(-M // 128) * -(-N // 128)
            total = -(-K // 64)
            per = -(-total // min(1024 // tiles, total))
            splits = -(-total // per)
            mp, npad = -(-M // 128) * 128, -(-N // 128) * 128
            assert wb(BF, M, N, K) == splits * (mp * npad + mp) * 4 > 0
        assert wb(BF, 768, 768, K, split_k=5) == 5 * 9 * TILE + 5 * 3 * 768 * 4
        assert wb(BF, 400, 768, 64) == 0                                          # one slice: one split, nothing to combine
    # ... and unchanged with the switch off again
    assert {mn: wb(BF, *mn, K) for mn in off} == off
    with ops.options(tn_reduce=1):
        assert {mn: wb(BF, *mn, K) for mn in off} == red


# ------------------------------------------------------------------------------------------------ the split-K NT GEMM
def test_split_k_nt_gemm_is_refused_under_the_switch(lib):
    P1, P2, P3 = 256, 512, 1024          # non-null "pointers": never dereferenced, the call fails its checks first
    args = (P1, 64, P2, 64, _lib.F32, P3, 64, _lib.F32, 64, 64, 64, None, _lib.EPI_ATOMIC, None, None, 0)
    with ops.thread_options(deterministic=1):
        assert lib.maest_gemm_nt(*args, 2, None) == 1
        msg = lib.maest_last_error()
        assert b"MAEST_OPT_DETERMINISTIC" in msg and b"split_k" in msg, msg
