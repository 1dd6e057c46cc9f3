"""CPU (`-m "not gpu"`): the guard layer's own checks (tests/guard.py): the table of written arguments against include/maest_hip.h, the
band check on a byte flipped in front of and behind a tensor, the fill pattern, and the walk over the entry points: every one that takes
a device pointer is named by an emulator guard test and by a GPU guard test."""
import os
import re

import pytest
import torch

from maest_amd import _lib
from tests import guard

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maest_hip.h")


def _prototypes():
    """name -> [(type text, parameter name)] of every `int maest_*(...)` declaration of the header."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(maest_\w+)\s*\(([^)]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p and p != "void":
                mm = re.match(r"(.*?)(\w+)$", p)
                params.append((mm.group(1).strip(), mm.group(2)))
        out[m.group(1)] = params
    return out


def test_written_table_matches_the_header():
    """_lib.WRITTEN / _lib.HOST_POINTERS against the declarations: a device pointer is written iff it is not declared const (for the
    arrays of device pointers: iff the pointed-to type is not const); the stream is the last pointer; host pointers are what the table says."""
    protos = _prototypes()
    for name, sig in _lib.SIGNATURES.items():
        params = protos[name]
        assert len(params) == len(sig), name
        host = _lib.HOST_POINTERS.get(name, {})
        ptr_pos = [i for i, (ty, _) in enumerate(params) if "*" in ty]
        assert ptr_pos == [i for i, ty in enumerate(sig) if ty is _lib._P], name
        if not ptr_pos:
            assert name not in _lib.WRITTEN and not host, name
            continue
        if all(i in host for i in ptr_pos):
            assert name not in _lib.WRITTEN, name
            assert all(params[i][1] != "stream" for i in ptr_pos), name
            continue
        assert params[ptr_pos[-1]] == ("void*", "stream"), name
        written = []
        for i in ptr_pos[:-1]:
            ty = params[i][0]
            if i in host:
                assert (host[i] == "device pointers") == (ty.count("*") == 2), (name, i, ty)
                if ty.count("*") == 2 and not ty.startswith("const"):
                    written.append(i)
            else:
                assert ty.count("*") == 1, (name, i, ty)
                if not ty.startswith("const"):
                    written.append(i)
        assert tuple(written) == tuple(_lib.WRITTEN[name]), (name, written, _lib.WRITTEN[name])
    assert set(_lib.WRITTEN) <= set(_lib.SIGNATURES) and set(_lib.HOST_POINTERS) <= set(_lib.SIGNATURES)
    assert set(protos) == set(_lib.SIGNATURES) | {"maest_version"}


def test_every_device_entry_point_is_named_by_an_emulator_and_a_gpu_guard_test():
    from tests import test_emu_guard, test_guard_gpu
    entries = guard.device_entries()
    assert len(entries) == len(_lib.WRITTEN) == 47
    for where, covered in (("tests/test_emu_guard.py", test_emu_guard.COVERED), ("tests/test_guard_gpu.py", test_guard_gpu.COVERED)):
        missing = [e for e in entries if e not in covered]
        assert not missing, f"{where} covers no guarded call of {missing}"
        assert covered <= set(entries), sorted(covered - set(entries))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int32, torch.int64])
def test_fill_pattern_is_a_quiet_nan_in_every_float_format(dtype):
    t = guard.fill_pattern_(torch.empty(37, dtype=dtype))
    if dtype in (torch.int32, torch.int64):
        assert bool((t == 1).all()) and bool(guard.untouched(t).all())
        return
    raw = t.view(torch.uint8)
    assert raw.tolist() == ([0xC1, 0x7F] * raw.numel())[:raw.numel()]
    if dtype != torch.uint8:
        assert bool(torch.isnan(t).all()) and bool(guard.untouched(t).all())
        assert bool(torch.isnan(t.view(torch.uint8)[:36 * t.element_size() // 2 * 2].view(torch.float16)).all())
        t[5] = 1.0
        assert guard.untouched(t).tolist() == [i != 5 for i in range(37)]


@pytest.mark.parametrize("shape,offset", [((5, 7), 0), ((300, 768), 0), ((11,), 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32])
def test_band_check_sees_one_flipped_byte_on_either_side(dtype, shape, offset):
    base = torch.zeros(offset + int(torch.tensor(shape).prod()), dtype=dtype)
    t = base[offset:].view(shape)
    ar = guard._Arena(t.untyped_storage(), [("0", t, False)])
    pitch = shape[-1] * t.element_size() if len(shape) > 1 else t.element_size()
    assert ar.off >= max(64 * 1024, 256 * pitch) and ar.buf.numel() - ar.off - ar.nbytes >= max(64 * 1024, 256 * pitch)
    assert (ar.buf.data_ptr() + ar.off) % 512 == t.untyped_storage().data_ptr() % 512
    assert ar.ptr(t) - (ar.buf.data_ptr() + ar.off) == offset * t.element_size()
    ar.check("self-test")                                   # intact
    for pos, what in ((ar.off + ar.nbytes, r"BEHIND .* byte \+0 "), (ar.buf.numel() - 1, "BEHIND"), (ar.off - 1, r"IN FRONT .* byte -1 "),
                      (0, "IN FRONT")):
        old = int(ar.buf[pos])
        ar.buf[pos] = old ^ 0x10
        with pytest.raises(guard.GuardError, match=what):
            ar.check("self-test")
        ar.buf[pos] = old
    ar.check("self-test")
    ar.interior[ar.nbytes // 2] ^= 1                        # a const argument modified
    with pytest.raises(guard.GuardError, match="declared const"):
        ar.check("self-test")
