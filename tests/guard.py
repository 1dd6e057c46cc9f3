"""Guarded C-ABI calls (TEST INFRASTRUCTURE ONLY): run every call `maest_amd.ops` makes with each tensor argument moved into an arena

    [ band | the tensor's whole storage, copied | band ]

so that a load or a store outside an operand lands in memory the test owns and is seen.

    with guard.guarded() as g:
        KC.case_gemm(dev, torch.bfloat16, 150, 200, 128)
    assert g.calls["maest_gemm_nt"]

What a guarded call does (include/maest_hip.h, "Conventions": the memory contract):
  * the kernel gets the arena's pointer plus the tensor's offset inside its storage; sizes and leading dimensions stay as they were.
    Arguments that share a storage (x_out aliasing x, column slices such as a_full[:, :M]) share one arena.  The arena interior keeps the
    storage pointer's offset modulo 512 bytes.
  * bands: at least 256 rows of the widest argument's pitch and never under 64 KiB, on each side.  Floating-point tensors, 16-bit
    containers and byte workspaces: the 16-bit pattern 0x7FC1 -- a quiet NaN as bfloat16, as IEEE half and, doubled (0x7FC17FC1), as fp32.
    Integer tensors: the constant 1, so that a stray index read stays inside owned memory instead of steering a wild access; their
    bands are checked for writes only (a stray read of a 1 shows in no result).
  * everything `ops` allocates itself (outputs, delta, work, the split-K workspace) comes back filled with the same pattern (integer
    buffers: with the constant 1, for the same reason as above): regions a kernel promises not to write are recognisable bit for bit
    (`untouched`), and a read before the first write is a NaN in the result instead of whatever the allocator handed out.
  * after the call, on the call's stream and then synchronised: (1) both bands of every arena are bitwise intact, (2) every arena none of
    whose arguments the header declares writable (_lib.WRITTEN) is bitwise unchanged; (3) only then the arenas that hold a written
    argument are copied back into the caller's storages.  A failure raises GuardError naming the entry point, the argument positions and the
    first changed byte relative to the storage's start or end.
  * the two entries that take HOST arrays of device pointers are relocated element by element (the tensors are known from the wrapper's
    own checks and allocations); a pointer the layer cannot trace to a tensor raises "unguarded argument".

Mechanism: the names `call`, `_p`, `_chk` and `torch` inside maest_amd.ops are replaced for the duration of the block (ops.py itself is
unchanged and allocates / marshals as ever with the guard off).  Not for use under graph capture; one guarded block at a time."""
import collections
import ctypes

import torch

from maest_amd import _lib, ops

BAND_MIN = 64 * 1024
BAND_ROWS = 256
NAN16 = 0x7FC1                     # bf16 qNaN; IEEE half qNaN; fp32 0x7FC17FC1 qNaN
INT_FILL = 1
_PATTERN_NAN = bytes([0xC1, 0x7F] * 4)                                # 8 bytes of the pattern, little endian
_INT_DTYPES = (torch.int32, torch.int64, torch.int16, torch.int8)


class GuardError(AssertionError):
    pass


def fill_pattern_(t):
    """Fill a freshly allocated tensor with the guard pattern of its dtype (see the module docstring); returns it."""
    if t.numel() == 0:
        return t
    flat = t.view(-1) if t.is_contiguous() else t
    if t.dtype in _INT_DTYPES:
        return t.fill_(INT_FILL)
    if t.dtype == torch.float32:
        flat.view(torch.int32).fill_(0x7FC17FC1)
    elif t.dtype in (torch.bfloat16, torch.float16):
        flat.view(torch.int16).fill_(NAN16)
    elif t.dtype == torch.uint8:
        flat[0::2] = 0xC1
        flat[1::2] = 0x7F
    elif t.dtype == torch.float64:
        flat.view(torch.int64).fill_(0x7FC17FC17FC17FC1)
    else:
        raise GuardError(f"guard: no fill pattern for dtype {t.dtype}")
    return t


def untouched(t):
    """Boolean tensor, True where an element of `t` (float32, a 16-bit container, or an integer tensor) still holds the fill pattern."""
    if t.dtype in _INT_DTYPES:
        return t == INT_FILL
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32) == 0x7FC17FC1
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16) == NAN16
    raise GuardError(f"guard: no fill pattern for dtype {t.dtype}")


def _expected(kind, start, length, device):
    """The bytes [start, start + length) of a buffer filled with pattern `kind` from its (8-byte aligned) beginning."""
    pat = torch.tensor(list(kind), dtype=torch.uint8, device=device)
    phase = start % 8
    return pat.repeat((length + phase + 7) // 8)[phase:phase + length]


def first_changed(got, want):
    """Index of the first byte at which two uint8 tensors differ, or None."""
    diff = got != want
    if not bool(diff.any()):
        return None
    return int(diff.nonzero()[0])


class _Ref(ctypes.c_void_p):
    """What the replaced ops._p hands to the call: the pointer, and the tensor it came from."""


class _TorchProxy:
    """The `torch` name inside ops while a guard is active: torch, with empty / empty_like filled and recorded."""

    def __init__(self, g):
        self._g = g

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **kw):
        return self._g._allocated(torch.empty(*a, **kw))

    def empty_like(self, *a, **kw):
        return self._g._allocated(torch.empty_like(*a, **kw))


class _Arena:
    def __init__(self, storage, members):
        """members: [(argument label, tensor, written)] sharing `storage`."""
        self.members = members
        dev = members[0][1].device
        self.nbytes = n = storage.nbytes()
        self.base = storage.data_ptr()
        self.orig = torch.empty(0, dtype=torch.uint8, device=dev).set_(storage, 0, (n,), (1,))
        pitch = 1
        for _, t, _ in members:
            pitch = max(pitch, (t.stride(-2) if t.dim() >= 2 else 1) * t.element_size())
        band = -(-max(BAND_MIN, BAND_ROWS * pitch) // 512) * 512
        ints = {t.dtype in _INT_DTYPES for _, t, _ in members}
        if len(ints) != 1:
            raise GuardError(f"guard: integer and floating arguments share a storage: {[m[0] for m in members]}")
        self.kind = None
        total = -(-(2 * band + n + 512) // 8) * 8
        self.buf = torch.empty(total, dtype=torch.uint8, device=dev)
        if ints.pop():
            it = members[0][1].dtype
            self.buf.view(it).fill_(INT_FILL)
            self.kind = bytes(self.buf[:8].cpu().tolist())
        else:
            self.buf.view(torch.int16).fill_(NAN16)
            self.kind = _PATTERN_NAN
        p0 = self.buf.data_ptr()
        assert p0 % 8 == 0
        self.off = band + (self.base - (p0 + band)) % 512          # interior start: same offset modulo 512 as the storage
        assert (p0 + self.off - self.base) % 512 == 0 and self.off + n + band <= total
        self.interior = self.buf[self.off:self.off + n]
        self.interior.copy_(self.orig)
        self.written = any(w for _, _, w in members)

    def ptr(self, t):
        return self.buf.data_ptr() + self.off + (t.data_ptr() - self.base)

    def check(self, entry):
        labels = ", ".join(m[0] for m in self.members)
        dev = self.buf.device
        rear0 = self.off + self.nbytes
        i = first_changed(self.buf[rear0:], _expected(self.kind, rear0, self.buf.numel() - rear0, dev))
        if i is not None:
            raise GuardError(f"{entry}: argument {labels}: the band BEHIND the storage was modified, first at byte +{i} past its end "
                             f"(storage of {self.nbytes} bytes)")
        front = self.buf[:self.off]
        diff = front != _expected(self.kind, 0, self.off, dev)
        if bool(diff.any()):
            last = int(diff.nonzero()[-1])
            first = int(diff.nonzero()[0])
            raise GuardError(f"{entry}: argument {labels}: the band IN FRONT of the storage was modified, from byte -{self.off - first} to "
                             f"byte -{self.off - last} before its start")
        if not self.written:
            i = first_changed(self.interior, self.orig)
            if i is not None:
                raise GuardError(f"{entry}: argument {labels} is declared const but was modified, first at byte {i} of its storage")

    def copy_back(self):
        if self.written:
            self.orig.copy_(self.interior)


class guarded:
    """``with guarded() as g:`` -- see the module docstring.  g.calls: Counter of guarded calls per entry point.
    withhold: a predicate on tensors; a tensor it selects is handed to the call as a bare pointer (as code that bypasses the layer
    would) -- the self-test of the "unguarded argument" refusal."""

    _active = None

    def __init__(self, withhold=None):
        self.calls = collections.Counter()
        self.withhold = withhold
        self._known = {}          # data_ptr -> tensor: what the running wrapper checked or allocated (for the pointer-array entries)

    def __enter__(self):
        if guarded._active is not None:
            raise GuardError("guard: guarded() blocks do not nest")
        guarded._active = self
        self._saved = {n: getattr(ops, n) for n in ("call", "_p", "_chk", "torch")}
        ops.call, ops._p, ops._chk, ops.torch = self._call, self._p, self._chk, _TorchProxy(self)
        return self

    def __exit__(self, *a):
        for n, v in self._saved.items():
            setattr(ops, n, v)
        guarded._active = None
        self._known.clear()

    # ---- the replaced names
    def _allocated(self, t):
        fill_pattern_(t)
        self._known[t.data_ptr()] = t
        return t

    def _chk(self, *ts):
        self._saved["_chk"](*ts)
        for t in ts:
            if t is not None:
                self._known[t.data_ptr()] = t

    def _p(self, t):
        if t is None or t.numel() == 0:
            return None
        if self.withhold is not None and self.withhold(t):
            return ctypes.c_void_p(t.data_ptr())
        r = _Ref(t.data_ptr())
        r.tensor = t
        return r

    def _call(self, name, *args):
        sig = _lib.SIGNATURES[name]
        host = _lib.HOST_POINTERS.get(name, {})
        ptrs = [i for i, ty in enumerate(sig) if ty is ctypes.c_void_p]
        if all(i in host for i in ptrs):                     # no device pointer (switches, the workspace query): nothing to guard
            return self._saved["call"](name, *args)
        written = set(_lib.WRITTEN[name])
        members = []                                         # (label, tensor, written)
        slots = []                                           # (argument position, index in a host array or None, tensor)
        keep = []
        args = list(args)
        assert len(args) == len(sig), (name, len(args), len(sig))
        for i in ptrs[:-1]:
            a = args[i]
            if i in host:
                if host[i] != "device pointers" or a is None or not a.value:
                    continue
                n = int(args[0])
                arr = (ctypes.c_void_p * n).from_address(a.value)
                new = (ctypes.c_void_p * n)(*[arr[k] for k in range(n)])
                keep.append(new)
                args[i] = ctypes.cast(new, ctypes.c_void_p)
                for k in range(n):
                    if not arr[k]:
                        continue
                    t = self._known.get(arr[k])
                    if t is None:
                        raise GuardError(f"{name}: unguarded argument {i}[{k}]: a device pointer the guard cannot trace to a tensor")
                    members.append((f"{i}[{k}]", t, i in written))
                    slots.append((new, k, t))
                continue
            if a is None:
                continue
            if not isinstance(a, _Ref):
                if isinstance(a, ctypes.c_void_p) and not a.value:
                    continue
                raise GuardError(f"{name}: unguarded argument {i}: a device pointer reached the call without passing through the guard")
            members.append((str(i), a.tensor, i in written))
            slots.append((i, None, a.tensor))
        dev = members[0][1].device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise GuardError("guard: not for use under graph capture")
        by_storage = collections.OrderedDict()
        stores = {}
        for m in members:
            st = m[1].untyped_storage()
            by_storage.setdefault(st.data_ptr(), []).append(m)
            stores[st.data_ptr()] = st
        arenas = {k: _Arena(stores[k], ms) for k, ms in by_storage.items()}
        for where, k, t in slots:
            p = arenas[t.untyped_storage().data_ptr()].ptr(t)
            if k is None:
                args[where] = ctypes.c_void_p(p)
            else:
                where[k] = p
        try:
            self._saved["call"](name, *args)
        finally:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            self._known.clear()
        for ar in arenas.values():
            ar.check(name)
        for ar in arenas.values():
            ar.copy_back()
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        self.calls[name] += 1


def device_entries():
    """The entry points of _lib.SIGNATURES that take at least one device pointer."""
    out = []
    for name, sig in _lib.SIGNATURES.items():
        ptrs = [i for i, ty in enumerate(sig) if ty is ctypes.c_void_p]
        if ptrs and not all(i in _lib.HOST_POINTERS.get(name, {}) for i in ptrs):
            out.append(name)
    return out


def covering(registry, *entries, limit=None):
    """Decorator of a test: run it inside guarded() and require every one of `entries` to have been called under the guard; `registry` (a
    set of the test module) collects the names, so that a CPU test can see which entry points the module covers without running it.
    limit (seconds; the GPU tests): the test's own time limit -- a watchdog thread that prints every thread's stack and ends the process
    when the test has not returned by then (a hung kernel blocks inside a synchronise, where no Python-level timeout is delivered; after a
    hang nothing more may start on the device, so the run ends there)."""
    import faulthandler
    import functools

    def deco(fn):
        registry.update(entries)

        @functools.wraps(fn)
        def run(*a, **kw):
            if limit:
                faulthandler.dump_traceback_later(limit, exit=True)
            try:
                with guarded() as g:
                    fn(*a, **kw)
            finally:
                if limit:
                    faulthandler.cancel_dump_traceback_later()
            missing = [e for e in entries if not g.calls[e]]
            assert not missing, f"{fn.__name__}: no guarded call of {missing} (guarded: {dict(g.calls)})"
        return run
    return deco
