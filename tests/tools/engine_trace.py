"""The launch trace of the engine (TEST INFRASTRUCTURE ONLY): what a callable makes the library do, recorded with no library bound and no
device -- the C-ABI calls in order, every non-pointer argument by value, every pointer as (storage, byte offset).

    from tests.tools import engine_trace as ET
    entries = ET.trace(lambda: net(mel))          # CPU tensors, nothing is launched

    python tests/tools/engine_trace.py [--repo PATH] [--forms all|none] [--dump DIR] [CASE ...]

The second form runs the matrix of cases below against the tree at PATH (default: this tree) in a fresh interpreter and prints one line
per case: name, number of calls, digest.  Two trees whose tables agree line for line make the same launches with the same arguments on
the same buffers; where they differ, `diff` of the two --dump directories names the first differing launch.  `--time CASE` prints the
wall time of --iters runs of one case after a warm-up run: with nothing launched, host time alone.

Mechanism (that of tests/guard.py): for the duration of a trace the names `call`, `_p`, `_chk` and `torch` inside maest_amd.ops and
`call` inside maest_amd._lib are replaced, and _lib._host_emulation is set so that CPU tensors pass the device check; everything is put
back in a `finally`.  The recorder answers maest_get_option, maest_set_option_thread and maest_kernel_forms itself: option defaults from
include/maest_hip.h (overridable per trace: `options`), the kernel-forms mask a parameter (all forms or none).

One entry: (entry point, the thread's flavour, the thread's option overrides in force, the arguments).  A pointer argument is None or
(ordinal of its storage in order of first appearance in the trace, byte offset); the pointer tables of maest_cast_weights_multi and
maest_swa_update_multi (_lib.HOST_POINTERS) are expanded element by element.  Every tensor that reaches the layer is kept alive until
the trace ends, so no address is reused inside it, and a pointer that cannot be traced to a tensor raises TraceError.  The trace ends
with the identity and shape of every tensor the callable returned: a statement of launches and of the dataflow between them, which does
not depend on allocation order."""
import argparse
import collections
import ctypes
import hashlib
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ALL_FORMS = 7          # MAEST_FORM_GEMM_NT_OW | MAEST_FORM_GEMM_TN_OW | MAEST_FORM_ATTN_FWD_PW


class TraceError(AssertionError):
    pass


Ptr = collections.namedtuple("Ptr", "storage offset")      # a pointer argument: ordinal of its storage in the trace, byte offset into it


class _Ref(ctypes.c_void_p):
    """What the replaced ops._p hands to the call: the pointer, and the tensor it came from."""


def option_defaults(header):
    """{switch name: default} as include/maest_hip.h states them ("env MAEST_X, default v" beside each MAEST_OPT_X)."""
    text = open(header).read()
    found = {n.lower(): int(v) for n, v in re.findall(r"MAEST_OPT_([A-Z_]+)\s+(?:\d+ /\* |\()env \w+,\s+default (-?\d+)", text)}
    return found


class Recorder:
    """``with Recorder() as r: ...; r.entries`` -- see the module docstring.  forms: the mask maest_kernel_forms reports; options: process-wide
    switch values that differ from the header's defaults."""

    def __init__(self, forms=ALL_FORMS, options=None):
        self.forms, self.options = int(forms), dict(options or {})
        self.entries = []
        self._keep = []           # every tensor seen: no address is reused while the trace runs
        self._known = {}          # data_ptr -> tensor: what a wrapper checked or allocated (for the pointer tables)
        self._ordinal = {}        # storage address -> ordinal, in order of first appearance in a recorded call

    def __enter__(self):
        import torch
        from maest_amd import _lib, ops
        self._torch, self._lib_mod, self._ops = torch, _lib, ops
        self._defaults = option_defaults(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "maest_hip.h"))
        missing = set(_lib.OPTIONS) - set(self._defaults)
        if missing:
            raise TraceError(f"include/maest_hip.h states no default for {sorted(missing)}")
        self._by_index = {v: k for k, v in _lib.OPTIONS.items()}
        self._saved_ops = {n: getattr(ops, n) for n in ("call", "_p", "_chk", "torch")}
        self._saved_lib = (_lib.call, _lib._host_emulation, dict(_lib._values))
        rec = self

        class TorchProxy:      # the `torch` name inside ops: torch, with what the wrappers allocate remembered
            def __getattr__(self, name):
                return getattr(torch, name)

            def empty(self, *a, **kw):
                return rec._remember(torch.empty(*a, **kw))

            def empty_like(self, *a, **kw):
                return rec._remember(torch.empty_like(*a, **kw))

        try:
            _lib._values.clear()      # (process-wide values read from a bound library: not this recorder's table)
            _lib._host_emulation = True
            _lib.call = ops.call = self._call
            ops._p, ops._chk, ops.torch = self._p, self._chk, TorchProxy()
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *a):
        for n, v in self._saved_ops.items():
            setattr(self._ops, n, v)
        _lib = self._lib_mod
        _lib.call, _lib._host_emulation, values = self._saved_lib
        _lib._values.clear()
        _lib._values.update(values)
        self._keep.clear()
        self._known.clear()

    # ---- the replaced names
    def _remember(self, t):
        self._keep.append(t)
        self._known[t.data_ptr()] = t
        return t

    def _chk(self, *ts):
        self._saved_ops["_chk"](*ts)
        for t in ts:
            if t is not None:
                self._remember(t)

    def _p(self, t):
        if t is None:
            return None
        r = _Ref(t.data_ptr())
        r.tensor = t
        self._keep.append(t)
        return r

    def _ident(self, t):
        if t.numel() == 0:
            return ("empty",)
        st = t.untyped_storage()
        base = st.data_ptr()
        if base not in self._ordinal:
            self._ordinal[base] = len(self._ordinal)
            self._keep.append(st)
        return Ptr(self._ordinal[base], t.data_ptr() - base)

    def _option(self, name):
        _lib = self._lib_mod
        v = _lib._tls.options.get(name)
        if v is None and (v := _lib._set.get(name)) is None:
            v = self.options.get(name, self._defaults[name])
        return 0 if (name == "attn_bwd" and v == 2) else int(v)      # (the library maps the removed form 2 to 0 wherever a value enters)

    def note(self, *what):
        """An entry of the callable's own (the stand-in gradient sink reports its calls this way)."""
        self.entries.append(tuple(what))

    def _call(self, name, *args):
        _lib = self._lib_mod
        sig = _lib.SIGNATURES[name]
        if len(args) != len(sig):
            raise TraceError(f"{name}: {len(args)} arguments for a signature of {len(sig)}")
        if name == "maest_get_option":
            args[1]._obj.value = self._option(self._by_index[args[0]])
            return
        if name == "maest_kernel_forms":
            args[0]._obj.value = self.forms
            return
        if name == "maest_set_option_thread":       # (_lib keeps the override in _tls.options, which _option reads)
            return
        host = _lib.HOST_POINTERS.get(name, {})
        ptrs = [i for i, ty in enumerate(sig) if ty is ctypes.c_void_p]
        stream = ptrs[-1] if ptrs and ptrs[-1] not in host else None
        out = []
        for i, (a, ty) in enumerate(zip(args, sig)):
            if ty is not ctypes.c_void_p:
                v = getattr(a, "value", a)
                out.append(float(v) if ty is ctypes.c_float else int(v))
            elif i in host:
                kind = host[i]
                if kind == "result":
                    a._obj.value = 0
                    out.append("result")
                    continue
                n = int(args[0])
                if a is None or not a.value:
                    out.append(None)
                elif kind == "sizes":
                    width = ctypes.c_int64 if name == "maest_swa_update_multi" else ctypes.c_int
                    out.append(tuple((width * n).from_address(a.value)))
                else:
                    arr = (ctypes.c_void_p * n).from_address(a.value)
                    out.append(tuple(self._table_entry(name, i, k, arr[k]) for k in range(n)))
            elif i == stream:
                if a is not None:
                    raise TraceError(f"{name}: a stream handle under the recorder")
                out.append(None)
            elif a is None:
                out.append(None)
            elif isinstance(a, _Ref):
                out.append(self._ident(a.tensor))
            else:
                raise TraceError(f"{name}: argument {i}: a pointer reached the call without passing through ops._p")
        opts = tuple(sorted((k, v) for k, v in _lib._tls.options.items() if v is not None))
        self.entries.append((name, _lib._tls.flavour, opts, tuple(out)))

    def _table_entry(self, name, i, k, addr):
        if not addr:
            return None
        t = self._known.get(addr)
        if t is None:
            raise TraceError(f"{name}: argument {i}[{k}]: a device pointer the recorder cannot trace to a tensor")
        return self._ident(t)

    # ---- what the callable returned
    def returned(self, obj, path="ret", depth=0):
        torch = self._torch
        if isinstance(obj, torch.Tensor):
            st = obj.untyped_storage()
            ident = "untraced" if obj.numel() == 0 or st.data_ptr() not in self._ordinal else self._ident(obj)
            self.entries.append(("<returned>", path, ident, tuple(obj.shape), str(obj.dtype)))
        elif isinstance(obj, (list, tuple)):
            for k, v in enumerate(obj):
                self.returned(v, f"{path}[{k}]", depth + 1)
        elif isinstance(obj, dict):
            for k in obj:
                self.returned(obj[k], f"{path}[{k!r}]", depth + 1)
        elif depth < 4 and hasattr(obj, "__dict__") and not isinstance(obj, (torch.nn.Module, type)) and not callable(obj):
            for k in sorted(vars(obj)):
                self.returned(vars(obj)[k], f"{path}.{k}", depth + 1)


def trace(fn, forms=ALL_FORMS, options=None, recorder_arg=False):
    """The entries of `fn()` (fn(recorder) with recorder_arg), closed by what it returned."""
    with Recorder(forms, options) as r:
        r.returned(fn(r) if recorder_arg else fn())
        return list(r.entries)


def calls(entries, name=None):
    """The C-ABI calls of a trace (without the callable's own notes and the returned tensors), optionally of one entry point."""
    return [e for e in entries if e[0].startswith("maest_") and (name is None or e[0] == name)]


def renumbered(entries):
    """The entries with the storage ordinals dealt again in order of first appearance: what is left of a trace after calls were taken out
    of it, comparable with a trace that never made them."""
    seen = {}

    def again(v):
        if isinstance(v, Ptr):
            return Ptr(seen.setdefault(v.storage, len(seen)), v.offset)
        return tuple(again(x) for x in v) if isinstance(v, tuple) else v
    return [again(e) for e in entries]


def _fmt(v):
    if v is None:
        return "-"
    if isinstance(v, Ptr):
        return f"@{v.storage}+{v.offset}"
    if isinstance(v, tuple):
        return "[" + ",".join(_fmt(x) for x in v) + "]"
    return repr(v)


def lines(entries):
    """One line of text per entry; pointers as @ordinal+offset."""
    out = []
    for e in entries:
        if e[0].startswith("maest_"):
            name, flavour, opts, args = e
            out.append(f"{name} {flavour} {{{','.join(f'{k}={v}' for k, v in opts)}}} " + " ".join(_fmt(a) for a in args))
        else:
            out.append(" ".join(_fmt(x) if isinstance(x, tuple) or x is None else str(x) for x in e))
    return out


def digest(entries):
    return hashlib.sha256("\n".join(lines(entries)).encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------ the matrix
ARCH = "passt_s_swa_p16_128_ap476"
S, L = 128, 400      # input_t: 9 x 12 patches, N = 110 (one attention tile, M = 220 < 512) / 9 x 39 patches, N = 353 (M = 706, no head-row backward)
BATCH = 2
PRECISIONS = ("fp32", "bf16x3", "bf16", "fp16", "auto")


def build(t=S, precision="bf16", train=False, qkv_bias=True, **kw):
    """A fresh model (its operand-copy caches cold) in train() or eval().  The weights' values play no part in a trace."""
    import torch
    from maest_amd import get_maest
    from maest_amd.maest import MAEST
    torch.manual_seed(0)
    if qkv_bias:
        net = get_maest(ARCH, pretrained=False, input_t=t, precision=precision, **kw)
    else:       # (the factory has no such argument: the constructor, with the factory's geometry)
        net = MAEST(img_size=(96, t), stride=(10, 10), num_classes=400, qkv_bias=False, precision=precision, **kw)
    return net.train(train)


def mel(t=S, seed=1):
    import torch
    return torch.randn((BATCH, 1, 96, t), generator=torch.Generator().manual_seed(seed))


def evaluate(net, x, **kw):
    import torch

    def run():
        torch.manual_seed(7)
        with torch.no_grad():
            return net(x, **kw)
    return run


def train_step(net, x, loss=lambda o: o[0].sum(), **kw):
    import torch

    def run():
        torch.manual_seed(7)
        outs = net(x, **kw)
        loss(outs).backward()
        return outs, x.grad
    return run


class Sink:
    """Stand-in gradient sink: views of one flat buffer, two buckets, its own calls appended to the trace."""
    collective = True

    def __init__(self, net, rec):
        import torch
        self.rec = rec
        names = [n for n, p in net.named_parameters()]
        off, self.views = 0, {}
        sizes = {n: p.numel() for n, p in net.named_parameters()}
        self.flat = torch.zeros(sum((k + 3) & ~3 for k in sizes.values()))
        for n, p in net.named_parameters():
            self.views[n] = self.flat[off:off + p.numel()].view(p.shape)
            off += (p.numel() + 3) & ~3
        self.bucket_of = {n: int(n.startswith("blocks.")) for n in names}
        self.pending = [sum(1 for b in self.bucket_of.values() if b == k) for k in (0, 1)]

    def grad_buffer(self, name):
        return self.views.get(name)

    def note_grad(self, name):
        b = self.bucket_of[name]
        self.pending[b] -= 1
        self.rec.note("sink.note_grad", name)
        return b if self.pending[b] == 0 else None

    def reduce_bucket(self, b, dedicated_stream=False):
        self.rec.note("sink.reduce_bucket", b, dedicated_stream)


def _engine_switch(name, value, precision="bf16", train=True, t=S):
    def make():
        net = build(t, precision, train)
        setattr(net._engine, name, value)
        return (train_step if train else evaluate)(net, mel(t))
    return make


def _regularised(precision, **rates):
    def make():
        net = build(S, precision, True, **rates)
        net.set_regulariser_seed(5)
        return train_step(net, mel())
    return make


def _hooks(precision):
    def make():
        import torch
        net = build(S, precision, True)
        stripes = (torch.tensor([[[3, 4]], [[20, 2]]], dtype=torch.int32), torch.tensor([[[5, 6]], [[40, 3]]], dtype=torch.int32))
        return train_step(net, mel(), _mixup=(torch.tensor([1, 0]), torch.tensor([0.3, 0.6])), _specmask=stripes,
                          _patchout=(0, [0, 1, 2, 4, 5, 7, 8, 9, 11]))
    return make


def _frozen_blocks(precision):
    def make():
        net = build(S, precision, True)
        for blk in list(net.blocks)[:6]:
            for p in blk.parameters():
                p.requires_grad_(False)
        return train_step(net, mel())
    return make


def _input_grad(precision):
    def make():
        net = build(S, precision, False)
        for p in net.parameters():
            p.requires_grad_(False)
        return train_step(net, mel().requires_grad_(True))
    return make


def _with_sink(precision):
    def make():
        net = build(S, precision, True)

        def run(rec):
            net._grad_sink = Sink(net, rec)
            return train_step(net, mel())()
        run.recorder_arg = True
        return run
    return make


def _method(name, *args, precision="bf16x3", t=S, **kw):
    def make():
        import torch
        net, x = build(t, precision, False), mel(t)

        def run():
            torch.manual_seed(7)
            return getattr(net, name)(x, *[a() if callable(a) else a for a in args], **kw)
        return run
    return make


def _keep(counts, blank=False):
    """bool [B, 108] masks: clip b keeps its first counts[b] tokens (blank: the first two of them blanked)."""
    def make():
        import torch
        m = torch.zeros((BATCH, 108), dtype=torch.bool)
        for b, c in enumerate(counts):
            m[b, :2 if blank else c] = True
        return m
    return make


def _scores():
    import torch
    return torch.rand((BATCH, 108), generator=torch.Generator().manual_seed(3)) + 0.1


def matrix():
    """[(case name, make, recorder arguments)]: make() builds the model and the input and returns the callable to trace."""
    M = []

    def add(name, make, **rec):
        M.append((name, make, rec))

    for tn, t in (("S", S), ("L", L)):
        for p in PRECISIONS:
            add(f"{p} eval at {tn}", lambda p=p, t=t: evaluate(build(t, p, False), mel(t)))
            add(f"{p} train at {tn}", lambda p=p, t=t: train_step(build(t, p, True), mel(t)))
    for p in ("bf16", "fp32"):
        both, dist, feat = (lambda o: o[0].sum() + o[1].sum()), (lambda o: o[1].sum()), (lambda o: o[2].sum())
        for ln, loss in (("both logits", both), ("logits_dist", dist), ("features", feat)):
            add(f"{p} train separated, loss on {ln}",
                lambda p=p, loss=loss: train_step(build(S, p, True, distilled_type="separated"), mel(), loss))
        add(f"{p} train drop_rate", _regularised(p, drop_rate=0.1))
        add(f"{p} train drop_path_rate", _regularised(p, drop_path_rate=0.2))
        add(f"{p} train drop_rate and drop_path_rate", _regularised(p, drop_rate=0.1, drop_path_rate=0.2))
        for k in (0, 1, 2):
            add(f"{p} train split_add={k}", _engine_switch("split_add", k, p))
        for sw in ("head_tail", "fold_delta", "fold_qscale"):
            add(f"{p} train {sw}=False", _engine_switch(sw, False, p))
        add(f"{p} train qkv_bias=False", lambda p=p: train_step(build(S, p, True, qkv_bias=False), mel()))
        add(f"{p} train u_patchout=20 s_patchout_t=2", lambda p=p: train_step(build(S, p, True, u_patchout=20, s_patchout_t=2), mel()))
        add(f"{p} train private hooks", _hooks(p))
        add(f"{p} train blocks 0-5 frozen", _frozen_blocks(p))
        add(f"{p} eval() input gradient, parameters frozen", _input_grad(p))
        for blk in (5, 11):
            for rsa in (False, True):
                add(f"{p} train transformer_block={blk}" + (" return_self_attention" if rsa else ""),
                    lambda p=p, blk=blk, rsa=rsa: train_step(build(S, p, True), mel(), lambda o: o[1].sum(), transformer_block=blk,
                                                             return_self_attention=rsa))
        add(f"{p} train option attn_bwd=1", lambda p=p: train_step(build(S, p, True), mel()), options={"attn_bwd": 1})
        add(f"{p} train gradient sink", _with_sink(p))
    for k in (0, 1, 2):
        add(f"bf16 eval split_add_eval={k}", _engine_switch("split_add_eval", k, "bf16", False))
    add("bf16x3 eval x3_fast=False", _engine_switch("x3_fast", False, "bf16x3", False))
    add("bf16x3 eval at L, kernel forms none", lambda: evaluate(build(L, "bf16x3", False), mel(L)), forms=0)
    # (beyond the issue's list: with the header's gemm_min_m = 8192 no shape of the matrix reaches ops.gemm_split3_out_fast's threshold,
    # so the fc1 epilogue that writes split rows -- and fc2 on them -- is traced with the switch at 512, where M = 706 qualifies)
    add("bf16x3 eval at L, option gemm_min_m=512", lambda: evaluate(build(L, "bf16x3", False), mel(L)), options={"gemm_min_m": 512})
    add("bf16x3 eval at L, option gemm_min_m=512, kernel forms none", lambda: evaluate(build(L, "bf16x3", False), mel(L)),
        options={"gemm_min_m": 512}, forms=0)
    for rsa in (False, True):
        add("bf16x3 eval transformer_block=5" + (" return_self_attention" if rsa else ""),
            lambda rsa=rsa: evaluate(build(S, "bf16x3", False), mel(), transformer_block=5, return_self_attention=rsa))
    for q in ("head", "all"):
        for h in ("all", "mean"):
            add(f"attention_maps queries={q} heads={h}", _method("attention_maps", blocks=(3, 11), queries=q, heads=h))
    add("attention_rollout", _method("attention_rollout"))
    add("attention_relevance", _method("attention_relevance", 7))
    add("attention_heads", _method("attention_heads"))
    add("attention_heads target", _method("attention_heads", 7))
    for pool in ("embedding", "time", "freq", "states"):
        add(f"hidden_states pool={pool}", _method("hidden_states", blocks=(2, 7), pool=pool))
        add(f"hidden_states pool={pool}, last block", _method("hidden_states", blocks=(2, 11), pool=pool))
    add("forward_tokens", _method("forward_tokens", _keep((60, 60))))
    add("forward_tokens blank", _method("forward_tokens", _keep((60, 60)), _keep((60, 60), blank=True)))
    add("forward_tokens ragged, unequal counts", _method("forward_tokens", _keep((60, 41)), ragged=True))
    add("forward_tokens ragged, equal counts", _method("forward_tokens", _keep((60, 60)), ragged=True))
    add("forward_lengths", lambda: (lambda net, x: lambda: net.forward_lengths(x[:, 0], [128, 77]))(build(S, "bf16x3", False), mel()))
    for mode in ("drop", "blank"):
        add(f"perturbation_curve mode={mode}", _method("perturbation_curve", _scores, 7, fractions=(0.0, 0.5), mode=mode))
    add("perturbation_curve by=mass", _method("perturbation_curve", _scores, 7, fractions=(0.0, 0.5), by="mass"))
    return M


def run_case(make, rec):
    run = make()
    return trace(run, recorder_arg=getattr(run, "recorder_arg", False), **rec)


def _child(a):
    sys.path.insert(0, os.path.abspath(a.repo))
    import torch
    torch.set_num_threads(1)
    rows = [(n, mk, rec) for n, mk, rec in matrix() if not a.cases or n in a.cases]
    unknown = set(a.cases) - {n for n, _, _ in rows}
    if unknown:
        raise SystemExit(f"no such case: {sorted(unknown)}")
    forms = {"all": ALL_FORMS, "none": 0}[a.forms]
    if a.time:
        (name, make, rec), = rows
        rec.setdefault("forms", forms)
        run = make()
        one = lambda: trace(run, recorder_arg=getattr(run, "recorder_arg", False), **rec)
        one()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            one()
        print(f"{name}\t{a.iters} iterations\t{time.perf_counter() - t0:.4f} s", flush=True)
        return
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    for name, make, rec in rows:
        rec.setdefault("forms", forms)
        entries = run_case(make, rec)
        print(f"{name}\t{len(calls(entries))} calls\t{digest(entries)}", flush=True)
        if a.dump:
            with open(os.path.join(a.dump, re.sub(r"[^A-Za-z0-9_.=-]+", "_", name) + ".txt"), "w") as f:
                f.write("\n".join(lines(entries)) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repo", default=ROOT, help="the tree whose maest_amd is traced (default: this one)")
    ap.add_argument("--forms", choices=("all", "none"), default="all", help="what maest_kernel_forms reports where a case does not say")
    ap.add_argument("--dump", metavar="DIR", help="write the full trace of every case to DIR/<case>.txt")
    ap.add_argument("--time", action="store_true", help="time one case: --iters traced runs after one warm-up")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("cases", nargs="*", help="case names (default: the whole matrix)")
    a = ap.parse_args(argv)
    if a.time and len(a.cases) != 1:
        ap.error("--time takes exactly one case")
    if a.child:
        return _child(a)
    # a fresh interpreter, so that `maest_amd` is the tree at --repo whatever this process has imported
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (sys.argv[1:] if argv is None else list(argv))
    env = dict(os.environ, PYTHONPATH=os.path.abspath(a.repo))
    return subprocess.run(cmd, env=env, cwd=os.path.abspath(a.repo)).returncode


if __name__ == "__main__":
    sys.exit(main())
