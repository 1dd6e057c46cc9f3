"""ctypes binding of libmaest_hip.so (C ABI: include/maest_hip.h).

The product path has NO CPU fallback: if the shared library is missing, or a tensor that is not
on a HIP device reaches a kernel wrapper, an exception is raised.  (``_testing_override`` exists
so that tests/emu can run the same kernel sources under the host SIMT emulator; nothing in the
package calls it.)
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MAEST_HIP_LIB: another build of the same library -- e.g. the fallback form of maest_amd/build.py --leave-out, for running the suite against it)
LIB_PATH = os.environ.get("MAEST_HIP_LIB") or os.path.join(_HERE, "libmaest_hip.so")

F32 = 0
BF16 = 1
F16 = 3     # IEEE half, input of maest_patch_im2col only (and dx of maest_patch_im2col_bwd)
BF16_QS = 4 # bf16 qkv tensor with q columns pre-multiplied by scale * log2(e) (maest_attn_* dtype only)
SPLIT3_A, SPLIT3_B, F32X3_A3 = 5, 6, 7   # the split-bf16 product as one bf16 GEMM of 3 K (include/maest_hip.h)
F32X3 = 2   # fp32 tensors, split-bf16 matrix products (maest_gemm_nt in_dtype / maest_attn_fwd dtype only)
ATTN_PROBS, ATTN_PROBS_MEAN = 0x100, 0x200   # flag bits ORed into the dtype of maest_attn_fwd(_rows): the attention maps (include/maest_hip.h)
ATTN_APPLY = 0x400   # flag bit ORed into the dtype of maest_attn_bwd(_rows): weighted attention pooling (include/maest_hip.h)
ATTN_APPLY_GRAD = 0x800   # ... with MAEST_ATTN_APPLY: the gradient-weighted form, out = dO (include/maest_hip.h)
ATTN_LENS = 0x2000   # flag bit ORed into the dtype of maest_attn_fwd(_rows): `lse` carries int32 [B] token counts per clip (include/maest_hip.h)
ATTN_APPLY_HEADS = 0x1000   # ... with MAEST_ATTN_APPLY (and ..._GRAD): the heads kept apart, dqkv = fp32 [B, 12, R, N] (include/maest_hip.h)


GATHER_POOLS = 0x100   # flag bit ORed into the dtype of maest_gather_head_rows: the grid pools of the hidden states (include/maest_hip.h)
IM2COL_CLIP_TOKENS = 0x100   # flag bit ORed into the dtype of maest_patch_im2col(_strided): tok_ft is [B, P, 2], a table per clip (include/maest_hip.h)
TOK_BLANK = 0x40000000       # ... a bit of an entry's f word under that flag: the operand row is written as zeros and x is not read


def gather_pools_t(t: int) -> int:
    """MAEST_GATHER_POOLS_T(t): the number of kept time patches, Tk = 1 .. 32767, as bits of the dtype argument."""
    return t << 16


def attn_apply_rows(r: int) -> int:
    """MAEST_ATTN_APPLY_ROWS(r): the number of weight rows, R = 1 .. 8, as bits of the dtype argument."""
    return (r - 1) << 16


EPI_NONE, EPI_GELU, EPI_RESIDUAL, EPI_MUL, EPI_ATOMIC = 0, 1, 2, 3, 4

_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float
_U = ctypes.c_uint32

# name -> argtypes, in the order of include/maest_hip.h
SIGNATURES = {
    "maest_gemm_nt": [_P, _L, _P, _L, _I, _P, _L, _I, _I, _I, _I, _P, _I, _P, _P, _L, _I, _P],
    "maest_gemm_nt_rowdot": [_P, _L, _P, _L, _I, _P, _L, _I, _I, _I, _I, _P, _P, _L, _P, _I, _P],
    "maest_gemm_tn": [_P, _L, _P, _L, _I, _P, _L, _I, _I, _I, _P, _I, _P],
    "maest_gemm_tn_workspace_bytes": [_I, _I, _I, _I, _I, _P],
    "maest_gemm_tn_ws": [_P, _L, _P, _L, _I, _P, _L, _I, _I, _I, _P, _I, _P, _L, _P],
    "maest_transpose": [_P, _L, _P, _L, _I, _I, _I, _P],
    "maest_cast_weights": [_P, _P, _P, _I, _I, _I, _P],
    "maest_cast_weights_multi": [_I, _P, _P, _P, _P, _P, _P, _F, _I, _P],
    "maest_layernorm_fwd": [_P, _L, _P, _P, _P, _L, _I, _P, _P, _I, _I, _F, _P],
    "maest_add_layernorm_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _P],
    "maest_layernorm_bwd": [_P, _L, _I, _P, _L, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P],
    "maest_attn_fwd": [_P, _P, _P, _I, _I, _I, _F, _P],
    "maest_attn_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P],
    "maest_attn_fwd_rows": [_P, _P, _P, _I, _I, _I, _F, _I, _P],
    "maest_attn_bwd_rows": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P],
    "maest_layernorm_bwd_headres": [_P, _L, _I, _P, _L, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P],
    "maest_gather_head_rows": [_P, _I, _I, _I, _I, _P, _P],
    "maest_scatter_head_rows": [_P, _I, _I, _I, _I, _I, _P, _P],
    "maest_patch_im2col": [_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P],
    "maest_patch_im2col_strided": [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P],
    "maest_patch_im2col_bwd": [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _L, _P, _I, _P],
    "maest_token_assemble": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P],
    "maest_token_assemble_bwd": [_P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P],
    "maest_head_pool_fwd": [_P, _I, _I, _P, _P, _F, _P, _P, _P, _P, _P, _P],
    "maest_head_pool_bwd": [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "maest_embed_pool": [_P, _I, _I, _P, _P],
    "maest_embed_pool_bwd": [_P, _I, _I, _P, _P, _I, _P],
    "maest_bce_logits": [_P, _P, _P, _P, _I, _I, _F, _P, _P, _P],
    "maest_sigmoid_mean": [_P, _I, _I, _P, _P],
    "maest_colsum": [_P, _L, _I, _I, _I, _P, _P],
    "maest_spec_mask": [_P, _I, _I, _I, _P, _I, _P, _I, _P],
    "maest_swa_update_multi": [_I, _P, _P, _P, _F, _P],
    "maest_affine_f32": [_P, _L, _F, _F, _P],
    "maest_augment_mel": [_P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _F, _F, _F, _F, _F, _P, _P],
    "maest_augment_mel_bwd": [_P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _F, _F, _F, _F, _P, _L, _P, _P],
    "maest_melfile_assemble": [_P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P],
    "maest_logmel": [_P, _I, _I, _P, _P, _P, _P, _P, _I, _F, _F, _F, _P, _P],
    "maest_logmel_bwd": [_P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _F, _F, _F, _P, _L, _P, _P],
    "maest_logmel_rows_f16": [_P, _L, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _F, _P, _L, _P],
    "maest_resample": [_P, _L, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _L, _P],
    "maest_scale_f32": [_P, _L, _F, _P],
    "maest_scale_dev_f32": [_P, _L, _P, _P],
    "maest_cast_rows": [_P, _L, _P, _L, _I, _I, _I, _P],
    "maest_rng_advance": [_P, _P, _P],
    "maest_dropout": [_P, _P, _I, _I, _I, _I, _I, _U, _F, _I, _P, _P],
    "maest_drop_add_layernorm_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _F, _I, _U, _F, _I, _U, _F, _P, _P],
    "maest_drop_add": [_P, _P, _I, _P, _I, _I, _I, _I, _I, _U, _F, _I, _U, _F, _P, _P],
    "maest_drop_cast": [_P, _P, _I, _I, _I, _I, _I, _I, _U, _F, _I, _U, _F, _P, _P],
    "maest_set_option": [_I, _I, _I],
    "maest_get_option": [_I, _P],
    "maest_set_option_thread": [_I, _I, _I],
    "maest_kernel_forms": [_P],
}
# name -> positions (in SIGNATURES[name]) of the DEVICE pointer arguments the entry point may write: the ones include/maest_hip.h does not
# declare const (for the two entries that take host arrays of device pointers: the arrays whose elements point at written memory).
# Every other device pointer is only read.  tests/test_guard_cpu.py checks the table against the header; tests/guard.py relies on it.
WRITTEN = {
    "maest_gemm_nt": (5, 14), "maest_gemm_nt_rowdot": (5, 14), "maest_gemm_tn": (5, 10), "maest_gemm_tn_ws": (5, 10, 12),
    "maest_transpose": (2,), "maest_cast_weights": (1, 2), "maest_cast_weights_multi": (2, 3),
    "maest_layernorm_fwd": (4, 7, 8), "maest_add_layernorm_fwd": (3, 6, 8, 9), "maest_layernorm_bwd": (9, 10, 12, 13),
    "maest_attn_fwd": (1, 2), "maest_attn_bwd": (4, 5), "maest_attn_fwd_rows": (1, 2), "maest_attn_bwd_rows": (4, 5),
    "maest_layernorm_bwd_headres": (9, 10, 12, 13), "maest_gather_head_rows": (5,), "maest_scatter_head_rows": (6,),
    "maest_patch_im2col": (13,), "maest_patch_im2col_strided": (15,), "maest_patch_im2col_bwd": (15, 17),
    "maest_token_assemble": (12,), "maest_token_assemble_bwd": (7, 9, 10, 11, 12, 13),
    "maest_head_pool_fwd": (6, 7, 8, 9, 10), "maest_head_pool_bwd": (9, 10, 11), "maest_embed_pool": (3,), "maest_embed_pool_bwd": (3, 4),
    "maest_bce_logits": (7, 8), "maest_sigmoid_mean": (3,), "maest_colsum": (5,), "maest_spec_mask": (0,),
    "maest_swa_update_multi": (1,), "maest_affine_f32": (0,), "maest_augment_mel": (15,), "maest_augment_mel_bwd": (17, 19),
    "maest_melfile_assemble": (9,), "maest_logmel": (12,), "maest_logmel_bwd": (15, 17), "maest_logmel_rows_f16": (13,),
    "maest_resample": (12,), "maest_scale_f32": (0,), "maest_scale_dev_f32": (0,), "maest_cast_rows": (2,),
    "maest_rng_advance": (0, 1), "maest_dropout": (0, 1), "maest_drop_add_layernorm_fwd": (3, 6, 8, 9), "maest_drop_add": (3,),
    "maest_drop_cast": (1,),
}
# name -> {position: kind} of the pointer arguments that are HOST memory: results written through a pointer, and the arrays (of device
# pointers, of sizes) of the two multi-tensor entries.  Every other pointer but the last one (the stream) is a device pointer.
HOST_POINTERS = {
    "maest_gemm_tn_workspace_bytes": {5: "result"}, "maest_get_option": {1: "result"}, "maest_kernel_forms": {0: "result"},
    "maest_cast_weights_multi": {1: "device pointers", 2: "device pointers", 3: "device pointers", 4: "sizes", 5: "sizes", 6: "sizes"},
    "maest_swa_update_multi": {1: "device pointers", 2: "device pointers", 3: "sizes"},
}
FORM_GEMM_NT_OW, FORM_GEMM_TN_OW, FORM_ATTN_FWD_PW = 1, 2, 4

ABI_VERSION = 9
OPTIONS = {"gemm_min_m": 0, "gemm_variant": 1, "gemm_epilogue": 2, "attn_bwd": 3, "ln_bwd_blocks": 4, "gemm_tail": 5, "attn_fwd": 6, "attn_fwd_waves": 7,
           "tn_reduce": 8, "gemm_wgs": 9, "gemm_panel": 10, "deterministic": 11}

_lib = None
_lib_f16 = None
_host_emulation = False  # set only by tests/emu
# The library's second build: the same sources with IEEE half as the 16-bit operand type (csrc/common.h: MAEST_16BIT_F16).  A thread selects it
# for the calls it makes inside `with flavour("f16"):` (maest.py: precision="fp16" evaluation forwards); tensors keep the bf16 dtype TAG -- a
# 16-bit container whose bits the kernels of the selected build interpret.
LIB_PATH_F16 = os.environ.get("MAEST_HIP_LIB_F16") or os.path.join(_HERE, "libmaest_hip_f16.so")


class _Thread(threading.local):
    def __init__(self):     # flavour(): the build this thread's C-ABI calls go to; thread_options(): its overrides, name -> value
        self.flavour, self.options = "bf16", {}


_tls = _Thread()


class _Block:
    """A `with` block that sets values through `put(key, value)`; on exit each key gets back the value `get(key)` gave before it."""

    def __init__(self, get, put, kw):
        self.get, self.put, self.kw = get, put, kw

    def __enter__(self):
        self.prev = {k: self.get(k) for k in self.kw}
        for k, v in self.kw.items():
            self.put(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.prev.items():
            self.put(k, v)


def flavour(name):
    """``with _lib.flavour("f16"): ...`` -- C-ABI calls of this thread go to libmaest_hip_f16.so inside the block."""
    assert name in ("bf16", "f16")
    return _Block(lambda k: getattr(_tls, k), lambda k, v: setattr(_tls, k, v), {"flavour": name})


class MaestHipError(RuntimeError):
    pass


def _bind(lib):
    lib.maest_version.restype = c_int
    lib.maest_version.argtypes = []
    lib.maest_last_error.restype = c_char_p
    lib.maest_last_error.argtypes = []
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = c_int
        fn.argtypes = argtypes
    return lib


def _open(path, missing):
    """Bind the build at `path` and bring its switches to this process's state: the values of set_option, the overrides of the
    binding thread's thread_options blocks."""
    if not os.path.exists(path):
        raise MaestHipError(missing)
    lib = _bind(ctypes.CDLL(path))
    if lib.maest_version() != ABI_VERSION:
        raise MaestHipError(f"{os.path.basename(path)} ABI version mismatch")
    for name, v in _set.items():
        lib.maest_set_option(OPTIONS[name], v or 0, v is None)
    for name, v in _tls.options.items():
        lib.maest_set_option_thread(OPTIONS[name], v or 0, v is None)
    return lib


def load():
    """Load (once) and return the bound library -- the build the calling thread's flavour selects; raise loudly when it is absent."""
    global _lib, _lib_f16
    if _tls.flavour == "f16":
        if _lib_f16 is None:
            if _host_emulation:       # (never the bf16 emulator build in its place: its kernels would read the half bits as bfloat16)
                raise MaestHipError("flavour(\"f16\") under host emulation, but no half-precision emulator build is bound "
                                    "(_testing_override(path, path_f16))")
            _lib_f16 = _open(LIB_PATH_F16, f"{LIB_PATH_F16} not found: precision=\"fp16\" needs the half-precision build of the kernels "
                                           "(`python -c 'import __graft_entry__ as g; g.build()'` builds both).")
        return _lib_f16
    if _lib is None:
        _lib = _open(LIB_PATH, f"{LIB_PATH} not found: the MI355X kernels are not built. Run "
                               "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                               "maest_amd has no CPU fallback.")
    return _lib


def _testing_override(path, path_f16=None):
    """tests/emu only: bind a host-emulation build of the same sources -- and, with `path_f16`, its half-precision flavour, which
    flavour("f16") calls then go to (without it they raise)."""
    global _lib, _lib_f16, _host_emulation
    _lib = _open(path, path)
    _lib_f16 = _open(path_f16, path_f16) if path_f16 else None
    _host_emulation = True
    return _lib


def _testing_restore():
    global _lib, _lib_f16, _host_emulation
    _lib = _lib_f16 = None
    _host_emulation = False


def host_emulation():
    return _host_emulation


def kernel_forms():
    """Bit mask of the owned-register kernels present in this build (include/maest_hip.h: MAEST_FORM_*)."""
    return _out_int("maest_kernel_forms")


def _out_int(name, *args):
    """The int that entry point `name` writes through its last argument."""
    c = c_int(0)
    call(name, *args, ctypes.byref(c))
    return c.value


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise MaestHipError(f"{name} failed (status {rc}): {lib.maest_last_error().decode()}")


# ------------------------------------------------------------------------------------ library switches (include/maest_hip.h)
# Every write goes to every bound build, and _open brings a build bound later (the f16 one at the first fp16 forward) to the same state:
# one value per name holds for both.  get_option, on the hot path (per wgrad GEMM, per backward block), does not cross the C ABI.
_set = {}       # set_option: name -> value, None = the environment default
_values = {}    # name -> process-wide value as the library reports it (maest_get_option), read once after each set_option


def set_option(name: str, value: int | None):
    """maest_set_option on every bound build; a build bound later starts from the values set here (_open replays them, so a missing f16
    build still fails only when an fp16 forward asks for it).  `value` None restores the default (environment, read once at first use)."""
    v = _set[name] = None if value is None else int(value)
    for lib in filter(None, (_lib, _lib_f16)):
        lib.maest_set_option(OPTIONS[name], v or 0, v is None)
    _values.pop(name, None)


def get_option(name: str) -> int:
    """This thread's override of the switch (thread_options), else its process-wide value."""
    v = _tls.options.get(name)
    if v is None and (v := _values.get(name)) is None:      # (no override on this thread: the library reports the process-wide value)
        v = _values[name] = _out_int("maest_get_option", OPTIONS[name])
    return v


def _set_thread(name, value):
    """maest_set_option_thread on every build: `value` None clears this thread's override."""
    _tls.options[name] = v = None if value is None else int(value)      # (first: a build that the read below binds replays it)
    for lib in filter(None, (_lib, _lib_f16)):
        lib.maest_set_option_thread(OPTIONS[name], v or 0, v is None)
    _tls.options[name] = v if v is None else _out_int("maest_get_option", OPTIONS[name])    # the value as the library maps it


def options(**kw):
    """``with ops.options(gemm_min_m=512): ...`` -- set switches for a block, restore the previous values after."""
    return _Block(_set.get, set_option, kw)


def thread_options(**kw):
    """``with ops.thread_options(gemm_wgs=256): ...`` -- override switches for launches made by THIS thread inside the block
    (maest_set_option_thread); other threads see the process-wide values.  Blocks nest: on exit each switch gets back the override it
    had before the block, or none."""
    return _Block(lambda k: _tls.options.get(k), _set_thread, kw)
