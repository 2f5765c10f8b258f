"""ctypes binding of libdfe_hip.so (the C ABI declared in include/dfe_hip.h).

The product path has no CPU fallback: if the library is missing or a tensor is not a
contiguous fp32 HIP tensor, the call raises.  PyTorch is used only for device memory and
the current HIP stream."""
from __future__ import annotations

import ctypes
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DFE_HIP_LIB: another build of the same sources (the ablation / experiment variants tools/*_experiment.sh and tools/*ablate*.sh
# put under scratch/abl/), for measurements only
LIB_PATH = os.environ.get("DFE_HIP_LIB") or os.path.join(_HERE, "libdfe_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dfe_hip.h")

_lib = None
_lock = threading.Lock()


class DfeError(RuntimeError):
    pass


# The type language of the header's prototypes.  Every parameter whose type contains ``*`` is a c_void_p (what ptr(), ctypes
# arrays, byref(struct) and None are passed through); anything outside these tables is refused at load time.
_ARG_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
              "unsigned long long": ctypes.c_ulonglong}
_RETURN_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}
_TYPE_WORDS = {"void", "char", "short", "int", "long", "float", "double", "signed", "unsigned", "const"}


def _argtype(symbol, param):
    if "*" in param:
        return ctypes.c_void_p
    m = re.fullmatch(r"(.+) ([A-Za-z_]\w*)", param)            # "type name"; a prototype may also leave the name out
    ctype = _ARG_TYPES.get(m.group(1) if m and m.group(2) not in _TYPE_WORDS else param)
    if ctype is None:
        raise DfeError("%s: cannot bind the parameter '%s' (the binding knows pointers, %s)"
                       % (symbol, param, ", ".join(_ARG_TYPES)))
    return ctype


def header_signatures(path: str = HEADER_PATH):
    """``{symbol: (restype, [argtypes])}`` for every prototype of include/dfe_hip.h, in ctypes types.  The header is the one
    statement of the C ABI: a prototype this cannot read raises DfeError (no symbol is left with ctypes' untyped default)."""
    with open(path) as fh:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", fh.read(), flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\b[^{;]*\{[^}]*\}[^;]*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text).replace("}", " ")   # the struct bodies are gone: the only brace left closes it
    sigs = {}
    for decl in text.split(";"):
        decl = re.sub(r"\s*\*\s*", "* ", " ".join(decl.split())).strip()
        if not decl:
            continue
        m = re.fullmatch(r"(.*?)\b(dfe_\w+) ?\((.*)\)", decl)
        if m is None:
            raise DfeError("%s: cannot read '%s' as a prototype" % (path, decl))
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret not in _RETURN_TYPES:
            raise DfeError("%s: cannot bind the return type '%s' (the binding knows %s)" % (name, ret, ", ".join(_RETURN_TYPES)))
        sigs[name] = (_RETURN_TYPES[ret], [] if params == "void" else [_argtype(name, p.strip()) for p in params.split(",")])
    return sigs


def header_symbols(path: str = HEADER_PATH):
    """Function names declared in include/dfe_hip.h."""
    return sorted(header_signatures(path))


def header_abi_version(path: str = HEADER_PATH) -> int:
    """``DFE_ABI_VERSION`` as include/dfe_hip.h states it: bumped whenever an exported signature changes or disappears, so a
    stale libdfe_hip.so is refused at load time instead of being called with shifted arguments."""
    with open(path) as fh:
        return int(re.search(r"#define\s+DFE_ABI_VERSION\s+(\d+)", fh.read()).group(1))


def get_lib():
    """Load libdfe_hip.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise DfeError(
                    "libdfe_hip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
            lib = ctypes.CDLL(LIB_PATH)
            for name, (restype, argtypes) in header_signatures().items():
                fn = getattr(lib, name)  # AttributeError if the header and the library disagree
                fn.restype, fn.argtypes = restype, argtypes
            if lib.dfe_abi_version() != header_abi_version():
                raise DfeError("libdfe_hip.so ABI version %d != include/dfe_hip.h's DFE_ABI_VERSION %d: a stale build; "
                               "rebuild with __graft_entry__.build()" % (lib.dfe_abi_version(), header_abi_version()))
            _lib = lib
    return _lib


def check(code: int, what: str = ""):
    if code != 0:
        msg = get_lib().dfe_error_string(code)
        raise DfeError("%s failed: %s (code %d)" % (what or "dfe call", msg.decode() if msg else "?", code))


def ptr(t, strided=False):
    """Device pointer of a contiguous fp32 HIP tensor (None -> NULL).  ``strided=True`` skips the contiguity check
    for entry points that take explicit strides."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise DfeError("expected a torch.Tensor, got %r" % type(t))
    if not t.is_cuda:
        raise DfeError("the HIP loss stack only accepts tensors on a HIP device (got %s); there is no CPU "
                       "fallback in the product path" % t.device)
    if t.dtype not in (torch.float32, torch.uint8, torch.int32, torch.int64):
        raise DfeError("unsupported dtype %s" % t.dtype)
    if not strided and not t.is_contiguous():
        raise DfeError("tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def ptr_any(t):
    """Device pointer of a contiguous HIP tensor of any of the dtypes the entry points take (fp32, fp64, int32, int64, uint8)."""
    if t.dtype == torch.float64:
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError("a contiguous fp64 HIP tensor expected")
        return ctypes.c_void_p(t.data_ptr())
    return ptr(t)


def raw_stream():
    """The current HIP stream's handle as an integer.  ``torch.cuda.current_stream()`` builds a Stream object and resolves the
    device index through four Python frames (~9 us under cProfile, ~180 calls per training step: 1.6 ms of the ~17 ms the host
    needs to enqueue a step -- scratch/host_prof.py, round 6: 17.6 -> 14.3 ms at B = 1); the raw accessor is one C call."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def stream_ptr():
    return ctypes.c_void_p(raw_stream())


def f32c(t):
    """Contiguous fp32 view/copy on the same device."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
