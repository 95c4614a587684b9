"""ctypes binding of the C-ABI library ``lib/libsmsut_hip.so``, read from its header ``include/smsut_hip.h``.

The header is the one place an entry point is written down: the compiler holds every definition to it (csrc/common.h includes
it) and this module parses it at import into the ctypes prototypes and the per-argument checks of ``call``.

PyTorch is used here only for device memory and the current HIP stream.  There is NO fallback:
if the library is missing or a tensor is not on a HIP device the call raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsmsut_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "smsut_hip.h")


class SmsutHipError(RuntimeError):
    pass


# signature codes: p = device pointer, i = int32, l = int64, f = float, d = double, s = stream (the trailing void* stream)
_CT = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "f": ctypes.c_float, "d": ctypes.c_double,
       "s": ctypes.c_void_p}
_SCALAR = {"int": "i", "int64_t": "l", "float": "f", "double": "d"}
# What a tensor argument may be, by the pointee type its parameter declares.  `void` takes any dtype (the header declares fp16 and
# byte workspaces so); every other pointee (a `T* const*` host array of pointers, say) takes no tensor at all.
_ANY = "any dtype"
_POINTEE = {"float": torch.float32, "double": torch.float64, "uint8_t": torch.uint8, "int": torch.int32,
            "int64_t": torch.int64, "void": _ANY}


def _parse_header(path: str):
    """{entry point: (return type, [(parameter name, kind letter, declared type)])} of every ``int|int64_t smsut_*(...);``"""
    if not os.path.exists(path):
        raise SmsutHipError(f"C-ABI header not found: {path} is missing; the binding of {LIB_PATH} is read from it.")
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(int|int64_t)\s+(smsut_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        params = [" ".join(a.split()) for a in m.group(3).split(",")]
        params = [a for a in params if a and a != "void"]
        out = []
        for k, a in enumerate(params):
            ctype, pname = re.fullmatch(r"(.*?)(\w+)", a).groups()
            ctype = ctype.strip()
            if "*" in ctype:
                kind = "s" if (ctype, pname, k) == ("void*", "stream", len(params) - 1) else "p"
            elif ctype in _SCALAR:
                kind = _SCALAR[ctype]
            else:
                raise SmsutHipError(f"{path}: unparsed parameter {a!r} of {m.group(2)}")
            out.append((pname, kind, ctype))
        decls[m.group(2)] = (m.group(1), out)
    return decls


_DECLS = _parse_header(HEADER_PATH)
SIGNATURES: Dict[str, str] = {name: "".join(k for _, k, _ in ps) for name, (_, ps) in _DECLS.items()}
_RET_I64 = {name for name, (ret, _) in _DECLS.items() if ret == "int64_t"}
# An entry point that takes a stream enqueues work and returns a status; one that takes none returns a count, a size or a form id.
# The two measurement entry points below take a stream but return a count (their split slabs).
_NO_STATUS = {name for name, sig in SIGNATURES.items() if not sig.endswith("s")} | {
    "smsut_conv2d_wgrad_mfma_slabs", "smsut_conv2d_wgrad_pair_slabs"}


def _accepts(kind: str, ctype: str):
    """The dtype a tensor in this slot must have: a torch dtype, _ANY, or None = no tensor belongs here."""
    return _POINTEE.get(ctype.replace("const", "").replace(" ", "")[:-1]) if kind == "p" else None


# entry point -> (returns a status, the accepted tensor dtype of each parameter): all that ``call`` looks up per call
_CHECKS = {name: (name not in _NO_STATUS, tuple(_accepts(k, t) for _, k, t in ps)) for name, (_, ps) in _DECLS.items()}

_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """dlopen the C-ABI library and bind every entry point; raises loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmsutHipError(
            f"HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, sig in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.argtypes = [_CT[c] for c in sig]
        fn.restype = ctypes.c_int64 if name in _RET_I64 else ctypes.c_int
    _lib = lib
    return lib


def stream_ptr() -> int:
    if not torch.cuda.is_available():
        raise SmsutHipError("SMSUT HIP ops need an MI355X (no HIP device visible; there is no CPU fallback)")
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise SmsutHipError("SMSUT HIP ops need tensors on a HIP device (no CPU fallback in the product path)")
    return t.data_ptr()


def _bad_tensor(name: str, i: int, t: torch.Tensor) -> SmsutHipError:
    pname, kind, ctype = _DECLS[name][1][i]
    want = _accepts(kind, ctype)
    expected = ("a number" if kind in "ilfd" else "the stream handle" if kind == "s" else
                "a host address" if want is None else f"a {str(want)[6:]} tensor")
    return SmsutHipError(f"{name}: argument {i} (`{ctype} {pname}`) takes {expected}, got a {str(t.dtype)[6:]} tensor")


def call(name: str, *args):
    """Invoke an entry point; tensors are passed as device pointers, the stream is appended by the caller.  Each tensor is first
    held against the parameter the header declares for its position: a pointer, and of the tensor's dtype unless `void*`."""
    lib = load()
    status, accepts = _CHECKS[name]
    conv = list(args)
    declared = len(conv) == len(accepts)        # (a wrong count is ctypes' to report)
    for i, a in enumerate(conv):
        if isinstance(a, torch.Tensor):
            if declared and accepts[i] is not a.dtype and accepts[i] is not _ANY:
                raise _bad_tensor(name, i, a)
            conv[i] = ptr(a)
    rc = getattr(lib, name)(*conv)
    if not status:
        return rc
    if rc != 0:
        raise SmsutHipError(f"{name} failed with status {rc}" + (" (invalid argument)" if rc == -1 else " (hipError_t)"))
    return rc
