"""ctypes binding of libmakani_amd.so -- the C ABI declared in include/makani_amd.h.

The library is the product; there is no fallback.  If it is missing (and cannot be
built because hipcc is absent) importing any compute entry point raises.
"""
import ctypes
import os
import re

# torch must be loaded first: libmakani_amd.so needs libamdhip64.so.7 and has to bind to the SAME HIP
# runtime instance torch brought (its streams and allocations are what the kernels receive); loading
# the extension first would pull a second runtime from /opt/rocm into the process.
import torch  # noqa: F401

from . import build as _build

_LIB = None

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}
_DECL = re.compile(r"([^;{}()]*?)\b(mk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(text, what, decl):
    """ctypes type of one C return / parameter type (an abstract declarator: the parameter's name already removed)."""
    t = " ".join(text.replace("const", " ").split())
    if "*" in t:
        # callers pass data_ptr() integers and None; only the message of mk_last_error comes back as a string
        return ctypes.c_char_p if (what == "return" and t == "char*") else ctypes.c_void_p
    if t not in _SCALARS:
        raise ValueError(f"include/makani_amd.h: unknown {what} type {text.strip()!r} in `{decl}`")
    return _SCALARS[t]


def parse_signatures(header_text):
    """name -> (restype, argtypes) of every `type mk_name(params);` declaration of the header text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for ret, name, params in _DECL.findall(text):
        decl = " ".join(f"{ret} {name}({params});".split())
        params = [] if params.strip() in ("", "void") else params.split(",")
        # a parameter is `type name`; the name is the trailing identifier (the header names every parameter)
        args = [_ctype(re.sub(r"\b[A-Za-z_]\w*\s*$", "", q.strip()), "parameter", decl) for q in params]
        out[name] = (_ctype(ret, "return", decl), args)
    return out


# name -> (restype, argtypes) of every entry point, read off include/makani_amd.h: the header is the one place a signature is written
with open(os.path.join(_build.CSRC, _build.HEADERS[-1])) as _f:
    SIGNATURES = parse_signatures(_f.read())


def lib_path():
    return _build.LIB


def load():
    """Load (building first if the sources are newer) and return the ctypes handle."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB
    override = os.environ.get("MK_LIB_OVERRIDE")        # A/B builds of the kernels (tools only): load this file as it is
    if override:
        path = override
    elif _build.stale():
        # missing, or older than a source / header: rebuild when hipcc is here, never run a stale library silently
        if _build.have_hipcc():
            path = _build.build(verbose=False)
        elif not os.path.exists(path):
            raise RuntimeError(f"makani_amd: {path} is missing and hipcc is not available to build it")
        else:
            raise RuntimeError(f"makani_amd: {path} is older than its sources and hipcc is not available to rebuild it")
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover - environment problem, never silent
        raise RuntimeError(f"makani_amd: cannot load the HIP extension {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().mk_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"makani_amd {what} failed (code {rc}): {msg}")
