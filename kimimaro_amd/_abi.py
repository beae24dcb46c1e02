"""ctypes binding of libkimi_hip.so, derived from include/kimi_hip.h.

The header is the one statement of the C ABI.  This module reads it once at import -- no library, no torch -- and takes from it
the prototypes (``PROTOTYPES``, ``SYMBOLS``; ``lib()`` applies them to the CDLL), the ``KH_*`` constants and ``kh_label_t``
(``LABEL_T``).  The readers are closed: a type or a value form they do not know raises, naming it, instead of defaulting.  They
rely on the header's regular style: one prototype per ``;`` that begins its line with its return type, no function pointers
or macros in signatures (tests/test_abi.py checks that every prototype is consumed).

There is NO CPU fallback: if the library is missing, cannot be loaded, or no gfx950 device is
visible, every compute entry point raises ``HipUnavailableError``.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# KIMI_HIP_LIB: developer knob -- another build of the same sources (e.g. -DKH_SWEEP_PROBE, kimimaro_amd/build.py)
LIB_PATH = os.environ.get("KIMI_HIP_LIB") or os.path.join(HERE, "libkimi_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "kimi_hip.h")


class HipUnavailableError(RuntimeError):
    """libkimi_hip.so (or an MI355X) is not available; the product has no CPU path."""


class KimiHipError(RuntimeError):
    pass


# ---- the header readers: pure functions of the header's text
VALUE_TYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
               "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RETURN_TYPES = {"int": C.c_int, "int64_t": C.c_int64}
MEMBER_TYPES = {"uint32_t": "<u4", "float": "<f4"}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _param_type(func, param):
    m = re.fullmatch(r"(.*?)\w+", param.strip(), re.S)     # everything in front of the parameter's name
    ctype = re.sub(r"\bconst\b|\s", "", m.group(1)) if m else ""
    if ctype.endswith("*"):
        return C.c_char_p if ctype == "char*" else C.c_void_p
    if ctype not in VALUE_TYPES:
        raise TypeError("kimi_hip.h: %s has a parameter '%s' of a type the binding does not know" % (func, param.strip()))
    return VALUE_TYPES[ctype]


def header_prototypes(text):
    """[(name, restype, [argtypes])] of every `type kh_name(args);`, in header order"""
    out = []
    for ret, name, args in re.findall(r"^([\w \t*]+?)\b(kh_\w+)\s*\(([^)]*)\)\s*;", strip_comments(text), re.M):
        if ret.strip() not in RETURN_TYPES:
            raise TypeError("kimi_hip.h: %s returns '%s', a type the binding does not know" % (name, ret.strip()))
        params = [] if args.strip() == "void" else args.split(",")
        out.append((name, RETURN_TYPES[ret.strip()], [_param_type(name, p) for p in params]))
    return out


def header_defines(text):
    """{name: int} of every `#define KH_NAME value`; value is 16, 1u, 0x100 or (-1)"""
    out = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(KH_\w+)\b(.*)$", strip_comments(text), re.M):
        m = re.fullmatch(r"(\d+|0[xX][0-9a-fA-F]+)[uU]?|\((-\d+)\)", value.strip())
        if not m:
            raise ValueError("kimi_hip.h: #define %s has a value the binding cannot read: '%s'" % (name, value.strip()))
        out[name] = int(m.group(1) or m.group(2), 0)
    return out


def header_struct(text, name):
    """[(member, numpy format)] of `typedef struct name { ... } name;`, comma lists expanded"""
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), strip_comments(text), re.S)
    if not m:
        raise ValueError("kimi_hip.h: no typedef struct %s" % name)
    out = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        ctype, _, members = decl.partition(" ")
        members = [n.strip() for n in members.split(",")]
        if ctype not in MEMBER_TYPES or not all(re.fullmatch(r"[A-Za-z_]\w*", n) for n in members):
            raise TypeError("kimi_hip.h: %s has a member '%s' of a kind the binding does not know" % (name, decl))
        out += [(n, MEMBER_TYPES[ctype]) for n in members]
    return out


# ---- the ABI, read once per process
try:
    with open(HEADER_PATH) as _f:
        _header = _f.read()
except OSError as e:
    raise HipUnavailableError("kimimaro_amd: cannot read the C ABI %s (%s); the binding is derived from it." % (HEADER_PATH, e)) from e
PROTOTYPES = header_prototypes(_header)
SYMBOLS = [name for name, _, _ in PROTOTYPES]   # every symbol include/kimi_hip.h declares
_KH = header_defines(_header)
LABEL_T = np.dtype(header_struct(_header, "kh_label_t"))   # 55 x 4 bytes
assert LABEL_T.itemsize == 220
del _header

ENODEVICE = _KH["KH_ENODEVICE"]
# KH_TRACE_* (the flags of kh_trace_paths), KH_PDRF_BASE / _FINISH / _KEEP_OTHERS and KH_HOLES_PROCESSED / _FILLED / _KILLED (the
# label states of kh_host_resolve_holes) under their names without the KH_: TRACE_PROFILE, PDRF_BASE, HOLES_FILLED, ...
globals().update({k[3:]: v for k, v in _KH.items() if k.startswith(("KH_TRACE_", "KH_PDRF_", "KH_HOLES_"))})
SWEEP_LDS_LEVELS = _KH["KH_SWEEP_LDS_LEVELS"]
BRICK = (_KH["KH_BRICK_X"], _KH["KH_BRICK_Y"], _KH["KH_BRICK_Z"])   # the activity bricks of kh_geodesic_relax / kh_feature_relax
GRAPH_LDS_PAIRS = _KH["KH_GRAPH_LDS_PAIRS"]   # kh_voxel_graph searches a longer pair table in global memory
# the two below have no #define in the header (it is device-visible; the library's sources hold their own): literals
SWEEP_MAX_LEVELS = 1 << 22  # labels with more levels than this use the heap emulation only
NO_FEATURE = 0xFFFFFFFF     # the "no seed reaches this voxel" word of kh_geodesic_seed


def np_ptr(a):
    """the address of a numpy array's memory, for the host C functions"""
    return a.ctypes.data_as(C.c_void_p)


def is_pow2_exponent(e):
    """kimimaro/trace.py:343: is_power_of_two(pdrf_exponent) and pdrf_exponent < 2**16 (the repeated-squaring branch).
    The reference's test (trace.py:310-313) evaluates `num & (num - 1)`: an integral FLOAT exponent (16.0, np.float64(4))
    passes its `int(num) != num` line and then raises TypeError there; so does this mirror."""
    try:
        i = int(e)           # (a NaN raises ValueError here, as the reference's `int(num)` does)
    except TypeError:
        return False
    if i != e:
        return False
    if i == 0:               # trace.py:311: `if num != 0 and ...` short-circuits -- 0 and 0.0 take the np.power branch
        return False
    if isinstance(e, (float, np.floating)):
        raise TypeError("unsupported operand type(s) for &: 'float' and 'float' (pdrf_exponent must be an integer type, "
                        "kimimaro/trace.py:313)")
    return i > 0 and (i & (i - 1)) == 0 and i < 2 ** 16

ST_BITS = {_KH["KH_ST_QUEUE_OVERFLOW"]: "work-list overflow", _KH["KH_ST_HEAP_OVERFLOW"]: "invalidation heap overflow",
           _KH["KH_ST_PATH_OVERFLOW"]: "path buffer overflow", _KH["KH_ST_NO_RAIL"]: "no rail reachable from a target",
           _KH["KH_ST_PLATEAU"]: "float-absorption plateau while back-tracking", _KH["KH_ST_BAD_TARGET"]: "target outside the label"}

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipUnavailableError(
            "kimimaro_amd: %s is missing. Build it with `python -m kimimaro_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    try:
        # PyTorch is the device-memory plumbing and bundles its own HIP runtime: load it FIRST so that
        # libkimi_hip.so binds to the same libamdhip64 (two runtimes in one process cannot share a GPU).
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise HipUnavailableError("kimimaro_amd: cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, restype, argtypes in PROTOTYPES:
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def last_error():
    buf = C.create_string_buffer(512)
    lib().kh_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc):
    if rc == 0:
        return
    msg = last_error()
    if rc == ENODEVICE:
        raise HipUnavailableError(msg)
    raise KimiHipError("libkimi_hip error %d: %s" % (rc, msg))


def require_gpu():
    """Raise unless the library loads AND a gfx950 device is visible."""
    L = lib()
    if L.kh_device_count() <= 0:
        raise HipUnavailableError(
            "kimimaro_amd: no gfx950 (MI355X) device visible; the product path has no CPU fallback.")
    return L


def describe_status(bits):
    return ", ".join(v for k, v in ST_BITS.items() if bits & k) or "ok"
