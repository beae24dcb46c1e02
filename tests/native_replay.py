"""The two replay programs of tests/native_replay/ (replay_host.cpp: the kh_host_* entry points of the product; replay_oracle.c:
the ko_* functions of oracle/kimi_oracle.c), built with AddressSanitizer and UBSan once per process into a temporary directory,
and the one way to use them: call() writes a case file (tests/native_replay/replay_io.h), runs the program as a child process
and returns what the program left in every buffer.  The sanitizers live in the child alone: nothing sanitized is loaded into
this interpreter and the child's environment is this process's, unchanged.

A program fails a case by a non-zero exit status or by a sanitizer's words on stderr; the whole stderr goes into the error."""
import atexit
import concurrent.futures
import os
import shutil
import struct
import subprocess
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native_replay")
CSRC = os.path.join(ROOT, "kimimaro_amd", "csrc")
MAGIC = 0x3150524B
CANARY = 0xA5                       # the byte every output buffer holds before the call
CHILD_TIMEOUT = 60                  # seconds for one case; a case takes milliseconds
REPORTS = ("AddressSanitizer", "LeakSanitizer", "runtime error:")

HOST, ORACLE = "replay_host", "replay_oracle"
_state = {"dir": None, "programs": None, "build_seconds": None, "run_seconds": 0.0, "runs": 0}


class ReplayFailure(AssertionError):
    pass


def hipcc():
    path = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return path if os.path.exists(path) else shutil.which("hipcc")


def gcc():
    return shutil.which("gcc")


def commands(outdir):
    """{program: (path, command line)}: the product's flags (kimimaro_amd/build.py) and the oracle's (oracle/build.py) with -O1 -g
    in place of their optimisation level, and the sanitizers on the host side only"""
    host = os.path.join(outdir, HOST)
    oracle = os.path.join(outdir, ORACLE)
    return {
        HOST: (host, [hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                      "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                      "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", host,
                      os.path.join(SRC, "replay_host.cpp")] + [os.path.join(CSRC, s) for s in ("common.hip", "join.hip", "section.hip")]),
        ORACLE: (oracle, [gcc(), "-O1", "-g", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                          "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined",
                          "-fno-omit-frame-pointer", "-o", oracle, os.path.join(SRC, "replay_oracle.c"),
                          os.path.join(ROOT, "oracle", "kimi_oracle.c"), "-lm"]),
    }


def programs():
    """{program: path of the executable}, built on the first call (the two compilers side by side)"""
    if _state["programs"] is None:
        outdir = tempfile.mkdtemp(prefix="native_replay_")
        atexit.register(shutil.rmtree, outdir, ignore_errors=True)
        _state["dir"] = outdir
        t0 = time.perf_counter()
        cmds = commands(outdir)

        def compile_one(name):
            done = subprocess.run(cmds[name][1], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            if done.returncode != 0:
                raise RuntimeError("building %s failed:\n%s\n%s" % (name, " ".join(cmds[name][1]), done.stdout))
            return name, cmds[name][0]

        with concurrent.futures.ThreadPoolExecutor(max_workers=2) as pool:
            _state["programs"] = dict(pool.map(compile_one, (HOST, ORACLE)))
        _state["build_seconds"] = time.perf_counter() - t0
    return _state["programs"]


def timings():
    """(seconds the build took, seconds spent in child processes, number of child processes)"""
    return _state["build_seconds"], _state["run_seconds"], _state["runs"]


def known_functions(program):
    out = subprocess.run([programs()[program], "--list"], stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT, check=True).stdout
    return out.split()


def canary(count, dtype, shape=None):
    """an output buffer before the call: every byte CANARY"""
    a = np.frombuffer(bytes([CANARY]) * (int(count) * np.dtype(dtype).itemsize), dtype=dtype).copy()
    return a if shape is None else a.reshape(shape, order="F")


def is_canary(a):
    return bool(np.all(np.ascontiguousarray(a).reshape(-1).view(np.uint8) == CANARY))


def _raw(a):
    """the bytes of an array in memory order (C or Fortran contiguous)"""
    a = np.asarray(a)
    if not (a.flags.c_contiguous or a.flags.f_contiguous):
        raise ValueError("case arrays are contiguous")
    return a.tobytes(order="A")


def case_bytes(arrays, calls):
    out = [struct.pack("<II", MAGIC, len(arrays))]
    for a in arrays:
        a = np.asarray(a)
        out.append(struct.pack("<QQ", a.dtype.itemsize, a.size))
        out.append(_raw(a))
    out.append(struct.pack("<I", len(calls)))
    for function, scalars, indices in calls:
        name = function.encode()
        out.append(struct.pack("<I", len(name)) + name)
        out.append(struct.pack("<I", len(scalars)))
        for s in scalars:
            if isinstance(s, (bool, np.bool_)) or isinstance(s, (int, np.integer)):
                out.append(b"i" + struct.pack("<q", int(s)))
            elif isinstance(s, (float, np.floating)):
                out.append(b"d" + struct.pack("<d", float(s)))
            else:
                raise TypeError("a scalar is an int or a float, not %r" % (s,))
        out.append(struct.pack("<I", len(indices)))
        out.append(struct.pack("<%di" % len(indices), *[-1 if i is None else int(i) for i in indices]))
    return b"".join(out)


def run(program, arrays, calls, expect_failure=False):
    """calls = [(function, scalars, [index into arrays or None = NULL, ...]), ...] made in order on one set of buffers.
    -> ([return value of every call], [every array as the program left it, dtype and shape of the input]).
    expect_failure: -> (exit status, stderr) instead, nothing is asserted (the harness's own self-test)."""
    exe = programs()[program]
    with tempfile.TemporaryDirectory(dir=_state["dir"]) as tmp:
        case, result = os.path.join(tmp, "case.bin"), os.path.join(tmp, "result.bin")
        with open(case, "wb") as f:
            f.write(case_bytes(arrays, calls))
        t0 = time.perf_counter()
        done = subprocess.run([exe, case, result], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace",
                              timeout=CHILD_TIMEOUT)
        _state["run_seconds"] += time.perf_counter() - t0
        _state["runs"] += 1
        if expect_failure:
            return done.returncode, done.stderr
        if done.returncode != 0 or any(word in done.stderr for word in REPORTS):
            raise ReplayFailure("%s %s: exit status %d\n%s" % (program, [c[0] for c in calls], done.returncode, done.stderr))
        with open(result, "rb") as f:
            blob = f.read()
    ncalls, = struct.unpack_from("<I", blob, 0)
    assert ncalls == len(calls)
    rets = list(struct.unpack_from("<%dq" % ncalls, blob, 4))
    at = 4 + 8 * ncalls
    narrays, = struct.unpack_from("<I", blob, at)
    assert narrays == len(arrays)
    at += 4
    outs = []
    for a in arrays:
        a = np.asarray(a)
        nbytes, = struct.unpack_from("<Q", blob, at)
        at += 8
        assert nbytes == a.nbytes
        flat = np.frombuffer(blob, dtype=a.dtype, count=a.size, offset=at).copy()
        outs.append(flat.reshape(a.shape, order="F" if (a.flags.f_contiguous and not a.flags.c_contiguous) else "C"))
        at += nbytes
    assert at == len(blob)
    return rets, outs


def call(program, function, scalars, arrays):
    """one call: scalars in the order of the function's scalar parameters, arrays in the order of its pointer parameters (None =
    NULL).  -> (return value, [every array after the call, None for a NULL])"""
    given = [a for a in arrays if a is not None]
    indices, k = [], 0
    for a in arrays:
        indices.append(None if a is None else k)
        k += a is not None
    rets, outs = run(program, given, [(function, list(scalars), indices)])
    outs = iter(outs)
    return rets[0], [None if a is None else next(outs) for a in arrays]
