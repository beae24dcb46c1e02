"""Build recipe for the oracle (test infrastructure): gcc -> oracle/libkimi_oracle.so.

-ffp-contract=off: every float op is individually rounded, like numpy and like the
reference's g++ -O3 build on baseline x86-64 (no FMA), and like the HIP kernels.
"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "kimi_oracle.c")
LIB = os.path.join(HERE, "libkimi_oracle.so")


def build(force=False):
    if (not force and os.path.exists(LIB)
            and os.path.getmtime(LIB) >= os.path.getmtime(SRC)):
        return LIB
    # Link into a file of this process's own and rename it over LIB: two test processes that both find the library
    # stale (the world_size-2 workers of tests/test_distributed.py) then never load each other's half-written file.
    fd, tmp = tempfile.mkstemp(dir=HERE, prefix="libkimi_oracle.", suffix=".so")
    os.close(fd)
    try:
        subprocess.check_call(
            ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-Wall",
             "-shared", "-fPIC", SRC, "-o", tmp, "-lm"]
        )
        os.chmod(tmp, 0o755 & ~_umask())
        os.replace(tmp, LIB)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return LIB


def _umask():
    m = os.umask(0)
    os.umask(m)
    return m


if __name__ == "__main__":
    print(build(force=True))
