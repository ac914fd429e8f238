"""Build libbsgpu.so in-tree for gfx950 (hipcc, no JIT cache): `python -m bs_amd.build`."""
from __future__ import annotations

import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libbsgpu.so")
SOURCES = ["bsgpu_kernels.hip", "bsgpu_host.cpp", "host_sha256.cpp", "bs_split.cpp",
           "bs_filestore.cpp"]
ARCH = os.environ.get("BSG_OFFLOAD_ARCH", "gfx950")
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def _deps() -> list[str]:
    """SOURCES and every file they reach through #include "...", each relative to the file
    that names it (so ../../include/bsgpu.h works), as normalised absolute paths."""
    todo = [os.path.join(CSRC, f) for f in SOURCES]
    seen = []
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.append(path)
        with open(path, encoding="utf-8", errors="replace") as f:
            names = _INCLUDE.findall(f.read())
        todo += [os.path.join(os.path.dirname(path), n) for n in names]
    return sorted(seen)


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in _deps())


def _hipcc_cmd(out: str, extra_flags=()) -> list[str]:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared",
            *extra_flags, "-o", out, *(os.path.join(CSRC, f) for f in SOURCES)]


def build_locked(out: str, stale, compile_to) -> bool:
    """Runs compile_to(tmp) and renames tmp to `out` if stale() holds, under an exclusive
    flock on out + ".lock", so concurrent builders (bench ranks, test workers) compile once:
    the others wait, re-check stale() and find the fresh library. The temporary file is per
    process and the rename is atomic, so a process loading `out` never sees a partial file.
    Returns True if this call compiled."""
    import fcntl
    with open(out + ".lock", "a") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if not stale():
                return False
            tmp = f"{out}.tmp.{os.getpid()}"
            try:
                compile_to(tmp)
                os.replace(tmp, out)
            finally:
                if os.path.exists(tmp):
                    os.unlink(tmp)
            return True
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB

    def compile_to(tmp):
        cmd = _hipcc_cmd(tmp, ["-Wall", "-Wno-unused-function", "-Wno-unused-value",
                               "-Wno-unused-result"])
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)

    forced = [force]

    def stale():
        if forced[0]:
            forced[0] = False
            return True
        return _stale()

    build_locked(LIB, stale, compile_to)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
