"""Build the in-tree HIP library ``minbft_amd/libminbft_amd.so`` for gfx950.

Plain ``hipcc`` invocations (no cmake): the kernel units (``*.hip``) are
compiled for ``--offload-arch=gfx950`` only, the host units are ordinary C++
linked into the same shared object.  Rebuilds only when a source is newer than
the library.

    python -m minbft_amd.build [--force]
"""
from __future__ import annotations

import argparse
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libminbft_amd.so")
OBJDIR = os.path.join(HERE, "build")

ARCH = os.environ.get("MBFT_OFFLOAD_ARCH", "gfx950")
# every translation unit's flags (tests/test_sign_resources.py compiles the
# signer's kernels with the same ones)
COMMON_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-I", os.path.join(ROOT, "include")]

# heaviest first (each verify form takes minutes): the pool starts them first
DEVICE_SOURCES = ["verify_split.hip", "verify_quads.hip", "verify_server.hip", "verify_pairs.hip", "verify_large.hip",
                  "msg_kernels.hip", "sign_kernels.hip", "prep_kernels.hip", "ninv_kernels.hip", "table_kernels.hip",
                  "p384_kernels.hip", "key_rank.hip", "memo.hip", "key_account.hip"]
HOST_SOURCES = ["host.cpp", "der.cpp", "messages.cpp", "batch.cpp", "msgdev.cpp", "winv_host.cpp",
                "sha256_host.cpp", "resident.cpp", "join_host.cpp", "sign.cpp", "keys.cpp", "p384.cpp"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (ROCm required to build minbft_amd)")


def _deps(src: str) -> list:
    """src, the quoted headers it includes (transitively), the public
    header and this script."""
    import re
    seen, todo = set(), [src]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(f):
            continue
        seen.add(f)
        with open(f, errors="replace") as fh:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M):
                todo.append(os.path.normpath(os.path.join(os.path.dirname(f), inc)))
    return sorted(seen) + [os.path.join(ROOT, "include", "minbft_gpu.h"), os.path.abspath(__file__)]


def _inputs() -> set:
    """Every file the library is built from: _deps() of every source."""
    return {d for f in DEVICE_SOURCES + HOST_SOURCES for d in _deps(os.path.join(CSRC, f))}


def up_to_date() -> bool:
    if not os.path.exists(LIB):
        return False
    t = os.path.getmtime(LIB)
    return all(os.path.getmtime(f) <= t for f in _inputs())


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and up_to_date():
        return LIB
    hipcc = _hipcc()
    os.makedirs(OBJDIR, exist_ok=True)
    common = COMMON_FLAGS
    jobs = []
    for f in DEVICE_SOURCES:
        obj = os.path.join(OBJDIR, f + ".o")
        jobs.append(([hipcc, f"--offload-arch={ARCH}", *common, "-c", os.path.join(CSRC, f), "-o", obj], obj))
    for f in HOST_SOURCES:
        obj = os.path.join(OBJDIR, f + ".o")
        jobs.append(([hipcc, *common, "-c", os.path.join(CSRC, f), "-o", obj], obj))

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"compile failed: {' '.join(cmd)}\n{p.stdout}\n{p.stderr}")
        return p

    # an object is rebuilt only when its source or a header it includes
    # (transitively, quoted includes) is newer, or the build script changed
    stale = [j for j in jobs if force or not os.path.exists(j[1])
             or os.path.getmtime(j[1]) < max(os.path.getmtime(d) for d in _deps(j[0][-3]))]
    if stale:
        with ThreadPoolExecutor(max_workers=min(len(stale), int(os.environ.get("MAX_JOBS", 16)))) as ex:
            list(ex.map(lambda j: run(j[0]), stale))
    tmp = LIB + ".tmp"
    run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp, *[o for _, o in jobs]])
    os.replace(tmp, LIB)
    return LIB


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("-v", "--verbose", action="store_true")
    a = ap.parse_args(argv)
    print(build(force=a.force, verbose=a.verbose))


if __name__ == "__main__":
    sys.exit(main())
