"""Builds librsrmjx.so (HIP, gfx950) in-tree next to its sources."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB = os.path.join(CSRC, "librsrmjx.so")
# One translation unit per source: the kernels of one model family each (cube, T-shape, Go2: rsr_launch.hpp) and the two host
# units (the C ABI of include/rsr_mjx.h and of include/rsr_physics.h).  The T-shape and Go2 units are built with the SLP vectoriser
# off (its packed-fp32 pairing costs the Go2 and T-shape kernels ~3 % and gains the cube kernels ~0.5 %; measured A/B on one box).
# Kernels of one unit also perturb each other's register allocation: a unit holds one model family.
UNITS = [("rsr_cube.hip", []), ("rsr_tshape.hip", ["-fno-slp-vectorize"]), ("rsr_go2.hip", ["-fno-slp-vectorize"]),
         ("rsr_mjx.hip", []), (os.path.join("physics", "rsr_physics.hip"), [])]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


def _sources() -> list:
    """Every file the library is built from: csrc/ and csrc/physics/ sources and headers, and include/."""
    inc = os.path.join(_HERE, "..", "include")
    dirs = [CSRC, os.path.join(CSRC, "physics"), inc]
    return [os.path.join(d, f) for d in dirs for f in sorted(os.listdir(d)) if f.endswith((".hip", ".hpp", ".h"))]


def _stale(lib: str) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(f) > t for f in _sources()) or os.path.getmtime(__file__) > t


def compile_lib(lib: str = LIB, extra_flags=(), verbose: bool = False) -> str:
    """hipcc -c of every unit (in parallel), then the link; `extra_flags` go to every unit (e.g. -DRSR_PROFILE)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    stem = os.path.splitext(os.path.basename(lib))[0]
    objs, procs = [], []
    for src, flags in UNITS:
        o = os.path.join(CSRC, f"{stem}.{os.path.splitext(os.path.basename(src))[0]}.o")
        cmd = [hipcc] + HIPCC_FLAGS + list(flags) + list(extra_flags) + ["-c", os.path.join(CSRC, src), "-o", o]
        if verbose:
            cmd.append("-Rpass-analysis=kernel-resource-usage")
        objs.append(o)
        procs.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs, cwd=CSRC)
    for o in objs:
        os.remove(o)
    return lib


def build(force: bool = False, verbose: bool = False) -> str:
    """Compiles the HIP extension for gfx950 (hipcc cross-compiles without a GPU).  Returns the .so path."""
    if not force and not _stale(LIB):
        return LIB
    return compile_lib(LIB, verbose=verbose)


if __name__ == "__main__":
    print(build(force=True, verbose=True))
