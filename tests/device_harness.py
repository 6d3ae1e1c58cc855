"""Loader of tests/device/primitives.hip: the test-only HIP unit that runs the in-register L D L^T layouts, the wave sums and
the reciprocals of rsr_mjx_amd/csrc/rsr_device.hpp one wave per problem.  Builds it with the product's compiler flags into
tests/device/_build/ (stale against primitives.hip or any csrc header), loads it with ctypes as rsr_mjx_amd/_lib.py loads the
product library.  Nothing here decodes a layout: factor() returns the raw per-lane registers of all 64 lanes."""
from __future__ import annotations

import ctypes as C
import glob
import os
import shutil
import subprocess
from collections import namedtuple

import numpy as np

from rsr_mjx_amd import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "device", "primitives.hip")
BUILD_DIR = os.path.join(_HERE, "device", "_build")
LIB = os.path.join(BUILD_DIR, "libprimitives.so")

SYMBOLS = ["rsr_prim_dims", "rsr_prim_supported", "rsr_prim_nreg", "rsr_prim_factor", "rsr_prim_lane_map", "rsr_prim_sums",
           "rsr_prim_recips"]
KINDS = {"natural": 0, "rowchol": 1, "rowtree": 2, "arrow": 3}
DIMS = {"CubeDims": 0, "TShapeDims": 1, "Go2FlatDims": 2, "Go2Dims": 3, "HandDims": 4}
MASS_ONLY, HAS_DIAG = 1, 2                 # bits of `mode`: the factor's template arguments
DIMS_FIELDS = ("NV", "NCH", "LD", "ISO0", "ISO1", "TREE1", "TREE2", "NCT", "ANT", "ALEGN", "ALEGS", "NA", "NISO",
               "ROWCHOL", "ROWTREE", "ARROW")
DimsConst = namedtuple("DimsConst", DIMS_FIELDS)
Factor = namedtuple("Factor", "a lt dinv x")          # [n, 64, NREG] x 2, [n, 64] x 2 (float32, raw lane registers)
Sums = namedtuple("Sums", "wave_sum row_sum16 wave_sum3")      # [n, 3, 64] each

_lib = None


def _headers() -> list:
    return sorted(glob.glob(os.path.join(_build.CSRC, "*.hpp")) + glob.glob(os.path.join(_build.CSRC, "..", "..", "include", "*.h")))


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(f) > t for f in [SRC] + _headers())


def build(force: bool = False) -> str:
    """hipcc (gfx950, the product's flags) of the one unit; returns the library's path."""
    if force or _stale():
        os.makedirs(BUILD_DIR, exist_ok=True)
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = LIB + f".{os.getpid()}.tmp"
        subprocess.check_call([hipcc] + _build.HIPCC_FLAGS + ["-shared", SRC, "-o", tmp])
        os.replace(tmp, LIB)
    return LIB


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (its HIP runtime first: see rsr_mjx_amd/_lib.py)
    L = C.CDLL(os.environ.get("RSR_PRIM_LIB") or build())      # override: a build of a modified header (mutation checks)
    vp, i32 = C.c_void_p, C.c_int
    L.rsr_prim_dims.argtypes = [i32, C.POINTER(i32)]
    L.rsr_prim_supported.argtypes = [i32, i32, i32]
    L.rsr_prim_nreg.argtypes = [i32, i32]
    L.rsr_prim_factor.argtypes = [i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.rsr_prim_lane_map.argtypes = [i32, i32, vp, vp]
    L.rsr_prim_sums.argtypes = [i32, vp, vp, vp, vp]
    L.rsr_prim_recips.argtypes = [i32, vp, vp, vp, vp]
    _lib = L
    return L


def dims(name: str) -> DimsConst:
    """Compile-time constants of one shipped Dims instantiation (host call: no GPU needed)."""
    out = (C.c_int * len(DIMS_FIELDS))()
    rc = lib().rsr_prim_dims(DIMS[name], out)
    assert rc == 0, (name, rc)
    return DimsConst(*[int(v) for v in out])


def supported(kind: str, dims_name: str, mode: int) -> bool:
    return bool(lib().rsr_prim_supported(KINDS[kind], DIMS[dims_name], mode))


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what}: " + ("unsupported combination" if rc == -1 else f"hipError_t {rc}"))


def _dev(x, dtype=np.float32):
    import torch
    return torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()      # (a copy: the tests' shared inputs are read-only)


def factor(kind: str, dims_name: str, mode: int, H, diag=None, b=None, alias: int = 0, pad=None) -> Factor:
    """Factor + solve of H[n, NV, NV] (float32), one wave per matrix.  `pad[n, NV]` fills the padding word of each LDS row
    (default 0); `diag` is handed to the HAS_DIAG modes, `b` is the right-hand side.  Returns the raw registers."""
    import torch
    L, d = lib(), dims(dims_name)
    H = np.asarray(H, dtype=np.float32)
    n = H.shape[0]
    assert H.shape == (n, d.NV, d.NV)
    Hp = np.zeros((n, d.NV, d.LD), dtype=np.float32)
    Hp[:, :, :d.NV] = H
    if pad is not None:
        Hp[:, :, d.NV:] = np.asarray(pad, dtype=np.float32).reshape(n, d.NV, d.LD - d.NV)
    diag = np.zeros((n, d.NV), np.float32) if diag is None else np.asarray(diag, np.float32)
    b = np.zeros((n, d.NV), np.float32) if b is None else np.asarray(b, np.float32)
    assert diag.shape == (n, d.NV) and b.shape == (n, d.NV)
    nreg = L.rsr_prim_nreg(KINDS[kind], DIMS[dims_name])
    tH, tD, tB = _dev(Hp), _dev(diag), _dev(b)
    a = torch.zeros((n, 64, nreg), dtype=torch.float32, device="cuda")
    lt = torch.zeros_like(a)
    dinv = torch.zeros((n, 64), dtype=torch.float32, device="cuda")
    x = torch.zeros_like(dinv)
    torch.cuda.synchronize()
    _check(L.rsr_prim_factor(KINDS[kind], DIMS[dims_name], mode, n, tH.data_ptr(), tD.data_ptr(), tB.data_ptr(), int(alias),
                             a.data_ptr(), lt.data_ptr(), dinv.data_ptr(), x.data_ptr()), f"factor {kind} {dims_name} mode {mode}")
    return Factor(a.cpu().numpy(), lt.cpu().numpy(), dinv.cpu().numpy(), x.cpu().numpy())


def lane_map(kind: str, dims_name: str):
    """The device's own (dof_of_lane[64], lane_of_dof[NV]) of a layout."""
    import torch
    d = dims(dims_name)
    dof = torch.zeros(64, dtype=torch.int32, device="cuda")
    lane = torch.zeros(d.NV, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _check(lib().rsr_prim_lane_map(KINDS[kind], DIMS[dims_name], dof.data_ptr(), lane.data_ptr()), f"lane_map {kind} {dims_name}")
    return dof.cpu().numpy(), lane.cpu().numpy()


def sums(v) -> Sums:
    """v[n, 64] (the same vector in all three slots of wave_sum3) or v[n, 3, 64] (three vectors)."""
    import torch
    v = np.asarray(v, dtype=np.float32)
    if v.ndim == 2:
        v = np.repeat(v[:, None, :], 3, axis=1)
    n = v.shape[0]
    assert v.shape == (n, 3, 64)
    tv = _dev(v)
    out = [torch.zeros((n, 3, 64), dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    _check(lib().rsr_prim_sums(n, tv.data_ptr(), *[o.data_ptr() for o in out]), "sums")
    return Sums(*[o.cpu().numpy() for o in out])


def recips(x):
    """(frcp, frsq, fsqrt) of x[n] (float32)."""
    import torch
    x = np.asarray(x, dtype=np.float32).ravel()
    tx = _dev(x)
    out = [torch.zeros(x.size, dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    _check(lib().rsr_prim_recips(x.size, tx.data_ptr(), *[o.data_ptr() for o in out]), "recips")
    return tuple(o.cpu().numpy() for o in out)
