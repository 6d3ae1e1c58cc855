"""Loader of the test-only HIP units under tests/device/: primitives.hip runs the in-register L D L^T layouts, the wave sums and
the reciprocals of rsr_mjx_amd/csrc/rsr_device.hpp one wave per problem, hfield.hip the height-field narrow phase (hfield_place /
hfield_search / hfield_finish, closest_on_triangle) one wave per NPAIR spheres.  Builds each with the product's compiler flags into
tests/device/_build/ (stale against its own source or any csrc header), loads it with ctypes as rsr_mjx_amd/_lib.py loads the
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
BUILD_DIR = os.path.join(_HERE, "device", "_build")
Unit = namedtuple("Unit", "src lib env flags")       # source, library, environment variable that overrides the library's path,
#                                                      flags on top of the product's
# hfield_strict: hfield.hip once more with fma contraction off.  Under the product's flags the compiler fuses a * b + c wherever it
# likes, differently in each kernel a function is inlined into, so the last bits of one C++ expression differ between two kernels;
# a bit-for-bit comparison of hfield_search with a serial scan is a statement about the source's arithmetic and the pick, and is
# made on this build, where every operation rounds as written in both.  Everything else runs the product-flags build.
UNITS = {name: Unit(os.path.join(_HERE, "device", src + ".hip"), os.path.join(BUILD_DIR, f"lib{name}.so"), env, flags)
         for name, src, env, flags in (("primitives", "primitives", "RSR_PRIM_LIB", []), ("hfield", "hfield", "RSR_HFIELD_LIB", []),
                                       ("hfield_strict", "hfield", "RSR_HFIELD_STRICT_LIB", ["-ffp-contract=off"]))}
SRC, LIB = UNITS["primitives"].src, UNITS["primitives"].lib

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

HF_SYMBOLS = ["rsr_hf_npair", "rsr_hf_contact", "rsr_hf_scan", "rsr_hf_triangle"]
HfContact = namedtuple("HfContact", "flag dist pos nrm state c0 r0 searched p q n jdist best q_pre best_pre")
HfScan = namedtuple("HfScan", "state q best")

_lib = None
_hf_lib = None


def _headers() -> list:
    return sorted(glob.glob(os.path.join(_build.CSRC, "*.hpp")) + glob.glob(os.path.join(_build.CSRC, "..", "..", "include", "*.h")))


def _stale(unit: str = "primitives") -> bool:
    u = UNITS[unit]
    if not os.path.exists(u.lib):
        return True
    t = os.path.getmtime(u.lib)
    return any(os.path.getmtime(f) > t for f in [u.src] + _headers())


def build(force: bool = False, unit: str = "primitives") -> str:
    """hipcc (gfx950, the product's flags) of one unit; returns the library's path."""
    u = UNITS[unit]
    if force or _stale(unit):
        os.makedirs(BUILD_DIR, exist_ok=True)
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = u.lib + f".{os.getpid()}.tmp"
        subprocess.check_call([hipcc] + _build.HIPCC_FLAGS + u.flags + ["-shared", u.src, "-o", tmp])
        os.replace(tmp, u.lib)
    return u.lib


def _open(unit: str) -> C.CDLL:
    import torch  # noqa: F401  (its HIP runtime first: see rsr_mjx_amd/_lib.py)
    return C.CDLL(os.environ.get(UNITS[unit].env) or build(unit=unit))      # override: a build of a modified header (mutation checks)


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    L = _open("primitives")
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


# ---------------------------------------------------------------- hfield.hip
def hf_lib(strict: bool = False) -> C.CDLL:
    global _hf_lib
    _hf_lib = _hf_lib or {}
    unit = "hfield_strict" if strict else "hfield"
    if unit not in _hf_lib:
        L = _open(unit)
        vp, i32 = C.c_void_p, C.c_int
        L.rsr_hf_npair.argtypes = []
        L.rsr_hf_contact.argtypes = [i32] + [vp] * 14
        L.rsr_hf_scan.argtypes = [i32] + [vp] * 11
        L.rsr_hf_triangle.argtypes = [i32, vp, vp]
        _hf_lib[unit] = L
    return _hf_lib[unit]


def hf_npair() -> int:
    """spheres per wave (host call: no GPU needed)"""
    return int(hf_lib().rsr_hf_npair())


def _hf_inputs(hsize, data, hpos, hmat, spos, radius):
    data = np.asarray(data, dtype=np.float32)
    nrow, ncol = data.shape
    assert nrow >= 3 and ncol >= 3, "the host refuses smaller fields (check_hfield); the clamps assume it"
    spos = np.asarray(spos, dtype=np.float32)
    n, npair = spos.shape[0], hf_npair()
    assert spos.shape == (n, npair, 3) and np.shape(radius) == (n, npair) and np.shape(hpos) == (n, 3) and np.shape(hmat) == (n, 3, 3)
    assert np.shape(hsize) == (4,)
    t = [_dev(hsize), _dev(data), _dev([nrow], np.int32), _dev([ncol], np.int32), _dev(hpos), _dev(hmat), _dev(spos), _dev(radius)]
    return n, npair, t


def hf_contact(hsize, data, hpos, hmat, spos, radius, strict: bool = False) -> HfContact:
    """n waves of NPAIR spheres against the field (hsize[4], data[nrow, ncol]) in collision()'s sequence.  hpos[n, 3], hmat[n, 3, 3]
    (row-major), spos[n, NPAIR, 3], radius[n, NPAIR].  Returns per pair the contact and the raw HfJob (searched: the wave ran
    hfield_search; q_pre / best_pre: the job's q / best before it; fields hfield_place does not write hold -7.25 / -1).
    strict: the build without fma contraction (UNITS)."""
    import torch
    n, npair, t = _hf_inputs(hsize, data, hpos, hmat, spos, radius)
    z = lambda *s, dt=torch.float32: torch.zeros((n, npair) + s, dtype=dt, device="cuda")
    flag, dist, pos, nrm, ji, jf = z(dt=torch.int32), z(), z(3), z(3), z(4, dt=torch.int32), z(16)
    torch.cuda.synchronize()
    _check(hf_lib(strict).rsr_hf_contact(n, *[x.data_ptr() for x in t + [flag, dist, pos, nrm, ji, jf]]), "hf_contact")
    ji, jf = ji.cpu().numpy(), jf.cpu().numpy()
    return HfContact(flag.cpu().numpy(), dist.cpu().numpy(), pos.cpu().numpy(), nrm.cpu().numpy(), ji[..., 0], ji[..., 1], ji[..., 2],
                     ji[..., 3], jf[..., 0:3], jf[..., 3:6], jf[..., 6:9], jf[..., 9], jf[..., 10], jf[..., 11:14], jf[..., 14])


def hf_scan(hsize, data, hpos, hmat, spos, radius, strict: bool = False) -> HfScan:
    """hfield_place and then the unit's serial scan (k = 0..7, strict <) by the pair's lane: state, q, best per pair."""
    import torch
    n, npair, t = _hf_inputs(hsize, data, hpos, hmat, spos, radius)
    state = torch.zeros((n, npair), dtype=torch.int32, device="cuda")
    q = torch.zeros((n, npair, 3), dtype=torch.float32, device="cuda")
    best = torch.zeros((n, npair), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _check(hf_lib(strict).rsr_hf_scan(n, *[x.data_ptr() for x in t + [state, q, best]]), "hf_scan")
    return HfScan(state.cpu().numpy(), q.cpu().numpy(), best.cpu().numpy())


def hf_triangle(p, a, b, c):
    """closest_on_triangle of p[n, 3] on (a, b, c)[n, 3], one lane each"""
    import torch
    v = np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1, 3) for x in (p, a, b, c)], axis=1)
    tv = _dev(v)
    q = torch.zeros((len(v), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _check(hf_lib().rsr_hf_triangle(len(v), tv.data_ptr(), q.data_ptr()), "hf_triangle")
    return q.cpu().numpy()
