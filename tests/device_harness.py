"""Loader of the test-only HIP units under tests/device/: primitives.hip runs the in-register L D L^T layouts, the wave sums and
the reciprocals of rsr_mjx_amd/csrc/rsr_device.hpp one wave per problem, hfield.hip the height-field narrow phase (hfield_place /
hfield_search / hfield_finish, closest_on_triangle) one wave per NPAIR spheres, solver_rows.hip the Newton solver's leaf functions
(rows_cost, ls_prepare / ls_point / ls_eval / ls_costs, jdot, jt_force of rsr_solver.hpp) one wave per problem.  Builds each with the product's compiler flags into
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
# solver_rows_strict: the same for solver_rows.hip (ls_eval<3> against three ls_point, bit for bit); its tests run on both builds.
UNITS = {name: Unit(os.path.join(_HERE, "device", src + ".hip"), os.path.join(BUILD_DIR, f"lib{name}.so"), env, flags)
         for name, src, env, flags in (("primitives", "primitives", "RSR_PRIM_LIB", []), ("hfield", "hfield", "RSR_HFIELD_LIB", []),
                                       ("hfield_strict", "hfield", "RSR_HFIELD_STRICT_LIB", ["-ffp-contract=off"]),
                                       ("solver_rows", "solver_rows", "RSR_SOLVER_ROWS_LIB", []),
                                       ("solver_rows_strict", "solver_rows", "RSR_SOLVER_ROWS_STRICT_LIB", ["-ffp-contract=off"]))}
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

SR_SYMBOLS = ["rsr_sr_dims", "rsr_sr_rows_cost", "rsr_sr_linesearch", "rsr_sr_jproducts"]
SR_DIMS = ("CubeDims", "TShapeDims", "Go2FlatDims", "HandDims")           # (Go2Dims shares Go2FlatDims' row constants)
SR_DIMS_FIELDS = ("NV", "NEQ", "NF", "NL", "NCON", "NPYR", "NBC", "NEFC", "NCHUNK", "NBASE", "LDJ")
SrDims = namedtuple("SrDims", SR_DIMS_FIELDS)
RowsCost = namedtuple("RowsCost", "cost cost_lane force hw")      # [n, 64] x 2, [n, 2, NCHUNK, 64] x 2 (REDUCE = true, false)
LineSearch = namedtuple("LineSearch", "pt ev cost")               # [n, 3, 4] x 2 (q1, q2, d0(), d1()), [n, 2, 3]
JProducts = namedtuple("JProducts", "jd qfc")                     # [n, NCHUNK, 64], [n, 64]

_lib = None
_hf_lib = None
_sr_lib = None


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


# ---------------------------------------------------------------- solver_rows.hip
def sr_lib(strict: bool = False) -> C.CDLL:
    global _sr_lib
    _sr_lib = _sr_lib or {}
    unit = "solver_rows_strict" if strict else "solver_rows"
    if unit not in _sr_lib:
        L = _open(unit)
        vp, i32 = C.c_void_p, C.c_int
        L.rsr_sr_dims.argtypes = [i32, C.POINTER(i32)]
        L.rsr_sr_rows_cost.argtypes = [i32, i32] + [vp] * 9
        L.rsr_sr_linesearch.argtypes = [i32, i32] + [vp] * 11
        L.rsr_sr_jproducts.argtypes = [i32, i32] + [vp] * 6 + [C.c_float] + [vp] * 7
        _sr_lib[unit] = L
    return _sr_lib[unit]


def sr_dims(name: str) -> SrDims:
    """Row constants of one shipped Dims instantiation (host call: no GPU needed)."""
    out = (C.c_int * len(SR_DIMS_FIELDS))()
    rc = sr_lib().rsr_sr_dims(DIMS[name], out)
    assert rc == 0, (name, rc)
    return SrDims(*[int(v) for v in out])


def _sr_rows(d: SrDims, nefc, *per_lane):
    """device tensors of nefc[n] and of the per-lane arrays [n, NCHUNK, 64] (float32, or int32 for integer inputs)"""
    nefc = np.asarray(nefc, dtype=np.int32)
    n = len(nefc)
    assert n > 0 and (nefc >= d.NEQ + d.NF).all() and (nefc <= d.NEFC).all(), "nefc outside [NEQ + NF, NEFC]"
    out = [_dev(nefc, np.int32)]
    for a in per_lane:
        a = np.asarray(a)
        assert a.shape == (n, d.NCHUNK, 64), (a.shape, (n, d.NCHUNK, 64))
        out.append(_dev(a, np.int32 if a.dtype.kind in "iu" else np.float32))
    return n, out


def rows_cost(dims_name: str, nefc, jaref, D, R, floss, strict: bool = False) -> RowsCost:
    """rows_cost<C, true> and rows_cost<C, false> of n waves: the reduced cost as every lane holds it, each lane's share, and the
    force / weight registers of both calls.  Inputs [n, NCHUNK, 64] (row = lane + 64 * chunk)."""
    import torch
    d = sr_dims(dims_name)
    n, t = _sr_rows(d, nefc, jaref, D, R, floss)
    cost, lane = (torch.zeros((n, 64), dtype=torch.float32, device="cuda") for _ in range(2))
    force, hw = (torch.zeros((n, 2, d.NCHUNK, 64), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    _check(sr_lib(strict).rsr_sr_rows_cost(DIMS[dims_name], n, *[x.data_ptr() for x in t + [cost, lane, force, hw]]), "rows_cost")
    return RowsCost(*[x.cpu().numpy() for x in (cost, lane, force, hw)])


def linesearch(dims_name: str, nefc, jaref, jv, D, R, floss, g, alpha, strict: bool = False) -> LineSearch:
    """ls_prepare once, then ls_point at each of alpha[n, 3], ls_eval<C, 3> at the three together and ls_costs on either set of
    points; g[n, 3] = (g0, g1, g2)."""
    import torch
    d = sr_dims(dims_name)
    n, t = _sr_rows(d, nefc, jaref, jv, D, R, floss)
    assert np.shape(g) == (n, 3) and np.shape(alpha) == (n, 3)
    t += [_dev(g), _dev(alpha)]
    pt, ev = (torch.zeros((n, 3, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    cost = torch.zeros((n, 2, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _check(sr_lib(strict).rsr_sr_linesearch(DIMS[dims_name], n, *[x.data_ptr() for x in t + [pt, ev, cost]]), "linesearch")
    return LineSearch(pt.cpu().numpy(), ev.cpu().numpy(), cost.cpu().numpy())


def jproducts(dims_name: str, nl, ncon, B, bmu, sdof, mu, bn, bk, v, force, poison: float = float("nan"), strict: bool = False) -> JProducts:
    """vec_bcast + jdot of v[n, NV] and jt_force of force[n, NCHUNK, 64] on n LDS images.  nl[n], ncon[n]: active limits and
    contacts (nefc = NEQ + NF + nl + NPYR ncon, nbase = NEQ + NF + nl + NBC ncon); B[n, NBASE, NV]: the base rows, of which the
    first nbase are used; bmu[n, NBASE]: of which the contact tangents' are used; sdof[n, NSP]: of which the friction and limit
    rows' are used; mu, bn, bk [n, NCHUNK, 64]: the rows' registers (padding rows: 0, NBASE, NBASE).  The image holds these words,
    a zero null row and bval[NBASE .. NBASE + 4) = 0; every other word of J, bmu, bval, rw, jtp, wc and dgw holds `poison`
    (solver_rows.hip states the contract)."""
    import torch
    d = sr_dims(dims_name)
    nl, ncon = np.asarray(nl, dtype=np.int32), np.asarray(ncon, dtype=np.int32)
    assert (nl >= 0).all() and (nl <= d.NL).all() and (ncon >= 0).all() and (ncon <= d.NCON).all()
    rcon = d.NEQ + d.NF + nl
    nefc, nbase = rcon + d.NPYR * ncon, rcon + d.NBC * ncon
    bn, bk, sdof = np.asarray(bn), np.asarray(bk), np.asarray(sdof)
    n, t = _sr_rows(d, nefc, np.asarray(mu, np.float32), bn.astype(np.int32), bk.astype(np.int32))
    nsp = d.NEQ + d.NF + d.NL
    assert (bn >= 0).all() and (bn <= d.NBASE).all() and (bk >= 0).all() and (bk <= d.NBASE).all(), "base row index outside the image"
    assert sdof.shape == (n, nsp) and (sdof >= 0).all() and (sdof < d.NV).all(), "dof index outside the row"
    B, bmu = np.asarray(B, np.float32), np.asarray(bmu, np.float32)
    assert B.shape == (n, d.NBASE, d.NV) and bmu.shape == (n, d.NBASE) and np.shape(v) == (n, d.NV) and np.shape(force) == (n, d.NCHUNK, 64)
    J = np.full((n, d.NBASE + 1, d.LDJ), poison, np.float32)
    live = np.arange(d.NBASE)[None, :] < nbase[:, None]
    J[:, :d.NBASE, :d.NV] = np.where(live[:, :, None], B, np.float32(poison))
    J[:, d.NBASE, :] = 0.0
    k = np.arange(d.NBASE)[None, :] - rcon[:, None]
    tangent = live & (k >= 0) & (k % d.NBC != 0)
    bmu_i = np.full((n, d.NBASE + 4), poison, np.float32)
    bmu_i[:, :d.NBASE] = np.where(tangent, bmu, np.float32(poison))
    bval = np.full((n, d.NBASE + 4), poison, np.float32)
    bval[:, d.NBASE:] = 0.0
    sd = np.zeros((n, nsp + 1), np.int32)
    r = np.arange(nsp)[None, :]
    sd[:, :nsp] = np.where((r >= d.NEQ) & (r < rcon[:, None]), sdof, 0)
    jd = torch.zeros((n, d.NCHUNK, 64), dtype=torch.float32, device="cuda")
    qfc = torch.zeros((n, 64), dtype=torch.float32, device="cuda")
    nefc_t, mu_t, bn_t, bk_t = t
    args = [nefc_t, _dev(ncon, np.int32), _dev(J), _dev(bmu_i), _dev(bval), _dev(sd, np.int32)]
    tail = [mu_t, bn_t, bk_t, _dev(v), _dev(force), jd, qfc]
    torch.cuda.synchronize()
    _check(sr_lib(strict).rsr_sr_jproducts(DIMS[dims_name], n, *[x.data_ptr() for x in args], C.c_float(poison),
                                           *[x.data_ptr() for x in tail]), "jproducts")
    return JProducts(jd.cpu().numpy(), qfc.cpu().numpy())
