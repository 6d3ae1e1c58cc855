"""The test-only HIP unit of the height-field narrow phase (tests/device/hfield.hip, tests/device_harness.py) on the CPU: it
compiles for gfx950, exports its entry points and goes stale with the csrc headers; and the plain fp64 reference of the
sphere / height-field contact that tests/test_device_hfield_gpu.py holds the kernel to, checked here against the oracle.

The reference (ref_hfield) does not follow the oracle's construction: for a centre above the surface it takes the closest point
over ALL triangles of the 5 x 5 cells around the centre's cell, clipped to the field, with a closest point per triangle that is
not Ericson's region walk (projection onto the plane where the barycentric coordinates are inside, else the nearest of the three
edges); it also returns the gap to the runner-up -- the smallest distance among triangles whose closest point lies more than
1e-6 m from the winner's -- so that a tie between facets can be told from an error.  Below the surface it is the perpendicular
depth to the plane of the triangle over the centre, with the distance of (u, v) from the nearest cell edge or the diagonal.

test_reference_agrees_with_the_f64_oracle: on every input of the GPU module (6 fields x 2 poses, 7824 spheres, 5779 of them touching)
the f64 oracle's dist is within 1e-12 of the reference wherever the sphere touches, with NO exclusion (the distance to the surface
is 1-Lipschitz: a tie cannot move it), except below the surface within 1e-4 of a cell edge or the diagonal; pos / nrm agree to
1e-9 wherever the runner-up is more than 1e-4 m away.  The inputs include r = cell / 2 exactly, the host's limit: there the
oracle's 2 x 2 window still finds what the 5 x 5 window finds, which is the claim "the sphere spans at most two grid lines"."""
import os

import numpy as np
import pytest

import device_harness as DH

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rsr_mjx_amd", "assets")
GAP_MIN = 1e-4            # m: pos / nrm are compared only where the runner-up facet is further away than this
EDGE_MIN = 1e-4           # (u, v) units: below the surface, inputs this close to a cell edge or the diagonal are left out
(P_RANDOM, P_GRID, P_SURFACE, P_BELOW, P_EDGE_CELL, P_BORDER, P_OUTSIDE, P_MIXED) = range(1, 9)
FIELDS = ["shipped", "f3x3", "f3x7", "f7x3", "steep9", "flat"]
POSES = ["identity", "moved"]


# ---------------------------------------------------------------- the fp64 reference
def _seg(p, s, e):
    d = e - s
    t = np.clip((np.einsum("...k,...k", p - s, d) / np.einsum("...k,...k", d, d)), 0.0, 1.0)
    return s + t[..., None] * d


def closest_tri(p, a, b, c):
    """closest point of triangle abc to p, fp64, broadcast over leading axes: the projection onto the plane where it falls
    inside, else the nearest point of the three edges"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, c)))
    ab, ac, ap = b - a, c - a, p - a
    d00, d01, d11 = (np.einsum("...k,...k", x, y) for x, y in ((ab, ab), (ab, ac), (ac, ac)))
    d20, d21 = np.einsum("...k,...k", ap, ab), np.einsum("...k,...k", ap, ac)
    den = d00 * d11 - d01 * d01
    v, w = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    inside = (v >= 0) & (w >= 0) & (v + w <= 1)
    q = a + v[..., None] * ab + w[..., None] * ac
    cand = np.stack([_seg(p, a, b), _seg(p, b, c), _seg(p, c, a)])
    dist = np.linalg.norm(cand - p, axis=-1)
    k = np.argmin(dist, axis=0)
    qe = np.take_along_axis(cand, k[None, ..., None], axis=0)[0]
    return np.where(inside[..., None], q, qe)


def _grid(hsize, data):
    hs = np.asarray(hsize, np.float32).astype(np.float64)
    dat = np.asarray(data, np.float32).astype(np.float64)
    nrow, ncol = dat.shape
    return hs[0], hs[1], hs[2], dat, nrow, ncol, 2 * hs[0] / (ncol - 1), 2 * hs[1] / (nrow - 1)


def surface_under(hsize, data, x, y):
    """(zs, gx, gy, margin) of the triangle over (x, y), fp64: height, gradient, and the distance of (u, v) from the nearest
    cell edge or the diagonal (cells split along (col, row) - (col + 1, row + 1))"""
    sx, sy, sz, dat, nrow, ncol, dx, dy = _grid(hsize, data)
    ci = np.clip(np.floor((x + sx) / dx).astype(int), 0, ncol - 2)
    ri = np.clip(np.floor((y + sy) / dy).astype(int), 0, nrow - 2)
    u, v = (x - (-sx + dx * ci)) / dx, (y - (-sy + dy * ri)) / dy
    z00, z10, z01, z11 = dat[ri, ci] * sz, dat[ri, ci + 1] * sz, dat[ri + 1, ci] * sz, dat[ri + 1, ci + 1] * sz
    low = u >= v
    gx = np.where(low, z10 - z00, z11 - z01) / dx
    gy = np.where(low, z11 - z10, z01 - z00) / dy
    zs = z00 + gx * dx * u + gy * dy * v
    margin = np.minimum.reduce([u, 1 - u, v, 1 - v, np.abs(u - v)])
    return zs, gx, gy, margin


def ref_hfield(hsize, data, hpos, hmat, spos, radius):
    """fp64 sphere / height-field contact of M spheres (hpos[M, 3], hmat[M, 3, 3], spos[M, 3], radius[M], the fp32 values as
    given).  Returns a dict: flag, dist, pos, nrm (world), p, q, n (field frame), below, gap (above the surface; inf below),
    margin and depth (below the surface; inf and 0 above)."""
    sx, sy, sz, dat, nrow, ncol, dx, dy = _grid(hsize, data)
    hpos, hmat, spos, radius = (np.asarray(x, np.float32).astype(np.float64) for x in (hpos, hmat, spos, radius))
    M = len(spos)
    p = np.einsum("mkc,mk->mc", hmat, spos - hpos)
    flag = (np.abs(p[:, 0]) <= sx) & (np.abs(p[:, 1]) <= sy)
    zs, gx, gy, margin = surface_under(hsize, data, p[:, 0], p[:, 1])
    below = p[:, 2] < zs
    inv = 1.0 / np.sqrt(gx * gx + gy * gy + 1.0)
    n_b = np.stack([-gx * inv, -gy * inv, inv], 1)
    depth = (zs - p[:, 2]) * inv
    q_b, dist_b = p + n_b * depth[:, None], -depth - radius
    # above: every triangle of the 5 x 5 cells around the centre's cell
    ci = np.clip(np.floor((p[:, 0] + sx) / dx).astype(int), 0, ncol - 2)
    ri = np.clip(np.floor((p[:, 1] + sy) / dy).astype(int), 0, nrow - 2)
    Q, D = [], []
    for dr in range(-2, 3):
        for dc in range(-2, 3):
            c, r = ci + dc, ri + dr
            ok = (c >= 0) & (c <= ncol - 2) & (r >= 0) & (r <= nrow - 2)
            cc, rr = np.clip(c, 0, ncol - 2), np.clip(r, 0, nrow - 2)
            xa, ya = -sx + dx * cc, -sy + dy * rr
            v00 = np.stack([xa, ya, dat[rr, cc] * sz], 1); v10 = np.stack([xa + dx, ya, dat[rr, cc + 1] * sz], 1)
            v01 = np.stack([xa, ya + dy, dat[rr + 1, cc] * sz], 1); v11 = np.stack([xa + dx, ya + dy, dat[rr + 1, cc + 1] * sz], 1)
            for tri in ((v00, v10, v11), (v00, v11, v01)):
                qq = closest_tri(p, *tri)
                Q.append(qq); D.append(np.where(ok, np.linalg.norm(p - qq, axis=1), np.inf))
    Q, D = np.stack(Q, 1), np.stack(D, 1)                      # [M, 50, 3], [M, 50]
    kw = np.argmin(D, axis=1)
    q_a, dn = Q[np.arange(M), kw], D[np.arange(M), kw]
    other = np.linalg.norm(Q - q_a[:, None, :], axis=2) > 1e-6
    gap = np.where(other, D, np.inf).min(1) - dn
    safe = np.where(dn < 1e-12, 1.0, dn)
    n_a = np.where((dn < 1e-12)[:, None], np.array([0.0, 0.0, 1.0]), (p - q_a) / safe[:, None])
    q = np.where(below[:, None], q_b, q_a)
    n = np.where(below[:, None], n_b, n_a)
    dist = np.where(below, dist_b, dn - radius)
    pl = q + n * (0.5 * dist)[:, None]
    return dict(flag=flag, dist=dist, pos=hpos + np.einsum("mck,mk->mc", hmat, pl), nrm=np.einsum("mck,mk->mc", hmat, n), p=p, q=q, n=n,
                below=below, gap=np.where(below, np.inf, gap), margin=np.where(below, margin, np.inf), depth=np.where(below, depth, 0.0))


def oracle_hfield(O, precision, hsize, data, hpos, hmat, spos, radius):
    """oracle_hfield_sphere of the f32 / f64 oracle library per sphere: (flag[M], dist[M], pos[M, 3], nrm[M, 3]) as float64"""
    lib = O._load(precision)
    real = np.float32 if precision == "f32" else np.float64
    hs, dat = np.ascontiguousarray(hsize, np.float32), np.ascontiguousarray(data, np.float32)
    nrow, ncol = dat.shape
    hp, hm, sp, rd = (np.ascontiguousarray(np.asarray(x, np.float32), dtype=real) for x in (hpos, hmat, spos, radius))
    M = len(sp)
    flag, out, nrm = np.zeros(M, int), np.zeros((M, 4), real), np.zeros((M, 3), real)
    for i in range(M):
        flag[i] = lib.oracle_hfield_sphere(hp[i].ctypes.data, hm[i].ctypes.data, hs.ctypes.data, nrow, ncol, dat.ctypes.data,
                                           sp[i].ctypes.data, rd[i:i + 1].ctypes.data, out[i].ctypes.data, nrm[i].ctypes.data)
    return flag, out[:, 0].astype(np.float64), out[:, 1:4].astype(np.float64), nrm.astype(np.float64)


# ---------------------------------------------------------------- fields and placements
def field(name):
    """(hsize[4] float32, data[nrow, ncol] float32).  Every field but the shipped one has sx != sy, grid lines on binary
    fractions (dx, dy and every x, y of a grid line exact in fp32) and heights on multiples of 1 / 64 of a binary sz: vertices,
    edge midpoints and r = cell / 2 are exact fp32 numbers there."""
    if name == "shipped":
        a = np.load(os.path.join(ASSETS, "go2_rough.npz"), allow_pickle=True)
        nrow, ncol = int(a["hfield_nrow"][0]), int(a["hfield_ncol"][0])
        return a["hfield_size"][0].astype(np.float32), a["hfield_data"].astype(np.float32).reshape(nrow, ncol)
    rng = np.random.default_rng([7, FIELDS.index(name)])
    nrow, ncol, sx, sy, sz = {"f3x3": (3, 3, 1.0, 0.5, 0.25), "f3x7": (3, 7, 0.75, 0.5, 0.25), "f7x3": (7, 3, 0.5, 0.75, 0.25),
                              "steep9": (9, 9, 1.0, 0.5, 1.0), "flat": (5, 9, 1.0, 0.25, 0.5)}[name]
    data = rng.integers(0, 65, size=(nrow, ncol)) / 64.0 if name != "flat" else np.full((nrow, ncol), 0.375)
    return np.array([sx, sy, sz, 0.125], np.float32), data.astype(np.float32)


def cell_of(hsize, data):
    """the host's cell (check_hfield, fp32): spheres may be at most this wide"""
    nrow, ncol = data.shape
    return min(np.float32(2) * hsize[0] / np.float32(ncol - 1), np.float32(2) * hsize[1] / np.float32(nrow - 1))


def placements(name, seed=7):
    """Centres in the FIELD frame, radii and the placement of each, fp32, a multiple of NPAIR = 4 of them (a wave each four):
       1 random, reference dist in (-r, +0.5 r)              5 in the first / last cell of an axis (above and below)
       2 on grid lines and grid vertices, above (ties)       6 on the border p.x = +-sx, p.y = +-sy exactly
       3 exactly on the surface: vertices, edge midpoints    7 one nextafter outside the border
       4 below the surface                                   8 the 81 waves whose four pairs take the states (0, 1, 2) in every
                                                               arrangement (16 of them: no pair searches)
    every fourth of placements 1, 2, 4 and 5 has r = cell / 2 exactly; the others 0.2 .. 0.5 cell (the shipped field: the foot's
    0.023 on every second)."""
    hsize, data = field(name)
    nrow, ncol = data.shape
    sx, sy, sz = (float(v) for v in hsize[:3])
    dx, dy = 2 * sx / (ncol - 1), 2 * sy / (nrow - 1)
    cell = float(cell_of(hsize, data))
    rng = np.random.default_rng([seed, FIELDS.index(name)])
    P, R, T = [], [], []

    def radii(m):
        r = rng.uniform(0.2, 0.5, m) * cell
        if name == "shipped":
            r[1::2] = 0.023
        r[::4] = 0.5 * cell
        return r

    def zsurf(x, y):
        return surface_under(hsize, data, np.asarray(x, np.float64), np.asarray(y, np.float64))[0]

    def add(x, y, z, r, tag):
        P.append(np.stack([x, y, z], 1)); R.append(np.asarray(r, np.float64)); T.append(np.full(len(x), tag))

    def above(x, y, r, lo=0.02, hi=1.5):
        slope = np.sqrt(1 + sum(g * g for g in surface_under(hsize, data, x, y)[1:3]))
        return zsurf(x, y) + rng.uniform(lo, hi, len(x)) * r * slope

    # 1: random, kept where the reference says dist in (-r, 0.5 r)
    m = 512
    x, y, r = rng.uniform(-sx, sx, m), rng.uniform(-sy, sy, m), radii(m)
    c = np.stack([x, y, above(x, y, r)], 1).astype(np.float32)
    ref = ref_hfield(hsize, data, np.zeros((m, 3)), np.tile(np.eye(3), (m, 1, 1)), c, r.astype(np.float32))
    ok = np.nonzero(~ref["below"] & (ref["dist"] > -r) & (ref["dist"] < 0.5 * r))[0][:128]
    assert len(ok) == 128, (name, len(ok))
    add(c[ok, 0], c[ok, 1], c[ok, 2], r[ok], P_RANDOM)
    # 2: on grid lines (x, or y) and on vertices (both), a little above the surface
    m = 48
    gx_, gy_ = -sx + dx * rng.integers(0, ncol, m), -sy + dy * rng.integers(0, nrow, m)
    x = np.where(np.arange(m) % 3 != 1, gx_, rng.uniform(-sx, sx, m))
    y = np.where(np.arange(m) % 3 != 0, gy_, rng.uniform(-sy, sy, m))
    r = radii(m)
    add(x, y, above(x, y, r, 0.1, 0.9), r, P_GRID)
    # 3: exactly on the surface: vertices, and midpoints of x-edges, y-edges and diagonals
    m = 24
    ci, ri, kind = rng.integers(0, ncol - 1, m), rng.integers(0, nrow - 1, m), np.arange(m) % 4
    ex, ey = np.array([0, 1, 0, 1])[kind], np.array([0, 0, 1, 1])[kind]           # vertex, x-edge, y-edge, diagonal
    z0 = data[ri, ci].astype(np.float64) * sz
    z1 = data[ri + ey, ci + ex].astype(np.float64) * sz
    x, y, z = (v.astype(np.float32) for v in (-sx + dx * (ci + 0.5 * ex), -sy + dy * (ri + 0.5 * ey), 0.5 * (z0 + z1)))
    zs = zsurf(x, y)                                         # (the shipped field's grid is not exact in fp32: the first fp32 at or
    z = np.where(np.isin(kind, (0,)) & (z >= zs), z, zs.astype(np.float32))      #  above the surface over the rounded x, y)
    z = np.where(z < zs, np.nextafter(z, np.float32(np.inf)), z)
    add(x, y, z, radii(m), P_SURFACE)
    # 4: below the surface
    m = 48
    x, y, r = rng.uniform(-sx, sx, m), rng.uniform(-sy, sy, m), radii(m)
    add(x, y, zsurf(x, y) - rng.uniform(0.02, 2.0, m) * r, r, P_BELOW)
    # 5: the first and last cell of each axis, above and below
    m = 48
    x, y, r = rng.uniform(-sx, sx, m), rng.uniform(-sy, sy, m), radii(m)
    k = np.arange(m) % 4
    x = np.where(k == 0, -sx + dx * rng.uniform(0, 1, m), np.where(k == 1, sx - dx * rng.uniform(0, 1, m), x))
    y = np.where(k == 2, -sy + dy * rng.uniform(0, 1, m), np.where(k == 3, sy - dy * rng.uniform(0, 1, m), y))
    z = np.where(np.arange(m) % 8 < 6, above(x, y, r, 0.05, 0.9), zsurf(x, y) - rng.uniform(0.05, 1.0, m) * r)
    add(x, y, z, r, P_EDGE_CELL)
    # 6, 7: exactly on the border and one nextafter outside it
    m = 16
    for tag in (P_BORDER, P_OUTSIDE):
        x, y, r = rng.uniform(-sx, sx, m), rng.uniform(-sy, sy, m), rng.uniform(0.2, 0.5, m) * cell
        k = np.arange(m) % 4
        x = np.where(k == 0, -sx, np.where(k == 1, sx, x)); y = np.where(k == 2, -sy, np.where(k == 3, sy, y))
        z = np.where(np.arange(m) % 8 < 7, zsurf(x, y) + 0.5 * r, zsurf(x, y) - 0.5 * r)      # (below, on a cell edge: left out of dist)
        if tag == P_OUTSIDE:
            out = lambda v, s: np.nextafter(np.float32(v), np.float32(s * np.inf)).astype(np.float64)
            x = np.where(k == 0, out(-sx, -1), np.where(k == 1, out(sx, 1), x)); y = np.where(k == 2, out(-sy, -1), np.where(k == 3, out(sy, 1), y))
        add(x, y, z, r, tag)
    # 8: every arrangement of the states (0 outside, 1 below, 2 above) over the four pairs of a wave
    st = np.array([[(w // 3 ** i) % 3 for i in range(4)] for w in range(81)]).ravel()
    m = len(st)
    x, y, r = rng.uniform(-sx, sx, m), rng.uniform(-sy, sy, m), rng.uniform(0.2, 0.5, m) * cell
    z = np.where(st == 1, zsurf(x, y) - rng.uniform(0.1, 1.0, m) * r, zsurf(x, y) + rng.uniform(0.1, 0.9, m) * r)
    x = np.where(st == 0, 1.5 * sx, x)
    add(x, y, z, r, P_MIXED)
    P, R, T = np.concatenate(P).astype(np.float32), np.concatenate(R).astype(np.float32), np.concatenate(T)
    assert len(P) % 4 == 0
    return P, R, T, st


def pose(name, which, m):
    """(hpos[m, 3], hmat[m, 3, 3]) float32: the identity, or one rotation about a tilted axis and a shift"""
    if which == "identity":
        return np.zeros((m, 3), np.float32), np.tile(np.eye(3, dtype=np.float32), (m, 1, 1))
    rng = np.random.default_rng([11, FIELDS.index(name)])
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    ang = 0.7
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    return np.tile(rng.uniform(-0.5, 0.5, 3).astype(np.float32), (m, 1)), np.tile(Rm.astype(np.float32), (m, 1, 1))


_CASES = {}


def case(name, which):
    """Inputs of one (field, pose), read-only and cached: hsize, data, hpos, hmat, spos (world), radius, place, states (of the
    mixed waves), and ref = ref_hfield of them."""
    key = (name, which)
    if key not in _CASES:
        hsize, data = field(name)
        P, R, T, st = placements(name)
        hpos, hmat = pose(name, which, len(P))
        spos = (hpos.astype(np.float64) + np.einsum("mck,mk->mc", hmat.astype(np.float64), P.astype(np.float64))).astype(np.float32)
        c = dict(hsize=hsize, data=data, hpos=hpos, hmat=hmat, spos=spos, radius=R, place=T, states=st, local=P)
        c["ref"] = ref_hfield(hsize, data, hpos, hmat, spos, R)
        for v in [v for v in c.values() if isinstance(v, np.ndarray)] + list(c["ref"].values()):
            v.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def checked_sets(c):
    """(touch, dist_ok, geom_ok) of a case: the sphere touches (reference dist < 0, inside the field); dist is compared there
    except below the surface within EDGE_MIN of a cell edge or the diagonal -- unless the centre is less than 1e-6 m deep: across
    an edge the construction jumps from -r - depth / |(gx, gy, 1)| of one facet to the other's, by less than depth, so there the
    jump is below the rule's floor and the input stays in (the centres placed on the surface, once rotated and rounded).  pos / nrm
    are compared where moreover the input is away from the edges, the runner-up is more than GAP_MIN away and the centre is not on
    the surface itself (placement 3: the normal of a zero vector)."""
    ref = c["ref"]
    touch = ref["flag"] & (ref["dist"] < 0)
    dist_ok = touch & ((ref["margin"] > EDGE_MIN) | (ref["depth"] < 1e-6))
    geom_ok = dist_ok & (ref["margin"] > EDGE_MIN) & (ref["gap"] > GAP_MIN) & (c["place"] != P_SURFACE)
    return touch, dist_ok, geom_ok


# ---------------------------------------------------------------- CPU tests
def test_hfield_unit_compiles_exports_and_goes_stale(monkeypatch):
    path = DH.build(unit="hfield")
    assert os.path.exists(path) and os.path.dirname(path) == DH.BUILD_DIR and path != DH.build(unit="primitives")
    L = DH.hf_lib()
    for sym in DH.HF_SYMBOLS:
        getattr(L, sym)
    assert DH.hf_npair() == 4 and L.rsr_hf_triangle(0, None, None) == -1
    assert L.rsr_hf_contact(0, *[None] * 14) == -1 and L.rsr_hf_scan(0, *[None] * 11) == -1
    # stale against its own source and against any csrc header, as the primitives unit; not against the other unit's source
    assert not DH._stale("hfield")
    hdr = [h for h in DH._headers() if h.endswith("rsr_device.hpp")]
    assert len(hdr) == 1
    real = os.path.getmtime
    for f, want in ((DH.UNITS["hfield"].src, True), (hdr[0], True), (DH.UNITS["primitives"].src, False)):
        with monkeypatch.context() as mp:                      # (a newer time stamp on f, without touching the file)
            mp.setattr(DH.os.path, "getmtime", lambda x, f=f: real(x) + (1e6 if os.path.samefile(x, f) else 0.0))
            assert DH._stale("hfield") == want, f
    assert not DH._stale("hfield")
    assert DH.UNITS["hfield"].env == "RSR_HFIELD_LIB" and DH.UNITS["primitives"].env == "RSR_PRIM_LIB"
    # the build without fma contraction (the bit-identity test's): the same source, the product's flags plus that one
    u = DH.UNITS["hfield_strict"]
    assert u.src == DH.UNITS["hfield"].src and u.flags == ["-ffp-contract=off"] and u.env == "RSR_HFIELD_STRICT_LIB"
    assert DH.UNITS["hfield"].flags == [] and DH.UNITS["primitives"].flags == []
    strict = DH.build(unit="hfield_strict")
    assert os.path.exists(strict) and strict != path and DH.hf_lib(strict=True).rsr_hf_npair() == 4


def test_closest_tri_reference_against_dense_samples():
    rng = np.random.default_rng(0)
    a, b, c, p = (rng.normal(size=(64, 3)) for _ in range(4))
    q = closest_tri(p, a, b, c)
    u = rng.uniform(size=(20000, 2)); u = np.where((u.sum(1) > 1)[:, None], 1 - u, u)
    S = a[:, None] + u[None, :, :1] * (b - a)[:, None] + u[None, :, 1:] * (c - a)[:, None]
    dmin = np.linalg.norm(S - p[:, None], axis=2).min(1)
    d = np.linalg.norm(q - p, axis=1)
    assert (d <= dmin + 1e-12).all() and (dmin - d < 0.05).all()
    n = np.cross(b - a, c - a)
    assert np.abs(np.einsum("nk,nk->n", q - a, n)).max() < 1e-12          # on the plane (and inside: d <= every sample's)


def test_placements_cover_what_they_claim():
    for name in FIELDS:
        c = case(name, "identity")
        hsize, data, ref, T = c["hsize"], c["data"], c["ref"], c["place"]
        assert hsize[0] != hsize[1] or name == "shipped"
        r = c["radius"]
        cell = cell_of(hsize, data)
        assert (2 * r <= cell).all() and (2 * r == cell).sum() >= 64, name
        d1 = ref["dist"][T == P_RANDOM]
        assert (~ref["below"][T == P_RANDOM]).all() and (d1 > -r[T == P_RANDOM]).all() and (d1 < 0.5 * r[T == P_RANDOM]).all()
        assert ref["below"][T == P_BELOW].all() and ref["flag"][T == P_BORDER].all() and not ref["flag"][T == P_OUTSIDE].any()
        if name != "shipped":                                # exact fields: the centres of placement 3 lie on the surface exactly
            s = T == P_SURFACE
            assert (np.abs(ref["dist"][s] + r[s]) == 0).all(), name
            if name != "flat":
                assert (ref["gap"][T == P_GRID] < np.inf).all()
        # mixed waves: the reference sees the states they were built for
        st = np.where(~ref["flag"], 0, np.where(ref["below"], 1, 2))[T == P_MIXED]
        assert (st == c["states"]).all() and len(st) == 4 * 81
        assert (st.reshape(81, 4) == [0, 0, 0, 2]).all(1).any() and ((st.reshape(81, 4) != 2).all(1).sum() == 16)
        touch, dist_ok, geom_ok = checked_sets(c)
        print(name, "spheres %d touching %d left out of dist %d, of pos / nrm %d" % (len(T), touch.sum(), (touch & ~dist_ok).sum(), (dist_ok & ~geom_ok).sum()))


def test_reference_agrees_with_the_f64_oracle(oracle_mod):
    """See the module docstring.  Also the caps the GPU module asserts, here for the f64 oracle against the reference: at most 2 %
    of the touching inputs left out of the dist check, at most 5 % of the random placements out of the pos / nrm check."""
    total = touching = 0
    for name in FIELDS:
        for which in POSES:
            c = case(name, which)
            ref = c["ref"]
            flag, dist, pos, nrm = oracle_hfield(oracle_mod, "f64", c["hsize"], c["data"], c["hpos"], c["hmat"], c["spos"], c["radius"])
            touch, dist_ok, geom_ok = checked_sets(c)
            total, touching = total + len(flag), touching + int(touch.sum())
            if which == "identity":                            # (moved: a centre built on the border is no longer exactly on it)
                assert (flag == ref["flag"]).all(), name
            sure = np.abs(np.abs(ref["p"][:, :2]) - c["hsize"][:2]).min(1) > 1e-5
            assert (flag == ref["flag"])[sure].all(), (name, which)
            e = np.abs(dist - ref["dist"])
            assert e[dist_ok & (flag == 1)].max() < 1e-12, (name, which, e[dist_ok].max())
            # not touching: the 2 x 2 window may miss the closest facet, never find a closer one
            both = ref["flag"] & (flag == 1)
            assert (dist[both & ~ref["below"]] >= ref["dist"][both & ~ref["below"]] - 1e-12).all()
            g = geom_ok & (flag == 1)
            assert np.abs(pos - ref["pos"])[g].max() < 1e-9 and np.abs(nrm - ref["nrm"])[g].max() < 1e-9, (name, which)
            assert (touch & ~dist_ok).sum() <= 0.02 * touch.sum(), (name, which)
            rnd = c["place"] == P_RANDOM
            assert (rnd & touch & ~geom_ok).sum() <= 0.05 * rnd.sum(), (name, which, (rnd & touch & ~geom_ok).sum())
    print("spheres", total, "touching", touching)
