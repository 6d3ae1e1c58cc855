"""The height-field narrow phase of rsr_mjx_amd/csrc/rsr_device.hpp -- hfield_place, hfield_search<NPAIR>, hfield_finish and
closest_on_triangle -- called directly (tests/device/hfield.hip: one wave per NPAIR = 4 spheres, in collision()'s own sequence)
and compared with plain fp64 (test_device_hfield.ref_hfield: the closest point over all triangles of a 5 x 5-cell window; not
the oracle's construction, and checked against the oracle on the CPU there).

Inputs (test_device_hfield.placements, seed 7): six fields -- the shipped 256 x 256 one, random 3 x 3, 3 x 7 and 7 x 3 ones, a
steep 9 x 9 one, a flat one; all but the shipped one with sx != sy and with grid lines, heights and r = cell / 2 exact in fp32 --
each with the field at the origin and once rotated and shifted, 652 spheres per field and pose (7824 in all): random centres
with dist in (-r, 0.5 r), centres on grid lines and vertices, exactly on the surface, below it, in the first and last cells, on
the border and one nextafter outside it, and the 81 waves whose four pairs take the states (no contact, below, search) in every
arrangement.

Rule (set before measuring, rule of tests/physics_support.py): p99 <= 1e-5 or <= 3 x the p99 of the spread, every input within
max(1e-4, 20 x the largest spread); the spread is the distance of the F32 ORACLE's hfield_sphere from the same reference on the
same inputs.  dist is checked on every touching input (reference dist < 0) -- it is a minimum distance, 1-Lipschitz in the
centre, so no facet tie can excuse it -- except below the surface within 1e-4 (u, v units) of a cell edge or the diagonal, where
the construction itself jumps (2 of ~488 per case: the two centres put below the border on purpose; cap 2 %, asserted).  pos and
nrm are checked where moreover the runner-up facet is more than 1e-4 m further than the winner (cap: 5 % of the random
placements; on the CPU the f64 oracle against the reference leaves out 5, 1, 2, 4, 3, 5 of 128 for the six fields).

Needle triangles (fp32 area / longest edge^2 < 1e-6) are left out of the closest_on_triangle test: the face region's
barycentric sums cancel there.  No height-field triangle comes near that: its two legs are a cell's sides, so the ratio is
at least 1 / (2 (1 + slope^2)), 0.1 on the steep field.

Measured maxima (MI355X; kernel / f32-oracle spread, both against the fp64 reference; the worse of the two poses):

    field    dist                   pos                    nrm                    tied q
    shipped  1.07e-06 / 1.22e-06    7.54e-07 / 8.61e-07    3.96e-04 / 4.25e-04    2.32e-07 / 2.29e-07
    f3x3     7.36e-08 / 5.87e-08    7.86e-07 / 7.86e-07    6.06e-06 / 6.26e-06    6.93e-08 / 1.78e-07
    f3x7     4.06e-08 / 3.91e-08    9.61e-07 / 9.61e-07    1.48e-05 / 1.48e-05    6.30e-08 / 8.62e-08
    f7x3     6.22e-08 / 6.07e-08    4.46e-07 / 3.38e-07    1.14e-05 / 7.78e-06    5.87e-08 / 1.02e-07
    steep9   1.00e-07 / 1.10e-07    8.35e-07 / 1.50e-06    4.62e-05 / 1.05e-04    8.28e-08 / 9.93e-08
    flat     3.64e-08 / 3.52e-08    2.98e-07 / 2.98e-07    1.45e-05 / 1.45e-05    7.40e-08 / 1.36e-07
    (nrm on the shipped field: the foot's r = 0.023 at |x| up to 10, where an ulp of x is 1e-6 -- the f32 oracle shows the same.)
    closest_on_triangle: distance 1.33e-06 / 1.56e-06, point 1.15e-06 / 1.25e-06; no needle among the 4736 triangles.
    rigid motion: dist 1.33e-06 / 1.55e-06, pos 1.54e-06 / 2.26e-06, nrm 3.09e-04 / 6.89e-04 (the worst field each).
    On the exact fields all 24 centres placed on the surface gave best == 0 and n = (0, 0, 1).

Bit identity of hfield_search with the serial scan (test_search_is_the_serial_scan_bit_for_bit) is asserted on a build of the
unit WITHOUT fma contraction.  Under the product's flags the two kernels are separate compilations of the same C++ and the
compiler forms different fma's in each (even hfield_place's surface height moves by an ulp between them): measured there, of 350 /
358 searching inputs per field, best differs in 56, 56, 93, 70, 70, 0 and q in 62, 81, 108, 79, 70, 14 (shipped, f3x3, f3x7, f7x3,
steep9, flat) with the field at the origin, in up to 348 of 353 once it is rotated (the centre itself then differs by an ulp).
Without contraction every operation rounds as written, in both kernels, and (q, best) match on every one of the 4236 searching
inputs of the six fields and both poses (measured: 0 differ).
"""
import numpy as np
import pytest

import device_harness as DH
from physics_support import rule
from test_device_hfield import (FIELDS, P_BORDER, P_GRID, P_MIXED, P_OUTSIDE, P_RANDOM, P_SURFACE, POSES, case, checked_sets,
                                closest_tri, oracle_hfield)

pytestmark = pytest.mark.gpu

_RUN = {}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _args(c):
    n = len(c["spos"]) // 4
    return (c["hsize"], c["data"], c["hpos"][::4], c["hmat"][::4], c["spos"].reshape(n, 4, 3), c["radius"].reshape(n, 4))


def run(name, which, oracle_mod):
    """(case, kernel outputs flattened to one row per sphere, serial scan, f32 oracle's (flag, dist, pos, nrm)); cached"""
    key = (name, which)
    if key not in _RUN:
        c = case(name, which)
        k = DH.hf_contact(*_args(c))
        s = DH.hf_scan(*_args(c))
        flat = lambda v: v.reshape((-1,) + v.shape[2:])
        k = type(k)(*[flat(v) for v in k])
        s = type(s)(*[flat(v) for v in s])
        o32 = oracle_hfield(oracle_mod, "f32", c["hsize"], c["data"], c["hpos"], c["hmat"], c["spos"], c["radius"])
        _RUN[key] = (c, k, s, o32)
    return _RUN[key]


def _vec_err(a, ref):
    return np.abs(a - ref).max(1) / np.maximum(1.0, np.abs(ref).max(1))


@pytest.mark.parametrize("name", FIELDS)
def test_flag_and_dist_match_fp64(oracle_mod, name):
    """The contact flag on every input whose centre is not within 1e-5 of the border (moved pose) or at all (identity: the border
    itself is a contact, one nextafter outside is none); dist on every touching input under the rule; where the sphere does not
    touch, the 2 x 2 window may miss the closest facet but can never find a closer one; no NaN anywhere."""
    fails = []
    for which in POSES:
        c, k, s, (f32, d32, _, _) = run(name, which, oracle_mod)
        ref = c["ref"]
        for v in (k.dist, k.pos, k.nrm, k.q, k.best):
            assert np.isfinite(v).all(), (name, which)
        sure = np.abs(np.abs(ref["p"][:, :2]) - c["hsize"][:2]).min(1) > 1e-5
        if which == "identity":
            sure[:] = True
            assert (k.flag[c["place"] == P_BORDER] == 1).all() and (k.flag[c["place"] == P_OUTSIDE] == 0).all()
        assert (k.flag == ref["flag"])[sure].all(), (name, which)
        assert ((k.state != 0) == (k.flag == 1)).all()
        touch, dist_ok, _ = checked_sets(c)
        print(name, which, "touching %d, left out %d" % (touch.sum(), (touch & ~dist_ok).sum()))
        assert (touch & ~dist_ok).sum() <= 0.02 * touch.sum()
        sel = dist_ok & (k.flag == 1) & (f32 == 1)
        assert sel.sum() >= 0.95 * touch.sum()
        rule(f"{name}/{which}", "dist", np.abs(k.dist - ref["dist"])[sel], np.abs(d32 - ref["dist"])[sel], fails)
        cap = max(1e-4, 20.0 * float(np.abs(d32 - ref["dist"])[sel].max()))
        above = (k.flag == 1) & ref["flag"] & ~ref["below"] & (k.state == 2)
        assert (k.dist[above] >= ref["dist"][above] - cap).all(), (name, which)
    assert not fails, fails


@pytest.mark.parametrize("name", FIELDS)
def test_pos_and_normal_match_fp64(oracle_mod, name):
    """pos and nrm under the rule where the runner-up facet is more than 1e-4 m away (above) and away from the cell edges (below);
    |nrm| = 1 to 1e-6 and pos = q + n dist / 2 in the field frame on every contact."""
    fails = []
    for which in POSES:
        c, k, s, (f32, _, p32, n32) = run(name, which, oracle_mod)
        ref = c["ref"]
        touch, dist_ok, geom_ok = checked_sets(c)
        rnd = c["place"] == P_RANDOM
        print(name, which, "random placements left out of pos / nrm: %d of %d" % ((rnd & touch & ~geom_ok).sum(), rnd.sum()))
        assert (rnd & touch & ~geom_ok).sum() <= 0.05 * rnd.sum()
        sel = geom_ok & (k.flag == 1) & (f32 == 1)
        rule(f"{name}/{which}", "pos", _vec_err(k.pos, ref["pos"])[sel], _vec_err(p32, ref["pos"])[sel], fails)
        rule(f"{name}/{which}", "nrm", _vec_err(k.nrm, ref["nrm"])[sel], _vec_err(n32, ref["nrm"])[sel], fails)
        hit = k.flag == 1
        assert np.abs(np.linalg.norm(k.nrm.astype(np.float64), axis=1) - 1.0)[hit].max() <= 1e-6, (name, which)
        # the job in the field frame: n is unit, and the reported pos / nrm are hpos + R (q + n dist / 2), R n
        q, dist = k.q.astype(np.float64), k.dist.astype(np.float64)
        n = np.where((k.state == 2)[:, None], np.einsum("mkc,mk->mc", c["hmat"].astype(np.float64), k.nrm.astype(np.float64)), k.n)
        pl = q + n * (0.5 * dist)[:, None]
        pos = c["hpos"] + np.einsum("mck,mk->mc", c["hmat"].astype(np.float64), pl)
        tol = 4 * np.spacing(np.float32(np.abs(pos).max() + 1.0))
        assert np.abs(pos - k.pos)[hit].max() <= tol, (name, which, np.abs(pos - k.pos)[hit].max(), tol)
        searched = hit & (k.state == 2) & (k.best > 0)
        np.testing.assert_allclose(k.dist[searched], np.sqrt(k.best[searched].astype(np.float64)) - c["radius"][searched], atol=1e-6)
    assert not fails, fails


@pytest.mark.parametrize("name", FIELDS)
def test_ties_report_the_shared_point(oracle_mod, name):
    """Centres on grid lines and vertices (several triangles share the closest point) and exactly on the surface: the surface
    point q the kernel reports is the reference's, whichever of the tied triangles it took, under the rule (the f32 oracle's q,
    recovered as pos - nrm dist / 2, as spread); on the exact fields a centre on the surface gives best = 0, n = (0, 0, 1)."""
    fails = []
    for which in POSES:
        c, k, s, (f32, d32, p32, n32) = run(name, which, oracle_mod)
        ref = c["ref"]
        sel = np.isin(c["place"], (P_GRID, P_SURFACE)) & (k.flag == 1) & (f32 == 1) & ~ref["below"] & (k.state == 2)
        # a tie of points, not of facets at different points: the runner-up (a different point) is still 1e-4 m away
        sel &= ref["gap"] > 1e-4
        assert sel.sum() >= 24, (name, which, sel.sum())
        R = c["hmat"].astype(np.float64)
        q32 = np.einsum("mkc,mk->mc", R, p32 - n32 * (0.5 * d32)[:, None] - c["hpos"])
        rule(f"{name}/{which}", "tied q", _vec_err(k.q, ref["q"])[sel], _vec_err(q32, ref["q"])[sel], fails)
        if which == "identity" and name != "shipped":
            on = (c["place"] == P_SURFACE) & (k.state == 2)
            assert on.sum() >= 12
            zero = on & (k.best == 0)
            print(name, "centres on the surface: %d, best == 0 in %d" % (on.sum(), zero.sum()))
            assert (k.best[on] <= 1e-12).all()
            assert (k.nrm[zero] == [0, 0, 1]).all() and (k.dist[zero] == -c["radius"][zero]).all() and zero.sum() >= 6
    assert not fails, fails


def _run_strict(name, which):
    key = (name, which, "strict")
    if key not in _RUN:
        c = case(name, which)
        flat = lambda v: v.reshape((-1,) + v.shape[2:])
        k, s = DH.hf_contact(*_args(c), strict=True), DH.hf_scan(*_args(c), strict=True)
        _RUN[key] = (type(k)(*[flat(v) for v in k]), type(s)(*[flat(v) for v in s]))
    return _RUN[key]


@pytest.mark.parametrize("name", FIELDS)
def test_search_is_the_serial_scan_bit_for_bit(oracle_mod, name):
    """hfield_search's (q, best) against the unit's serial scan (the pair's lane, k = 0..7, strict <) on every input of every field,
    BIT FOR BIT, in the build of the unit without fma contraction (device_harness.UNITS: there every operation rounds as the
    source writes it, in both kernels, so the comparison is one of the source's arithmetic and of the pick -- the arg-min's three
    DPP steps, its first-of-equal-minima rule and the read-back of the winner).  In the product-flags build the two kernels are
    contracted differently and agree to rounding only: there the two distances sqrt(best) must lie within 8 ulp of the centre's
    largest coordinate (the distance is 1-Lipschitz in the centre and the vertices, each a handful of roundings; the POINT is not
    bounded so: where two facets are nearly as close, an ulp in the centre picks the other, 1.8 mm away on the shipped field).  In both builds: pairs in state 0 or 1
    keep the q / best they had, the wave runs the search exactly when one of its pairs is in state 2, and the 81 arrangements of
    states come out as built ("only pair 3 searches" and "no pair searches" among them)."""
    for which in POSES:
        c, kp, sp, _ = run(name, which, oracle_mod)
        ks, ss = _run_strict(name, which)
        w = (ks.state == 2) & (ss.state == 2)
        bad = (_bits(ks.q) != _bits(ss.q)).any(1) | (_bits(ks.best) != _bits(ss.best))
        wp = (kp.state == 2) & (sp.state == 2)
        dq = np.abs(kp.q - sp.q).max(1)
        print(name, which, "searching %d; no contraction: (q, best) differ in %d; product flags: best differs in %d, q in %d (max |dq| %.2e)"
              % (w.sum(), bad[w].sum(), (_bits(kp.best) != _bits(sp.best))[wp].sum(), (_bits(kp.q) != _bits(sp.q)).any(1)[wp].sum(), dq[wp].max()))
        assert (ks.state == ss.state).all() and w.sum() > 300
        assert not bad[w].any(), (name, which, np.nonzero(bad & w)[0][:8], ks.best[bad & w][:4], ss.best[bad & w][:4])
        dd = np.abs(np.sqrt(kp.best.astype(np.float64)) - np.sqrt(sp.best.astype(np.float64)))
        assert (dd <= 8 * np.spacing(np.maximum(np.abs(kp.p).max(1), 1.0).astype(np.float32)))[wp].all(), (name, which, dd[wp].max())
        assert (np.abs(kp.state - sp.state) <= 1).all() and ((kp.state == 0) == (sp.state == 0)).all()
        for k in (ks, kp):
            w, idle = k.state == 2, k.state != 2
            assert (_bits(k.q) == _bits(k.q_pre))[idle].all() and (_bits(k.best) == _bits(k.best_pre))[idle].all()
            assert (k.best[idle] == -7.25).all() and (k.q[k.state == 0] == -7.25).all()
            assert (k.searched.reshape(-1, 4) == (k.state.reshape(-1, 4) == 2).any(1, keepdims=True)).all()
            mixed = k.state[c["place"] == P_MIXED].reshape(81, 4)
            assert (mixed == c["states"].reshape(81, 4)).all()
            assert (k.c0 >= 0)[w].all() and (k.c0 <= c["data"].shape[1] - 3)[w].all() and (k.r0 >= 0)[w].all() and (k.r0 <= c["data"].shape[0] - 3)[w].all()


@pytest.mark.parametrize("name", FIELDS)
def test_rigid_motion_moves_the_answer(oracle_mod, name):
    """The kernel's answer with the field at the origin, rotated and shifted, against its answer for the rotated and shifted field
    and centre: under the rule, with the f32 oracle's same difference as spread.  dist on every touching input, pos / nrm away
    from facet ties."""
    c0, k0, _, o0 = run(name, "identity", oracle_mod)
    c1, k1, _, o1 = run(name, "moved", oracle_mod)
    R, t = c1["hmat"].astype(np.float64), c1["hpos"].astype(np.float64)
    move = lambda pos: t + np.einsum("mck,mk->mc", R, pos)
    rot = lambda n: np.einsum("mck,mk->mc", R, n)
    both = (k0.flag == 1) & (k1.flag == 1) & (o0[0] == 1) & (o1[0] == 1)
    sel = both & checked_sets(c0)[1] & checked_sets(c1)[1]
    geo = both & checked_sets(c0)[2] & checked_sets(c1)[2]
    assert sel.sum() > 400 and geo.sum() > 300
    fails = []
    rule(name, "moved dist", np.abs(k1.dist - k0.dist.astype(np.float64))[sel], np.abs(o1[1] - o0[1])[sel], fails)
    rule(name, "moved pos", _vec_err(k1.pos, move(k0.pos.astype(np.float64)))[geo], _vec_err(o1[2], move(o0[2]))[geo], fails)
    rule(name, "moved nrm", _vec_err(k1.nrm, rot(k0.nrm.astype(np.float64)))[geo], _vec_err(o1[3], rot(o0[3]))[geo], fails)
    assert not fails, fails


def _triangles():
    """4096 random (p, a, b, c) and, per Voronoi region (three vertices, three edges, the face), 64 points placed in it on
    purpose; plus p exactly on a vertex, on an edge (the midpoint of binary-fraction vertices) and in the plane."""
    rng = np.random.default_rng(5)
    n = 4096
    a, b, c = (rng.uniform(-1, 1, size=(n, 3)) for _ in range(3))
    p = rng.uniform(-1.5, 1.5, size=(n, 3))
    region = np.full(n, -1)
    m = 64
    A, B, Cc = (np.round(rng.uniform(-1, 1, size=(7 * m + 3 * m, 3)) * 64) / 64 for _ in range(3))
    nrm = np.cross(B - A, Cc - A)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cen = (A + B + Cc) / 3
    P, Rg = np.zeros_like(A), np.zeros(len(A), int)
    h = rng.uniform(-0.5, 0.5, len(A))[:, None] * nrm
    for g in range(7):
        s = slice(g * m, (g + 1) * m)
        V = [A[s], B[s], Cc[s]]
        if g < 3:                                         # beyond vertex g: against both of its edges (-(e1 + e2), unit e's)
            e1, e2 = V[(g + 1) % 3] - V[g], V[(g + 2) % 3] - V[g]
            away = -(e1 / np.linalg.norm(e1, axis=1, keepdims=True) + e2 / np.linalg.norm(e2, axis=1, keepdims=True))
            P[s] = V[g] + away * rng.uniform(0.1, 0.5, (m, 1)) + h[s]
        elif g < 6:                                       # beyond the middle of edge (g - 3, g - 2), in the plane's outward direction
            e0, e1 = V[g - 3], V[(g - 2) % 3]
            mid = e0 + (e1 - e0) * rng.uniform(0.3, 0.7, (m, 1))
            out = np.cross(e1 - e0, nrm[s]); out *= np.sign(np.einsum("nk,nk->n", out, mid - cen[s]))[:, None]
            P[s] = mid + out / np.linalg.norm(out, axis=1, keepdims=True) * rng.uniform(0.05, 0.5, (m, 1)) + h[s]
        else:                                             # over the face
            w = rng.dirichlet([2, 2, 2], m)
            P[s] = w[:, :1] * V[0] + w[:, 1:2] * V[1] + w[:, 2:] * V[2] + h[s]
        Rg[s] = g
    s = slice(7 * m, 8 * m); P[s] = [A[s], B[s], Cc[s]][1]; Rg[s] = 7                      # exactly on a vertex
    s = slice(8 * m, 9 * m); P[s] = 0.5 * (A[s] + Cc[s]); Rg[s] = 8                        # exactly on an edge
    s = slice(9 * m, 10 * m); w = rng.dirichlet([2, 2, 2], m); Rg[s] = 9                   # in the plane (to fp32 rounding)
    P[s] = w[:, :1] * A[s] + w[:, 1:2] * B[s] + w[:, 2:] * Cc[s]
    return (np.concatenate([p, P]).astype(np.float32), np.concatenate([a, A]).astype(np.float32), np.concatenate([b, B]).astype(np.float32),
            np.concatenate([c, Cc]).astype(np.float32), np.concatenate([region, Rg]))


def _tri32(p, a, b, c):
    """Ericson's region walk in numpy float32 (exact division, no fusion), per input: the spread of the triangle test"""
    f = np.float32
    out = np.zeros_like(p)
    for i in range(len(p)):
        P, A, B, C_ = p[i], a[i], b[i], c[i]
        ab, ac, ap = B - A, C_ - A, P - A
        d1, d2 = f(ab @ ap), f(ac @ ap)
        if d1 <= 0 and d2 <= 0: out[i] = A; continue
        bp = P - B; d3, d4 = f(ab @ bp), f(ac @ bp)
        if d3 >= 0 and d4 <= d3: out[i] = B; continue
        vc = f(d1 * d4) - f(d3 * d2)
        if vc <= 0 and d1 >= 0 and d3 <= 0: out[i] = A + ab * f(d1 / (d1 - d3)); continue
        cp = P - C_; d5, d6 = f(ab @ cp), f(ac @ cp)
        if d6 >= 0 and d5 <= d6: out[i] = C_; continue
        vb = f(d5 * d2) - f(d1 * d6)
        if vb <= 0 and d2 >= 0 and d6 <= 0: out[i] = A + ac * f(d2 / (d2 - d6)); continue
        va = f(d3 * d6) - f(d5 * d4)
        if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0: out[i] = B + (C_ - B) * f((d4 - d3) / ((d4 - d3) + (d5 - d6))); continue
        den = f(1) / (va + vb + vc)
        out[i] = A + ab * f(vb * den) + ac * f(vc * den)
    return out


def test_closest_on_triangle_matches_fp64():
    """Distance |p - q| of the kernel's closest_on_triangle against the fp64 closest point, under the rule, with the same walk in
    numpy float32 as spread; the point itself where the closest point is unique by construction (it always is on one triangle);
    p on a vertex or an edge midpoint comes back exactly.  Needle triangles are left out (module docstring)."""
    p, a, b, c, region = _triangles()
    q = DH.hf_triangle(p, a, b, c)
    assert np.isfinite(q).all()
    ab, ac, bc = (b - a).astype(np.float32), (c - a).astype(np.float32), (c - b).astype(np.float32)
    area = 0.5 * np.linalg.norm(np.cross(ab, ac).astype(np.float32), axis=1)
    edge2 = np.maximum.reduce([(v * v).sum(1) for v in (ab, ac, bc)])
    keep = area / edge2 >= 1e-6
    print("needle triangles left out: %d of %d" % ((~keep).sum(), len(keep)))
    assert (~keep).sum() <= 0.01 * len(keep)
    ref = closest_tri(p, a, b, c)
    d_ref = np.linalg.norm(p - ref, axis=1)
    d_k = np.linalg.norm(p.astype(np.float64) - q, axis=1)
    q32 = _tri32(p, a, b, c)
    d_32 = np.linalg.norm(p.astype(np.float64) - q32, axis=1)
    fails = []
    rule("triangle", "distance", np.abs(d_k - d_ref)[keep], np.abs(d_32 - d_ref)[keep], fails)
    rule("triangle", "point", _vec_err(q, ref)[keep], _vec_err(q32.astype(np.float64), ref)[keep], fails)
    for g in range(10):                                     # (7, 8, 9: p on a vertex, on an edge, in the plane)
        s = (region == g) & keep
        rule("triangle", f"region {g} distance", np.abs(d_k - d_ref)[s], np.abs(d_32 - d_ref)[s], fails)
    # the regions were hit: the fp64 closest point is the vertex / on the edge / strictly inside
    V = [a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)]
    for g in range(3):
        assert (np.linalg.norm(ref - V[g], axis=1)[region == g] < 1e-12).all(), g
    assert (_bits(q) == _bits(b))[region == 7].all(), "p on a vertex"
    assert np.abs(q - p)[region == 8].max() <= 2.0 ** -23, "p on an edge midpoint"
    assert not fails, fails
