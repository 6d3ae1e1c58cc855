"""Box-box and plane-box contact manifolds of the tshape and cube kernels (box_box_sat, plane_box_sat and the eight-lanes-per-pair
clip / manifold block of collision<C>) on the directed states of tests/golden/boxbox_states.npz: one Physics.set_state launch per
scene, then Physics.contacts() against (a) the f64 oracle per pair, set-matched, and (b) the numpy fp64 restatement of
tests/boxbox_ref.py.  Every exclusion is decided by the references (tests/test_boxbox_manifold.py rates them), never by the kernel."""
import itertools

import numpy as np
import pytest

import boxbox_cases as BC
import boxbox_ref as BR
from test_boxbox_manifold import load_scene

TOL, TOL_N = 2e-5, 1e-4          # the floors of test_physics_contacts_view: dist / pos, normal


@pytest.fixture(scope="module", params=["tshape", "cube"])
def run(request, oracle_mod):
    """the scene's references plus the kernel's contacts per state and pair: S["hip"][e] = by_pair(...), S["ncon"], S["dropped"]"""
    import torch
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.physics import Physics
    from physics_support import make
    S = load_scene(oracle_mod, request.param, near=False)
    n = len(S["qpos"])
    envdef, E, _, _ = make(S["name"], n, False)
    assert E.dims.ncon_max == S["cap"]
    E.reset(prng.split(prng.PRNGKey(2), n))
    phys = Physics(E)
    phys.set_state(qpos=S["qpos"], qvel=np.zeros((n, E.dims.nv), np.float32), ctrl=np.zeros((n, E.dims.nu), np.float32))
    torch.cuda.synchronize()
    c = {k: v.cpu().numpy() for k, v in phys.contacts().items()}
    A = S["arrays"]
    pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(A["pair_geom1"], A["pair_geom2"]))}
    S["ncon"], S["dropped"], S["hip"], S["hip_seq"] = c["ncon"], c["ncon_dropped"], [], []
    for e in range(n):
        nc = int(c["ncon"][e])
        seq = [pair_of[(int(a), int(b))] for a, b in zip(c["geom1"][e, :nc], c["geom2"][e, :nc])]
        S["hip_seq"].append(seq)
        S["hip"].append(BC.by_pair(seq, c["dist"][e, :nc], c["pos"][e, :nc], c["normal"][e, :nc]))
        assert (c["geom1"][e, nc:] == -1).all() and (c["dist"][e, nc:] == 0).all()
    return S


def _expected_sequence(c64, cap):
    """(pair per kept contact in pair order, pairs that are kept whole) of the f64 oracle under the capacity"""
    seq = [p for p in sorted(c64) for _ in c64[p][0]]
    kept = seq[:cap]
    return kept, {p for p in c64 if kept.count(p) == len(c64[p][0])}


@pytest.mark.gpu
def test_oracle_parity(run):
    """(a) ncon, ncon_dropped and the (geom1, geom2) sequence of every state without a tie equal the f64 oracle's under the capacity;
    then dist, pos and normal of every non-tie pair, set-matched: p99 <= 1e-5 or <= 3 x the f32 oracle's p99, every contact within
    max(2e-5, 20 x the f32 oracle's max) (normal: max(1e-4, ...)).  A count that differs on a non-tie pair fails."""
    S = run
    err = {k: [] for k in ("dist", "pos", "normal")}
    spread = {k: [] for k in ("dist", "pos", "normal")}
    klass, fails = [], []
    for e, (c64, c32, hip, res) in enumerate(zip(S["c64"], S["c32"], S["hip"], S["res"])):
        ties = {p for p in set(c64) | set(c32) if BC.is_tie(c32.get(p), c64.get(p))}
        kept, whole = _expected_sequence(c64, S["cap"])
        if not ties:
            if S["ncon"][e] != min(S["total"][e], S["cap"]) or S["dropped"][e] != S["total"][e] - min(S["total"][e], S["cap"]):
                fails.append(f"state {e}: ncon {S['ncon'][e]} dropped {S['dropped'][e]}, oracle {S['total'][e]}")
            if S["hip_seq"][e] != kept:
                fails.append(f"state {e}: pair sequence {S['hip_seq'][e]} != {kept}")
        for p in whole - ties:
            d64, p64, n64 = c64[p]
            if p not in hip or len(hip[p][0]) != len(d64):
                fails.append(f"state {e} pair {p}: {len(hip[p][0]) if p in hip else 0} points, oracle {len(d64)}")
                continue
            for src, (d, x, nrm) in ((err, hip[p]), (spread, c32[p])):
                perm, _ = BC.match_sets(p64, x)
                src["dist"] += list(np.abs(d[perm] - d64)); src["pos"] += list(np.abs(x[perm] - p64).max(1))
                src["normal"] += [np.abs(nrm - n64).max()] * len(d64)
            klass += [BC.KIND_CODE[res[p]["kind"]] * 10 + len(d64)] * len(d64)
    klass = np.array(klass)
    for k in err:
        a, s = np.array(err[k]), np.array(spread[k])
        p99, sp99 = np.quantile(a, 0.99), np.quantile(s, 0.99)
        print(f"{S['name']} {k:6s} all ({len(a)} contacts): p99 {p99:.2e} max {a.max():.2e}; f32 oracle p99 {sp99:.2e} max {s.max():.2e}")
        for kc in np.unique(klass):
            m = klass == kc
            print(f"{S['name']} {k:6s} {('', 'edge', 'face', 'plane')[kc // 10]} x{kc % 10} ({m.sum()}): p99 {np.quantile(a[m], 0.99):.2e} "
                  f"max {a[m].max():.2e}; f32 oracle p99 {np.quantile(s[m], 0.99):.2e} max {s[m].max():.2e}")
        if not (p99 <= 1e-5 or p99 <= 3 * sp99):
            fails.append(f"{k}: p99 {p99:.2e} (f32 oracle {sp99:.2e})")
        cap = max(TOL_N if k == "normal" else TOL, 20 * s.max())
        if not (a <= cap).all():
            fails.append(f"{k}: {(a > cap).sum()} contacts beyond {cap:.1e}, max {a.max():.2e}")
    assert len(klass) > 0.9 * sum(len(c[p][0]) for c in S["c64"] for p in c if p in _expected_sequence(c, S["cap"])[1])
    assert not fails, fails[:20]


def _assign(points, cand, allowed):
    """can the points be assigned to distinct candidates (each within TOL in dist and pos) so that the index set is allowed?"""
    near = [np.nonzero(np.abs(cand - pt).max(1) <= TOL)[0] for pt in points]
    if any(len(n) == 0 for n in near):
        return "a point is no candidate"
    for combo in itertools.product(*near):
        if len(set(combo)) == len(combo) and frozenset(int(i) for i in combo) in allowed:
            return None
    return f"no allowed selection among {sorted(map(sorted, allowed))} (nearest candidates {[list(n) for n in near]})"


def _rate_boxbox(r, geoms, dist, pos, nrm):
    """the geometric checks of one box-box result against the reference built on branch r; None if they all hold"""
    pa, Ra, sa, pb, Rb, sb = geoms
    if r["kind"] not in ("edge", "face"):
        return "reference has no contact on this axis"
    if np.abs(nrm - r["normal"]).max() > TOL_N:
        return "normal is not this axis"
    if r["kind"] == "edge":
        if len(dist) != 1:
            return "edge contact with more than one point"
        # pos: the midpoint of the two closest edge points; dist: their signed gap
        if np.abs(pos[0] - 0.5 * (r["qa"] + r["qb"])).max() > TOL or abs(dist[0] - (r["qb"] - r["qa"]) @ r["normal"]) > TOL:
            return "edge point"
        return None
    x, y, d = r["poly_x"], r["poly_y"], r["poly_d"]
    # every point projects onto a vertex of the clipped polygon, dist = -depth, pos half-way along the normal
    cand = np.c_[-d, r["o"] + np.outer(x, r["axu"]) + np.outer(y, r["axv"]) - 0.5 * np.outer(d, r["nref"])]
    cand[~r["mask"]] = np.inf
    return _assign(np.c_[dist, pos], cand, BR.selection_outcomes(x, y, r["mask"], tol=TOL))


@pytest.mark.gpu
def test_geometry_against_numpy_reference(run):
    """(b) every pair the kernel reports whole, ties included, against the fp64 restatement on the f64 oracle's geom poses: unit
    normal from geom1 to geom2 that is one of the 15 axes with an overlap of at most the least overlap / 0.95 + 2e-5; edge contacts
    at the midpoint of the closest edge points with their gap as dist; face contacts on distinct vertices of the clipped polygon
    with dist = -depth and pos half-way along the normal; plane-box contacts on box vertices inside the band, the deepest present;
    and the selection by value: the reported set is one the rule can give when a pick within 2e-5 of the winning value may
    replace the winner (so the count equals the reference's wherever that leaves one outcome).  A result on another axis than the
    reference's is rated on that axis if its separating value is within 2e-5 of the winning one."""
    S = run
    A = S["arrays"]
    size = np.asarray(A["geom_size"], np.float32).astype(float)
    fails, checked = [], 0
    for e, (c64, hip, res) in enumerate(zip(S["c64"], S["hip"], S["res"])):
        _, whole = _expected_sequence(c64, S["cap"])
        # the kernel must report exactly the pairs the reference has in contact (margins are clear), up to the capacity
        ref_pairs = {p for p, r in res.items() if r["kind"] in ("edge", "face", "plane")}
        if S["total"][e] <= S["cap"] and set(hip) != ref_pairs:
            fails.append(f"state {e}: pairs {sorted(hip)} != {sorted(ref_pairs)}")
            continue
        for p in set(hip) & whole:
            dist, pos, nrm = hip[p]
            r = res[p]
            checked += 1
            if abs(np.linalg.norm(nrm) - 1) > TOL_N or len(dist) > 4 or not (dist < 0).all():
                fails.append(f"state {e} pair {p}: normal length / count / sign of dist")
                continue
            if r["kind"] == "plane":
                sup = r["support"]
                cand = np.c_[-sup, r["vertices"] + 0.5 * np.outer(sup, r["normal"])]
                cand[~r["mask"]] = np.inf
                why = _assign(np.c_[dist, pos], cand, BR.selection_outcomes(r["x"], r["y"], r["mask"], tol=TOL))
                if why is None and np.abs(nrm - r["normal"]).max() > TOL_N:
                    why = "normal"
                if why is None and abs(dist.min() + r["smax"]) > TOL:
                    why = "deepest vertex absent"
            else:
                g1, g2 = int(A["pair_geom1"][p]), int(A["pair_geom2"][p])
                gp, gm = S["gpos"][e], S["gmat"][e]
                geoms = (gp[g1], gm[g1], size[g1], gp[g2], gm[g2], size[g2])
                if not nrm @ (gp[g2] - gp[g1]) > 0:
                    fails.append(f"state {e} pair {p}: normal does not point from geom1 to geom2")
                    continue
                least = -max(r["sep_face"].max(), np.nanmax(r["sep_edge"]) if not np.isnan(r["sep_edge"]).all() else -np.inf)
                # branches to rate on: the reference's own, and every axis whose overlap is within the bound
                branches = [None]
                branches += [("face", k) for k in range(6) if -r["sep_face"][k] <= least / BR.PREF + TOL]
                branches += [("edge", i, j) for i in range(3) for j in range(3)
                             if not np.isnan(r["sep_edge"][i, j]) and -r["sep_edge"][i, j] <= least / BR.PREF + TOL]
                why = None
                for br in branches:
                    if br is not None:
                        # another axis than the reference's is admissible only within tolerance of the deciding values
                        val = r["sep_face"][br[1]] if br[0] == "face" else r["sep_edge"][br[1], br[2]]
                        best_face, best_edge = r["sep_face"].max(), r.get("best_edge", -np.inf)
                        if br[0] == "face" and not (val >= best_face - TOL and (r["kind"] != "edge" or best_edge <= BR.PREF * best_face + BR.PAD + TOL)):
                            continue
                        if br[0] == "edge" and not (val >= best_edge - TOL and val >= BR.PREF * best_face + BR.PAD - TOL):
                            continue
                    why = _rate_boxbox(r if br is None else BR.box_box(*geoms, force=br), geoms, dist, pos, nrm)
                    if why is None:
                        break
            if why is not None:
                fails.append(f"state {e} pair {p} ({r['kind']}, {len(dist)} points): {why}")
    print(f"{S['name']}: {checked} pairs rated, {len(fails)} failures")
    assert checked > 1000 and not fails, fails[:20]


@pytest.mark.gpu
def test_branch_census_of_existing_states(run, oracle_mod):
    """(c) the branches that the states of test_physics_contacts_view reach, next to this fixture's, counted the same way over every
    pair in contact (fp64 labels).  Printed; the figures are in DESIGN.md."""
    import torch
    from rsr_mjx_amd import prng
    from physics_support import make, random_states
    S = run
    n = 256
    envdef, E, _, _ = make(S["name"], n, False)
    E.reset(prng.split(prng.PRNGKey(2), n))
    qpos, _, _ = random_states(envdef, S["name"], n, 12)
    torch.cuda.synchronize()
    o64 = oracle_mod.Oracle(E.blob, "f64")
    old = [BC.pair_results(S["arrays"], *BC.oracle_contacts(o64, q, E.dims.nv, E.dims.nu)[2:]) for q in qpos]
    rows = {}
    for name, states in (("contacts_view", old), ("fixture", S["res"])):
        lab = [BC.labels(r) for res in states for r in res.values() if r["kind"] in ("edge", "face", "plane")]
        cen = BC.census(lab)
        cen["states with >= 9 pending pairs"] = sum(sum(BC.is_pending(r) for r in res.values()) >= 9 for res in states)
        cen["states"] = len(states)
        rows[name] = cen
    for k in rows["fixture"]:
        print(f"{S['name']:7s} {k:32s} contacts_view {rows['contacts_view'][k]:6d}   fixture {rows['fixture'][k]:6d}")
    # the fixture reaches every class at least as often as the existing states do, and the classes those states never reach
    never = [k for k, v in rows["contacts_view"].items() if v == 0 and k != "clip emptied" and not (S["name"] == "cube" and k.startswith("states with"))]
    assert all(rows["fixture"][k] > 0 for k in never), [k for k in never if rows["fixture"][k] == 0]
    assert len(never) >= 30, never
