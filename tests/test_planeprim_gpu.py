"""Plane-sphere, plane-capsule and plane-cylinder contacts of the Footstand kernels (the PAIR_PLANE_SPHERE branch and the
Dims::CAPS block of collision<C>, the capsule frame of make_constraint and of contact_forces()) and the sphere branch of the
flat-terrain Go2 kernels, on the directed states of tests/golden/planeprim_states.npz: one Physics.set_state launch per scene, then
Physics.contacts() against (a) the f64 oracle per pair, set-matched, and (b) the numpy fp64 reference of tests/planeprim_ref.py
point by point in the narrow phase's order; then the frame through (c) the rows of Physics.inverse and (d) the contact forces.
Every exclusion is decided by the references (tests/test_planeprim.py rates them), never by the kernel.

Tie classes (cylinder aligned; exact branch): the axis is on the normal to rounding, every rim point is as low as the others and
the direction of the first one is rounding noise, so the f32 oracle, the f64 oracle and the kernel each put the three points
elsewhere on the rim.  Those pairs are held to what does not depend on the direction, see (b)."""
import numpy as np
import pytest

import planeprim_cases as PC
from physics_support import (contact_order_check, inverse_ref, keep, make, oracle_pass, ref_wrench, rel, rule, wrench_on_root)
from physics_support import npyr as npyr_of
from test_planeprim import SCENES, load_scene, pair_tie_class

TOL, TOL_N = 2e-5, 1e-4          # the floors of test_physics_contacts_view: dist / pos, normal
EPS32 = 2.0 ** -24
QVEL_SCALE = 0.2


_RUNS = {}


@pytest.fixture(scope="module", params=list(SCENES))
def run(request, oracle_mod):
    return _run(oracle_mod, request.param)


@pytest.fixture(scope="module")
def footstand_run(oracle_mod):
    return _run(oracle_mod, "footstand")


def _run(oracle_mod, name):
    """the scene's references plus the kernel's contacts per state and pair (one launch per scene, shared by the module's tests):
    S["hip"][e] = by_pair(...), S["hip_seq"], S["ncon"], S["dropped"]; S["phys"] / S["env"] for the tests that launch again;
    S["tied"][e]: the pairs of state e that are ties by the two oracles or of a declared tie class"""
    if name not in _RUNS:
        _RUNS[name] = _launch(oracle_mod, name)
    return _RUNS[name]


def _launch(oracle_mod, name):
    import torch
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.physics import Physics
    S = load_scene(oracle_mod, name)
    n = len(S["qpos"])
    envdef, E, _, _ = make(S["name"], n, False)
    assert E.dims.ncon_max == S["cap"] and bytes(E.blob) == bytes(S["blob"])
    E.reset(prng.split(prng.PRNGKey(2), n))
    phys = Physics(E)
    phys.set_state(qpos=S["qpos"], qvel=np.zeros((n, E.dims.nv), np.float32), ctrl=np.zeros((n, E.dims.nu), np.float32))
    torch.cuda.synchronize()
    c = {k: v.cpu().numpy() for k, v in phys.contacts().items()}
    A = S["arrays"]
    pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(A["pair_geom1"], A["pair_geom2"]))}
    S.update(env=E, envdef=envdef, phys=phys, ncon=c["ncon"], dropped=c["ncon_dropped"], hip=[], hip_seq=[], tied=[])
    for e in range(n):
        nc = int(c["ncon"][e])
        seq = [pair_of[(int(a), int(b))] for a, b in zip(c["geom1"][e, :nc], c["geom2"][e, :nc])]
        S["hip_seq"].append(seq)
        S["hip"].append(PC.by_pair(seq, c["dist"][e, :nc], c["pos"][e, :nc], c["normal"][e, :nc]))
        assert (c["geom1"][e, nc:] == -1).all() and (c["dist"][e, nc:] == 0).all()
        S["tied"].append({p for p in set(S["c64"][e]) | set(S["c32"][e])
                          if PC.is_tie(S["c32"][e].get(p), S["c64"][e].get(p)) or pair_tie_class(S, e, p)})
    return S


def _expected_sequence(c64, cap):
    """(pair per kept contact in pair order, pairs that are kept whole) of the f64 oracle under the capacity"""
    seq = [p for p in sorted(c64) for _ in c64[p][0]]
    kept = seq[:cap]
    return kept, {p for p in c64 if kept.count(p) == len(c64[p][0])}


def _class(r):
    return (PC.classes_of(r) or ["(no class)"])[0]


@pytest.mark.gpu
def test_oracle_parity(run):
    """(a) ncon, ncon_dropped and the (geom1, geom2) sequence of every state without a tie equal the f64 oracle's under the capacity;
    then dist, pos and normal of every kept pair that is no tie and of no declared tie class, set-matched: p99 <= 1e-5 or <= 3 x the
    f32 oracle's p99, every contact within max(2e-5, 20 x the f32 oracle's max) (normal: max(1e-4, ...)).  A count that differs on
    such a pair fails.  Prints p99 / max per class next to the f32 oracle's."""
    S = run
    err = {k: [] for k in ("dist", "pos", "normal")}
    spread = {k: [] for k in ("dist", "pos", "normal")}
    klass, fails, whole_total = [], [], 0
    for e, (c64, c32, hip, res) in enumerate(zip(S["c64"], S["c32"], S["hip"], S["res"])):
        ties = {p for p in set(c64) | set(c32) if PC.is_tie(c32.get(p), c64.get(p))}
        kept, whole = _expected_sequence(c64, S["cap"])
        whole_total += sum(len(c64[p][0]) for p in whole)
        if not ties:
            if S["ncon"][e] != min(S["total"][e], S["cap"]) or S["dropped"][e] != S["total"][e] - min(S["total"][e], S["cap"]):
                fails.append(f"state {e}: ncon {S['ncon'][e]} dropped {S['dropped'][e]}, oracle {S['total'][e]}")
            if S["hip_seq"][e] != kept:
                fails.append(f"state {e}: pair sequence {S['hip_seq'][e]} != {kept}")
        for p in whole - S["tied"][e]:
            d64, p64, n64 = c64[p]
            if p not in hip or len(hip[p][0]) != len(d64):
                fails.append(f"state {e} pair {p}: {len(hip[p][0]) if p in hip else 0} points, oracle {len(d64)}")
                continue
            for src, (d, x, nrm) in ((err, hip[p]), (spread, c32[p])):
                perm, _ = PC.match_sets(p64, x)
                src["dist"] += list(np.abs(d[perm] - d64)); src["pos"] += list(np.abs(x[perm] - p64).max(1))
                src["normal"] += [np.abs(nrm - n64).max()] * len(d64)
            klass += [_class(res[p])] * len(d64)
    klass = np.array(klass)
    for k in err:
        a, s = np.array(err[k]), np.array(spread[k])
        p99, sp99 = np.quantile(a, 0.99), np.quantile(s, 0.99)
        print(f"{S['name']} {k:6s} all ({len(a)} contacts): p99 {p99:.2e} max {a.max():.2e}; f32 oracle p99 {sp99:.2e} max {s.max():.2e}")
        for kc in sorted(set(klass)):
            m = klass == kc
            print(f"{S['name']} {k:6s} {kc:26s} ({m.sum():5d}): p99 {np.quantile(a[m], 0.99):.2e} max {a[m].max():.2e}; "
                  f"f32 oracle p99 {np.quantile(s[m], 0.99):.2e} max {s[m].max():.2e}")
        if not (p99 <= 1e-5 or p99 <= 3 * sp99):
            fails.append(f"{k}: p99 {p99:.2e} (f32 oracle {sp99:.2e})")
        cap = max(TOL_N if k == "normal" else TOL, 20 * s.max())
        if not (a <= cap).all():
            fails.append(f"{k}: {(a > cap).sum()} contacts beyond {cap:.1e}, max {a.max():.2e}")
    assert len(klass) > 0.9 * whole_total
    assert not fails, fails[:20]


def _rate_tie_class(r, dist, pos, nrm):
    """what holds of an aligned cylinder whatever the rim direction; None if it all does"""
    if not (np.isfinite(dist).all() and np.isfinite(pos).all() and np.isfinite(nrm).all()):
        return "not finite"
    if len(dist) != 3:
        return f"{len(dist)} points"
    if abs(dist[0] - r["dist"][0]) > TOL:
        return f"dist[0] {dist[0]} against {r['dist'][0]}"
    k = r["axis"] / np.linalg.norm(r["axis"])
    surface = pos + 0.5 * np.outer(dist, nrm)
    for i, s in enumerate(surface):
        off = [(abs(np.linalg.norm((s - c) - k * ((s - c) @ k)) - r["radius"]), abs((s - c) @ k)) for c in (r["facing"], r["other"])]
        if min(max(o) for o in off) > TOL:
            return f"point {i} is on no rim circle (off by {off})"
        if abs((s - r["point"]) @ r["normal"] - dist[i]) > TOL:
            return f"point {i}: dist is not its height"
    chord = np.linalg.norm(surface[0] - surface[2])
    if abs(chord - np.sqrt(3.0) * r["radius"]) > 2 * TOL:
        return f"points 0 and 2 are not 120 degrees apart (chord {chord})"
    return None


@pytest.mark.gpu
def test_geometry_against_numpy_reference(run):
    """(b) every pair the kernel reports whole against the numpy reference on the f64 oracle's geom poses, point by point in the
    narrow phase's order (capsule: +axis end first; cylinder: the deepest rim point, then -120 and +120 degrees or the other disk),
    ties by the oracles included: the same pairs and counts, normal within 1e-4, dist within 2e-5, pos within 2e-5 for spheres and
    capsules and within 2e-5 + r 8 eps / len for cylinders.  The second term is the rim direction's own conditioning: it is the
    normalised vector n - (n.a) a / (a.a) of length len = sin(angle between axis and normal); float32 kinematics (the trunk's
    matrix from its quaternion, one hinge, the geom's fixed rotation: three products of matrices with entries <= 1) leave each
    entry of the axis within about 8 eps (eps = 2^-24), so the direction within 8 eps / len and the rim point within r times that:
    3e-8 at len 1, 2.8e-6 at a tilt of 0.01, 2.3e-3 at 1.2e-5.  dist does not take part in it (the height is stationary in the
    direction at the lowest point).  Pairs of the declared tie classes: dist[0] to 2e-5, every pos + n dist / 2 on a rim circle of
    the cylinder to 2e-5 with its height as dist, points 0 and 2 a chord of r sqrt(3) apart, three finite points."""
    S = run
    A = S["arrays"]
    size = np.asarray(A["geom_size"], np.float32).astype(float)
    fails, checked, tie_checked, worst = [], 0, 0, {}
    for e, (c64, hip, res) in enumerate(zip(S["c64"], S["hip"], S["res"])):
        _, whole = _expected_sequence(c64, S["cap"])
        ref_pairs = {p for p, r in res.items() if r["touching"].any()}
        if S["total"][e] <= S["cap"] and set(hip) != ref_pairs:
            fails.append(f"state {e}: pairs {sorted(hip)} != {sorted(ref_pairs)}")
            continue
        for p in set(hip) & whole:
            dist, pos, nrm = hip[p]
            r = res[p]
            if pair_tie_class(S, e, p):
                tie_checked += 1
                why = _rate_tie_class(r, dist, pos, nrm)
            else:
                checked += 1
                rd, rp, rn = PC.contacts_of(r)
                tol_pos = TOL + (size[int(A["pair_geom2"][p]), 0] * 8 * EPS32 / r["len"] if r["kind"] == "cylinder" else 0.0)
                why = None
                if len(dist) != len(rd):
                    why = f"{len(dist)} points, reference {len(rd)}"
                elif np.abs(nrm - rn).max() > TOL_N:
                    why = "normal"
                elif np.abs(dist - rd).max() > TOL:
                    why = f"dist off by {np.abs(dist - rd).max():.2e}"
                elif np.abs(pos - rp).max() > tol_pos:
                    why = f"pos off by {np.abs(pos - rp).max():.2e} (bound {tol_pos:.2e})"
                if why is None:
                    w = worst.setdefault(_class(r), [0.0, 0.0])
                    w[0], w[1] = max(w[0], np.abs(dist - rd).max()), max(w[1], np.abs(pos - rp).max())
            if why is not None:
                fails.append(f"state {e} pair {p} ({_class(r)}): {why}")
    for k, (d, x) in sorted(worst.items()):
        print(f"{S['name']} {k:26s} largest difference from the reference: dist {d:.2e} pos {x:.2e}")
    print(f"{S['name']}: {checked} pairs rated point by point, {tie_checked} of the tie classes, {len(fails)} failures")
    assert checked > len(S["qpos"]) and (S["name"] != "footstand" or tie_checked >= 12)
    assert not fails, fails[:20]


def _moving(S):
    """(qvel, ctrl, clean): the seeded velocities of (c) and (d), zero ctrl, and the states without a tie or tie-class pair"""
    n, d = len(S["qpos"]), S["env"].dims
    qvel = (QVEL_SCALE * np.random.default_rng(S["seed"] + 100).normal(size=(n, d.nv))).astype(np.float32)
    return qvel, np.zeros((n, d.nu), np.float32), np.array([not t for t in S["tied"]])


@pytest.mark.gpu
def test_inverse_rows_carry_the_frame(run, oracle_mod):
    """(c) on the same states with a seeded qvel of scale 0.2 (the tangential rows then carry J qvel in aref): inverse_efc_force and
    inverse_qfrc_constraint of Physics.inverse(zeros) against physics_support.inverse_ref on the f64 oracle's rows, under the
    module's rule and keep().  No solve runs in inverse(), so the forces depend on the rows, and those on the tangents, directly.
    States that hold a tie or a pair of a tie class are left out of the comparison (by the references: their contact points, and
    with them their rows, differ between the two oracles); keep()'s 2 % condition is asked of the whole batch."""
    import torch
    S = run
    E, phys = S["env"], S["phys"]
    d, n = E.dims, len(S["qpos"])
    qvel, ctrl, clean = _moving(S)
    phys.set_state(qpos=S["qpos"], qvel=qvel, ctrl=ctrl)
    a = np.zeros((n, d.nv), np.float32)
    phys.inverse(torch.as_tensor(a, device=phys.device).contiguous())
    torch.cuda.synchronize()
    ref = oracle_pass(oracle_mod, E.blob, d, S["qpos"], qvel, ctrl)
    npyr = npyr_of(E)
    hc = phys.inverse_efc_counts.cpu().numpy().astype(int)
    ncon = hc[:, 0] - hc[:, 1] - hc[:, 2] - hc[:, 3]
    assert (ncon % npyr == 0).all() and (ncon >= 0).all()
    kept = keep(S["name"], np.stack([hc[:, 1], hc[:, 2], hc[:, 3], ncon // npyr], 1), ref, npyr) & clean
    print(S["name"], "states compared:", int(kept.sum()), "of", n)
    r64 = [inverse_ref(ref["f64"][e], a[e], np.float64, d.nefc_max) for e in range(n)]
    r32 = [inverse_ref(ref["f32"][e], a[e], np.float32, d.nefc_max) for e in range(n)]
    views = dict(efc_force=phys.inverse_efc_force, qfrc_constraint=phys.inverse_qfrc_constraint)
    fails = []
    for f, t in views.items():
        h = t.cpu().numpy().astype(np.float64)
        s64, s32 = np.stack([r[f] for r in r64]), np.stack([r[f] for r in r32])
        rule(S["name"], f"inverse {f}", rel(h, s64)[kept], rel(s32, s64)[kept], fails)
    assert kept.sum() > 0.8 * n and np.abs(phys.inverse_efc_force.cpu().numpy()).max() > 1.0
    assert not fails, fails


@pytest.mark.gpu
def test_capsule_contact_forces_carry_the_frame(footstand_run, oracle_mod):
    """(d) constraint_forces() + contact_forces()["force"] on the capsule contacts against the wrench from the f64 oracle's rows
    (physics_support.ref_wrench / wrench_on_root, rule and exclusion as in test_contact_wrench_matches_the_oracle_rows), on the
    states with at most 4 contacts, so that the one-iteration Go2 solve is not the subject, and without a tie; other kinds'
    contacts of those states are zeroed on both sides.  keep()'s 2 % condition is asked of that subset.  On the CPU the f32 and
    f64 oracles' row counts agree on every one of those states (0 excluded)."""
    import torch
    S = footstand_run
    E, phys, A = S["env"], S["phys"], S["arrays"]
    d, n, K = E.dims, len(S["qpos"]), E.dims.ncon_max
    qvel, ctrl, clean = _moving(S)
    phys.set_state(qpos=S["qpos"], qvel=qvel, ctrl=ctrl)
    phys.qacc_warmstart.zero_()
    phys.constraint_forces()
    torch.cuda.synchronize()
    ref_all = oracle_pass(oracle_mod, E.blob, d, S["qpos"], qvel, ctrl)
    npyr = npyr_of(E)
    sub = np.nonzero(clean & (np.array(S["total"]) <= 4))[0]
    ref = {p: [ref_all[p][e] for e in sub] for p in ("f32", "f64")}
    hc = phys.efc_counts.cpu().numpy().astype(int)[sub]
    cf = {k: v.cpu().numpy()[sub] for k, v in phys.contact_forces().items()}
    kept = keep(S["name"], np.stack([hc[:, 1], hc[:, 2], hc[:, 3], cf["ncon"]], 1), ref, npyr)
    contact_order_check(S["name"], A, cf["geom1"], cf["geom2"], ref, kept)
    m = len(sub)
    refF, refT = ({p: np.zeros((m, K, 2, 3)) for p in ("f32", "f64")} for _ in range(2))
    hipF, hipT = np.zeros((m, K, 2, 3)), np.zeros((m, K, 2, 3))
    seen = 0
    for i in np.nonzero(kept)[0]:
        capsule = np.zeros(K, bool)
        pr = ref["f64"][i]["contacts"][:, 9].astype(int)
        capsule[:len(pr)] = A["pair_kind"][pr] == PC.PAIR_PLANE_CAPSULE
        for p in ("f32", "f64"):
            F, T, on, root = ref_wrench(ref[p][i], A, npyr, K)
            refF[p][i], refT[p][i] = F * capsule[:, None, None], T * capsule[:, None, None]
        for c, side in zip(*np.nonzero(on & capsule[:, None])):
            sign = 1.0 if side == 1 else -1.0
            hipF[i, c, side] = sign * cf["force"][i, c]
            hipT[i, c, side] = wrench_on_root(cf["pos"][i, c], cf["force"][i, c], cf["torque"][i, c], ref["f64"][i], root[c, side], sign)
            seen += 1
    print(S["name"], "states with at most 4 contacts:", m, "capsule contacts compared:", seen)
    assert seen >= 40 and np.abs(refF["f64"]).max() > 1.0
    fails = []
    rule(S["name"], "capsule contact force", rel(hipF, refF["f64"])[kept], rel(refF["f32"], refF["f64"])[kept], fails)
    rule(S["name"], "capsule contact torque on the root", rel(hipT, refT["f64"])[kept], rel(refT["f32"], refT["f64"])[kept], fails)
    assert not fails, fails
