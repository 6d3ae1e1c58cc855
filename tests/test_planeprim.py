"""The numpy fp64 reference of the plane-sphere / -capsule / -cylinder contacts (tests/planeprim_ref.py) against the f64 oracle on
the states of tests/golden/planeprim_states.npz, the class census of that fixture, its threshold margins, and the share of pairs
that the GPU test (tests/test_planeprim_gpu.py) leaves out of its oracle-parity check.  No kernel runs here: this is the test of
the reference and of the fixture, so that every exclusion of the GPU test is decided by references alone."""
import ctypes as C
import os

import numpy as np
import pytest

import planeprim_cases as PC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planeprim_states.npz")
SCENES = {"footstand": 12, "go2flat": 4}          # scene -> contact capacity of its kernels
MARGIN = 1e-5
NL = len(PC.LABELS)


def load_scene(oracle_mod, name):
    """The fixture's states of one scene with both oracles' contacts per pair and the reference's result of every near pair.
    Returns a dict: qpos, pair (targeted), labels, arrays, blob, and per state c64 / c32 (contacts per pair, uncapped), total
    (the f64 count), gpos / gmat (the f64 oracle's geom poses), gmat32 (the f32 oracle's), res (pair -> reference result on the
    f64 oracle's geom poses, of every near pair and every pair either oracle has in contact), tie_state (the target is of a
    declared tie class: cylinder aligned, or the fixture's exact-branch flag)."""
    from model_variants import blob_of, envdef_of
    envdef = envdef_of(name)
    m, blob = envdef.sys, blob_of(envdef)
    o64, o32 = oracle_mod.Oracle(blob, "f64"), oracle_mod.Oracle(blob, "f32")
    z = np.load(GOLDEN)
    S = dict(name=name, model=m, arrays=m.arrays, blob=blob, cap=SCENES[name], qpos=z[f"{name}_qpos"], pair=z[f"{name}_pair"].astype(int),
             labels=z[f"{name}_labels"].astype(int), label_names=[str(s) for s in z["label_names"]], seed=int(z[f"{name}_seed"]),
             c64=[], c32=[], total=[], res=[], gpos=[], gmat=[], gmat32=[])
    assert S["qpos"].dtype == np.float32 and S["qpos"].shape == (len(S["pair"]), m.nq) and S["label_names"][:NL] == list(PC.LABELS)
    for q in S["qpos"]:
        c64, total, gpos, gmat = PC.oracle_contacts(o64, q, m.nv, m.nu)
        c32, _, _, gmat32 = PC.oracle_contacts(o32, q, m.nv, m.nu)
        S["c64"].append(c64); S["total"].append(total); S["gpos"].append(gpos); S["gmat"].append(gmat); S["c32"].append(c32); S["gmat32"].append(gmat32)
        res = PC.pair_results(m.arrays, gpos, gmat)
        res.update(PC.pair_results(m.arrays, gpos, gmat, only=(set(c64) | set(c32)) - set(res)))
        S["res"].append(res)
    aligned = 1 << PC.CLASSES.index("cylinder aligned")
    S["tie_state"] = ((S["labels"][:, 1] & aligned) != 0) | (S["labels"][:, NL + 1] != 0)
    oracle_mod.reset_switches()
    return S


def pair_tie_class(S, e, p):
    """is pair p of state e of a declared tie class?  (fp64 label `cylinder aligned`, or float32 `vec` exactly zero)"""
    r = S["res"][e][p]
    if r["kind"] != "cylinder":
        return False
    g1, g2 = int(S["arrays"]["pair_geom1"][p]), int(S["arrays"]["pair_geom2"][p])
    return "cylinder aligned" in PC.classes_of(r) or PC.exact_branch_f32(S["gmat32"][e][g1], S["gmat32"][e][g2])


@pytest.fixture(scope="module", params=list(SCENES))
def scene(request, oracle_mod):
    return load_scene(oracle_mod, request.param)


def test_reference_agrees_with_f64_oracle(scene, oracle_mod):
    """Per pair of every state, on the oracle's own geom poses: the same pairs are in contact, with the same points in the same
    order, dist, pos and normal to 1e-9; and the capsule's frame (n, b, n x b) to 1e-9.  The oracle's collision() copies the frame
    that its plane_capsule returns into the contact record; the record's getter lists the normal only, so the frame is read from
    the same function through its stand-alone entry point on the same geom poses, and its first row is held against the
    record's normal."""
    from oracle.oracle import _load
    lib64 = _load("f64")
    A = scene["arrays"]
    size = np.asarray(A["geom_size"], np.float32).astype(float)
    worst = dict(dist=0.0, pos=0.0, normal=0.0, frame=0.0)
    pairs = 0
    for e, (c64, res, gpos, gmat) in enumerate(zip(scene["c64"], scene["res"], scene["gpos"], scene["gmat"])):
        in_contact = {p for p, r in res.items() if r["touching"].any()}
        assert in_contact == set(c64), (scene["name"], e, in_contact, set(c64))
        for p in in_contact:
            r, (dist, pos, nrm) = res[p], c64[p]
            rd, rp, rn = PC.contacts_of(r)
            assert len(rd) == len(dist), (scene["name"], e, p)
            worst["dist"] = max(worst["dist"], np.abs(rd - dist).max()); worst["pos"] = max(worst["pos"], np.abs(rp - pos).max())
            worst["normal"] = max(worst["normal"], np.abs(rn - nrm).max())
            assert np.abs(rd - dist).max() <= 1e-9 and np.abs(rp - pos).max() <= 1e-9 and np.abs(rn - nrm).max() <= 1e-9, (scene["name"], e, p, r["kind"], PC.classes_of(r))
            pairs += 1
            if r["kind"] == "capsule":
                g1, g2 = int(A["pair_geom1"][p]), int(A["pair_geom2"][p])
                out, normal, frame = np.zeros(8), np.zeros(3), np.zeros(9)
                pp, pm, cp, cm = (np.ascontiguousarray(a, np.float64) for a in (gpos[g1], gmat[g1], gpos[g2], gmat[g2]))
                assert lib64.oracle_plane_capsule(pp.ctypes.data, pm.ctypes.data, cp.ctypes.data, cm.ctypes.data, C.c_double(size[g2, 0]), C.c_double(size[g2, 1]),
                                                  out.ctypes.data, normal.ctypes.data, frame.ctypes.data) == 2
                assert (frame[:3] == nrm).all() and (out[0::4][r["touching"]] == dist).all(), (e, p)
                worst["frame"] = max(worst["frame"], np.abs(frame.reshape(3, 3) - r["frame"]).max())
                assert np.abs(frame.reshape(3, 3) - r["frame"]).max() <= 1e-9, (scene["name"], e, p)
    print(f"{scene['name']}: {pairs} pairs in contact; largest difference", {k: f"{v:.1e}" for k, v in worst.items()})
    assert pairs >= len(scene["qpos"])


def test_fixture_labels_and_margins(scene):
    """The labels in the fixture are the reference's for the targeted pair; the stored contact count is the f64 oracle's; the
    exact-branch flag is planeprim_cases.exact_branch_f32 on the f32 oracle's matrices; every contact of the target is among the
    first ncon_max of the uncapped sequence; and no near pair of any state has a threshold quantity within 1e-5 of its threshold
    (`len` apart in the states of the two aligned classes; the flat / just-not-flat classes lie on either side of 1e-3)."""
    A = scene["arrays"]
    for e, (res, c64) in enumerate(zip(scene["res"], scene["c64"])):
        p = scene["pair"][e]
        assert scene["labels"][e, :NL].tolist() == PC.labels(res[p]), e
        assert scene["labels"][e, NL] == scene["total"][e], e
        exact = res[p]["kind"] == "cylinder" and PC.exact_branch_f32(scene["gmat32"][e][int(A["pair_geom1"][p])], scene["gmat32"][e][int(A["pair_geom2"][p])])
        assert scene["labels"][e, NL + 1] == int(exact), e
        seq = [q for q in sorted(c64) for _ in c64[q][0]]
        assert p in seq and max(i for i, q in enumerate(seq) if q == p) < scene["cap"], e
        near = {q: r for q, r in res.items() if r["dist"].min() <= 1e-2}
        assert min(PC.margin_of(r, aligned=bool(scene["tie_state"][e])) for r in near.values()) >= MARGIN, e
        cls = PC.classes_of(res[p])
        if "cylinder flat" in cls:
            assert abs(res[p]["prj"]) * res[p]["halflen"] < 5e-4
        if "cylinder just not flat" in cls:
            assert 2e-3 <= abs(res[p]["prj"]) * res[p]["halflen"] <= 6e-3 and not res[p]["flat"]


def test_class_census(scene):
    """Every class has at least 24 targeted states (the second scene, the flat-terrain Go2, has the sphere class only); the
    aligned class at least 12; every one of the Footstand's 30 pairs is the target of at least 4 states; at least 48 states hold
    more than ncon_max penetrating contacts.  The number of exact-branch states is printed, not asserted."""
    cen = PC.census([row[:NL].tolist() for row in scene["labels"]])
    for k, v in cen.items():
        print(f"{scene['name']:9s} {k:26s} {v}")
    over = int((np.array(scene["total"]) > scene["cap"]).sum())
    exact = int((scene["labels"][:, NL + 1] != 0).sum())
    print(f"{scene['name']:9s} states {len(scene['qpos'])}, over the capacity {over}, exact-branch {exact}")
    if scene["name"] == "footstand":
        short = {k: v for k, v in cen.items() if v < (12 if k == "cylinder aligned" else 24)}
        assert not short, short
        per_pair = np.bincount(scene["pair"], minlength=30)
        assert len(scene["arrays"]["pair_kind"]) == 30 and per_pair.min() >= 4, per_pair
        assert over >= 48
    else:
        assert cen["sphere foot"] >= 24 and np.bincount(scene["pair"], minlength=4).min() >= 4


def test_exclusion_caps(scene):
    """A pair in contact is a tie (left out of the GPU test's oracle-parity check only) if the f32 and f64 oracles disagree on its
    point count or, set-matched, by more than 1e-4 in pos.  Outside the two declared tie classes (cylinder aligned: the fp64 label;
    exact branch: float32 `vec` exactly zero) ties are at most 5 % of the pairs in contact, and at most 15 % of any class; decided
    by the two oracles alone."""
    per_class, ties, pairs, declared = {}, 0, 0, [0, 0]
    for e, (c64, c32, res) in enumerate(zip(scene["c64"], scene["c32"], scene["res"])):
        for p in set(c64) | set(c32):
            tie = PC.is_tie(c32.get(p), c64.get(p))
            if pair_tie_class(scene, e, p):
                declared[0] += 1; declared[1] += tie
                continue
            pairs += 1; ties += tie
            for k in PC.classes_of(res[p]) or ["(no class)"]:
                a = per_class.setdefault(k, [0, 0])
                a[0] += 1; a[1] += tie
    print(f"{scene['name']}: {ties} ties in {pairs} pairs in contact ({100 * ties / pairs:.2f} %); declared tie classes: {declared[1]} ties in {declared[0]} pairs")
    for k, (n, t) in sorted(per_class.items()):
        print(f"{scene['name']:9s} {k:26s} {t:4d} of {n:5d} ({100 * t / n:.1f} %)")
    assert ties <= 0.05 * pairs
    bad = {k: v for k, v in per_class.items() if v[1] > 0.15 * v[0]}
    assert not bad, bad
