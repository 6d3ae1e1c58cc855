"""The numpy fp64 restatement of the box-box / plane-box manifolds (tests/boxbox_ref.py) against the f64 oracle on the states of
tests/golden/boxbox_states.npz, the class census of that fixture, and the share of pairs that the GPU test
(tests/test_boxbox_manifold_gpu.py) leaves out of its oracle-parity check.  No kernel runs here: this is the test of the reference
and of the fixture, so that every exclusion of the GPU test is decided by references alone."""
import os

import numpy as np
import pytest

import boxbox_cases as BC
import boxbox_ref as BR
from conftest import ASSETS, make_blob

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxbox_states.npz")
SCENES = {"tshape": ("airbot_tshape.npz", 2048, 32), "cube": ("airbot_cube.npz", 512, 24)}
MARGIN = 1e-5


def load_scene(oracle_mod, name, near=True):
    """The fixture's states of one scene with both oracles' contacts per pair and the reference's result of every near pair.
    Returns a dict: qpos, pair (targeted), labels, arrays, and per state c64 / c32 (contacts per pair, uncapped), total
    (the f64 count), gpos / gmat (the f64 oracle's geom poses), res (pair -> reference result on the f64 oracle's geom poses; of
    every near pair, or with near=False of the pairs that either oracle has in contact, which is all the GPU test needs)."""
    from rsr_mjx_amd.mjcf import CompiledModel
    asset, n, cap = SCENES[name]
    m = CompiledModel.load(os.path.join(ASSETS, asset))
    blob = make_blob(m, name)
    o64, o32 = oracle_mod.Oracle(blob, "f64"), oracle_mod.Oracle(blob, "f32")
    z = np.load(GOLDEN)
    S = dict(name=name, model=m, arrays=m.arrays, cap=cap, qpos=z[f"{name}_qpos"], pair=z[f"{name}_pair"].astype(int),
             labels=z[f"{name}_labels"].astype(int), label_names=[str(s) for s in z["label_names"]], c64=[], c32=[], total=[], res=[], gpos=[], gmat=[])
    assert S["qpos"].shape == (n, m.nq) and S["qpos"].dtype == np.float32
    for q in S["qpos"]:
        c64, total, gpos, gmat = BC.oracle_contacts(o64, q, m.nv, m.nu)
        S["c64"].append(c64); S["total"].append(total); S["gpos"].append(gpos); S["gmat"].append(gmat)
        S["c32"].append(BC.oracle_contacts(o32, q, m.nv, m.nu)[0])
        S["res"].append(BC.pair_results(m.arrays, gpos, gmat, only=None if near else set(c64) | set(S["c32"][-1])))
    oracle_mod.reset_switches()
    return S


@pytest.fixture(scope="module", params=list(SCENES))
def scene(request, oracle_mod):
    return load_scene(oracle_mod, request.param)


def test_reference_agrees_with_f64_oracle(scene):
    """Per pair of every state: the same pairs are in contact with the same normal; every oracle point is a candidate of the
    reference (a vertex of its clipped polygon / a box vertex in the band / the edge point) with that candidate's depth, to 1e-9;
    and where the selection is clear (one outcome when a pick within 1e-4 of the winning value may replace the winner) the two
    report the same points as sets, to 1e-9."""
    clear = unclear = 0
    for e, (c64, res) in enumerate(zip(scene["c64"], scene["res"])):
        in_contact = {p for p, r in res.items() if r["kind"] in ("edge", "face", "plane")}
        assert in_contact == set(c64), (scene["name"], e, in_contact, set(c64))
        for p in in_contact:
            r, (dist, pos, nrm) = res[p], c64[p]
            # (the contact frame's first axis is the normal over its length; the columns of geom_xmat are unit to 1e-8 only)
            assert np.abs(nrm - r["normal"] / np.linalg.norm(r["normal"])).max() <= 1e-9, (e, p)
            if r["kind"] == "edge":
                cand = np.c_[r["dist"], r["pos"]]
                outcomes = 1
            elif r["kind"] == "face":
                x, y, d = r["poly_x"], r["poly_y"], r["poly_d"]
                cand = np.c_[-d, r["o"] + np.outer(x, r["axu"]) + np.outer(y, r["axv"]) - 0.5 * np.outer(d, r["nref"])][r["mask"]]
                outcomes = len(BR.selection_outcomes(x, y, r["mask"], rel=1e-4))
            else:
                sup = r["support"]
                cand = np.c_[-sup, r["vertices"] + 0.5 * np.outer(sup, r["normal"])][r["mask"]]
                outcomes = len(BR.selection_outcomes(r["x"], r["y"], r["mask"], rel=1e-4))
            got = np.c_[dist, pos]
            assert np.abs(got[:, None] - cand[None]).max(2).min(1).max() <= 1e-9, (scene["name"], e, p, r["kind"])
            if outcomes == 1:
                clear += 1
                assert len(dist) == len(r["sel"]), (scene["name"], e, p, r["kind"])
                perm, d = BC.match_sets(r["pos"], pos)
                assert d <= 1e-9 and np.abs(r["dist"] - dist[perm]).max() <= 1e-9, (scene["name"], e, p, r["kind"], d)
            else:
                unclear += 1
    print(f"{scene['name']}: {clear} pairs with a clear selection, {unclear} without")
    assert clear > 1000 and unclear == 0


def test_fixture_labels_and_margins(scene):
    """The labels in the fixture are the reference's for the targeted pair, and no near pair of any state has a threshold quantity
    within 1e-5 of its threshold, nor a manifold selection within 1e-4 (relative) of a tie that would change the reported set (clipped
    quadrilaterals with all four vertices penetrating are often such ties, and a third fp32 implementation resolves them its own
    way, so the generator rejects them); only states with 9 or more pending pairs exceed the contact capacity."""
    nl = len(BC.LABELS)
    for e, res in enumerate(scene["res"]):
        assert scene["labels"][e, :nl].tolist() == BC.labels(res[scene["pair"][e]]), e
        npend = sum(BC.is_pending(r) for r in res.values())
        assert scene["labels"][e, nl] == npend and scene["labels"][e, nl + 1] == scene["total"][e], e
        assert min(r["margin"] for r in res.values()) >= MARGIN, e
        for p, r in res.items():               # no pick within 1e-4 of the winning value that would change the reported set
            if r["kind"] in ("face", "plane"):
                x, y = (r["poly_x"], r["poly_y"]) if r["kind"] == "face" else (r["x"], r["y"])
                assert len(BR.selection_outcomes(x, y, r["mask"], rel=1e-4)) == 1, (e, p)
        assert scene["total"][e] <= scene["cap"] or npend >= 9, e


def test_class_census(scene):
    """Every class that the GPU test is meant to reach has at least 24 targeted cases in the T-shape set (the cube set runs the same
    code under other dimensions and is a quarter of the size: 4), at least 64 T-shape and 24 cube states hold 9 or more pending pairs,
    some of them beyond the contact capacity of their scene, and all three rotation scales are present.

    One class of the plan is absent: a clip pass that empties the polygon.  No overlapping pair produced one: none of 11.9 million random
    overlapping pairs of this model's box sizes (thin plates, the slab and the cube links against the T boxes and the cube, a third
    of them with a vertex of one box placed just inside a corner or rim of the other; 127 of them overlapped on all 15 axes without
    a penetrating point, none with an empty polygon), nor any of 20 000 shallow directed placements.
    The incident face always contains the incident box's deepest vertex along the reference normal, and when that vertex lies
    beside the reference rectangle the axis of least overlap is another one (the incident box's own face, or an edge axis), so
    the SAT does not pick this reference face; this is an argument, not a proof, and the census prints the count."""
    nl = len(BC.LABELS)
    cen = BC.census([row[:nl].tolist() for row in scene["labels"]])
    floor = 24 if scene["name"] == "tshape" else 4
    for k, v in cen.items():
        print(f"{scene['name']:7s} {k:16s} {v}")
    npend = scene["labels"][:, nl]
    over = int((np.array(scene["total"]) > scene["cap"]).sum())
    print(f"{scene['name']:7s} states with >= 9 pending pairs: {int((npend >= 9).sum())}, over the capacity: {over}")
    short = {k: v for k, v in cen.items() if v < floor and k != "clip emptied"}
    assert not short, short
    assert set(scene["labels"][:, nl + 2]) == {0, 1, 2}
    assert (npend >= 9).sum() >= (64 if scene["name"] == "tshape" else 24) and over >= 1


def test_exclusion_caps(scene):
    """A pair in contact is a selection tie (left out of the GPU test's oracle-parity check only) if the f32 and f64 oracles
    disagree on its point count or, set-matched, by more than 1e-4 in pos.  Ties are at most 5 % of the pairs in contact and at most
    15 % of any class; decided by the two oracles alone."""
    per_class, ties, pairs = {}, 0, 0
    for c64, c32, res in zip(scene["c64"], scene["c32"], scene["res"]):
        for p in set(c64) | set(c32):
            tie = BC.is_tie(c32.get(p), c64.get(p))
            pairs += 1; ties += tie
            for k in BC.pair_classes(res[p]):
                a = per_class.setdefault(k, [0, 0])
                a[0] += 1; a[1] += tie
    print(f"{scene['name']}: {ties} ties in {pairs} pairs in contact ({100 * ties / pairs:.2f} %)")
    for k, (n, t) in sorted(per_class.items()):
        print(f"{scene['name']:7s} {k:16s} {t:4d} of {n:5d} ({100 * t / n:.1f} %)")
    assert ties <= 0.05 * pairs
    bad = {k: v for k, v in per_class.items() if v[1] > 0.15 * v[0]}
    assert not bad, bad
