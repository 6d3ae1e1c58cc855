"""What the plane-sphere / -capsule / -cylinder tests build around the numpy reference (tests/planeprim_ref.py): the reference's
result for every such pair of a model, the classes a result belongs to and their census, the reference's contact list per pair,
and the float32 test for the device's exact `len < 1e-12` branch.  Contact lists per pair, the oracle's contacts, set matching and
the tie rule are those of tests/boxbox_cases.py."""
import numpy as np

from boxbox_cases import by_pair, is_tie, match_sets, oracle_contacts          # noqa: F401  (shared with the tests of this module)
from planeprim_ref import plane_capsule, plane_cylinder, plane_sphere

PAIR_PLANE_SPHERE, PAIR_PLANE_CAPSULE, PAIR_PLANE_CYLINDER = 2, 4, 5
KIND_CODE = {"sphere": PAIR_PLANE_SPHERE, "capsule": PAIR_PLANE_CAPSULE, "cylinder": PAIR_PLANE_CYLINDER}

# class -> bit of the fixture's class mask.  A pair may belong to several (a capsule to one tangent class and one sign class).
CLASSES = ("capsule axis tangent", "capsule fallback tangent", "capsule upright", "capsule lying flat", "capsule +end deeper",
           "capsule -end deeper", "cylinder tilt +", "cylinder tilt -", "cylinder flat", "cylinder just not flat",
           "cylinder small tilt", "cylinder near aligned", "cylinder aligned", "sphere foot")
# rim direction lost to rounding: the f32 and the f64 oracle put the points elsewhere on the rim (declared tie classes; the
# second one, the states whose float32 `vec` is exactly zero, is a flag of the fixture and not an fp64 label)
TIE_CLASSES = ("cylinder aligned", "cylinder exact branch")
LABELS = ("kind", "classes", "count")


def pair_results(arrays, gpos, gmat, skip_beyond=1e-2, only=None):
    """{pair index: reference result} for every plane-sphere / -capsule / -cylinder pair of the model whose lowest point is less
    than `skip_beyond` above the plane, or with `only` for exactly those pairs; gpos [ngeom, 3] and gmat [ngeom, 9] are the f64
    oracle's geom_xpos / geom_xmat."""
    gpos, gmat = np.asarray(gpos, float).reshape(-1, 3), np.asarray(gmat, float).reshape(-1, 9)
    size = np.asarray(arrays["geom_size"], np.float32).astype(float)          # (the model blob holds float32)
    incl = np.asarray(arrays["pair_margin"], np.float32).astype(float) - np.asarray(arrays["pair_gap"], np.float32).astype(float)
    out = {}
    for p, (g1, g2, kind) in enumerate(zip(arrays["pair_geom1"], arrays["pair_geom2"], arrays["pair_kind"])):
        if only is not None and p not in only:
            continue
        if kind == PAIR_PLANE_SPHERE:
            r = plane_sphere(gpos[g1], gmat[g1], gpos[g2], size[g2, 0], incl[p])
        elif kind == PAIR_PLANE_CAPSULE:
            r = plane_capsule(gpos[g1], gmat[g1], gpos[g2], gmat[g2], size[g2, 0], size[g2, 1], incl[p])
        elif kind == PAIR_PLANE_CYLINDER:
            r = plane_cylinder(gpos[g1], gmat[g1], gpos[g2], gmat[g2], size[g2, 0], size[g2, 1], incl[p])
        else:
            continue
        if only is None and r["dist"].min() - incl[p] > skip_beyond:
            continue
        out[p] = r
    return out


def contacts_of(r):
    """(dist[k], pos[k, 3], normal[3]) of the reference's points in contact, in the order the narrow phase lists them; None if none is"""
    m = r["touching"]
    return (r["dist"][m], r["pos"][m], r["normal"]) if m.any() else None


def classes_of(r):
    """the classes of CLASSES one pair's reference result belongs to (a pair out of contact: none)"""
    if not r["touching"].any():
        return []
    out = []
    if r["kind"] == "sphere":
        out.append("sphere foot")
    elif r["kind"] == "capsule":
        both = bool(r["touching"].all())
        if r["bn"] < 1e-5:
            out.append("capsule upright")
        elif r["fallback"]:
            out.append("capsule fallback tangent")
        elif both:
            out.append("capsule lying flat")
        elif r["bn"] >= np.sin(np.radians(35.0)):
            out.append("capsule axis tangent")
        if r["dist"][0] != r["dist"][1]:
            out.append("capsule +end deeper" if r["dist"][0] < r["dist"][1] else "capsule -end deeper")
    else:
        prj_hl = abs(r["prj"]) * r["halflen"]
        if r["theta"] < 5e-6:
            out.append("cylinder aligned")
        elif 1e-5 <= r["theta"] <= 1e-3:
            out.append("cylinder near aligned")
        elif 0.01 <= r["theta"] <= 0.1:
            out.append("cylinder small tilt")
        elif prj_hl < 5e-4:
            out.append("cylinder flat")
        elif 2e-3 <= prj_hl <= 6e-3:
            out.append("cylinder just not flat")
        elif r["theta"] > 0.1 and prj_hl > 6e-3:
            out.append("cylinder tilt +" if r["prj"] > 0 else "cylinder tilt -")
    return out


def labels(r):
    """the labels of one pair's result, as the integers of LABELS: kind code, class bit mask, points in contact"""
    return [KIND_CODE[r["kind"]], sum(1 << CLASSES.index(c) for c in classes_of(r)), int(r["touching"].sum())]


def census(rows):
    """class -> number of cases, from label rows (lists in the order of LABELS)"""
    mask = np.array([r[LABELS.index("classes")] for r in rows], dtype=np.int64)
    return {c: int(((mask >> i) & 1).sum()) for i, c in enumerate(CLASSES)}


def margin_of(r, aligned=False):
    """the least threshold margin of a result; aligned: without `len` (the aligned classes sit on that threshold on purpose)"""
    return min(v for k, v in r["margins"].items() if not (aligned and k == "len"))


def exact_branch_f32(pmat32, cmat32):
    """does the device's `len < 1e-12` branch apply in float32?  vec = axis * (axis . n) - n after the sign flip, from the f32
    oracle's geom_xmat of the plane and the cylinder, every operation rounded to float32; |vec|^2 underflows below 1e-24, which
    with a unit-length axis and normal happens only at vec == 0."""
    f = np.float32
    n, a = np.asarray(pmat32, f).reshape(3, 3)[:, 2], np.asarray(cmat32, f).reshape(3, 3)[:, 2]
    prj = f(f(f(n[0] * a[0]) + f(n[1] * a[1])) + f(n[2] * a[2]))
    sign = f(1.0) if prj < 0 else f(-1.0)
    a, prj = (a * sign).astype(f), f(prj * sign)
    vec = ((a * prj).astype(f) - n).astype(f)
    return bool(np.sqrt(f(f(f(vec[0] * vec[0]) + f(vec[1] * vec[1])) + f(vec[2] * vec[2]))) < f(1e-12))
