"""What the box-box / plane-box tests build around the numpy reference (tests/boxbox_ref.py): the reference's result for every pair of
a model, class labels and their census, the oracle's contact list per pair, set matching and the selection-tie rule."""
import numpy as np

from boxbox_ref import box_box, plane_box

PAIR_PLANE_BOX, PAIR_BOX_BOX = 0, 1


def pair_results(arrays, gpos, gmat, skip_beyond=1e-2, only=None):
    """{pair index: plane_box / box_box result} for every plane-box and box-box pair of the model whose bounding spheres are
    closer than `skip_beyond` (farther pairs are separated by at least that much on the centre line and are left out), or with `only` for exactly those pairs;
    gpos [ngeom, 3] and gmat [ngeom, 9] are the f64 oracle's geom_xpos / geom_xmat."""
    gpos, gmat = np.asarray(gpos, float).reshape(-1, 3), np.asarray(gmat, float).reshape(-1, 9)
    size = np.asarray(arrays["geom_size"], np.float32).astype(float)          # (the model blob holds float32)
    out = {}
    for p, (g1, g2, kind) in enumerate(zip(arrays["pair_geom1"], arrays["pair_geom2"], arrays["pair_kind"])):
        if only is not None:
            if p in only:
                out[p] = plane_box(gpos[g1], gmat[g1], gpos[g2], gmat[g2], size[g2]) if kind == PAIR_PLANE_BOX else \
                    box_box(gpos[g1], gmat[g1], size[g1], gpos[g2], gmat[g2], size[g2])
            continue
        if kind == PAIR_PLANE_BOX:
            n = gmat[g1].reshape(3, 3)[:, 2]
            if (gpos[g2] - gpos[g1]) @ n - np.linalg.norm(size[g2]) > skip_beyond:
                continue
            out[p] = plane_box(gpos[g1], gmat[g1], gpos[g2], gmat[g2], size[g2])
        elif kind == PAIR_BOX_BOX:
            if np.linalg.norm(gpos[g2] - gpos[g1]) - np.linalg.norm(size[g1]) - np.linalg.norm(size[g2]) > skip_beyond:
                continue
            out[p] = box_box(gpos[g1], gmat[g1], size[g1], gpos[g2], gmat[g2], size[g2])
    return out


def is_pending(r):
    """the pair claims a scratch slot of the kernel's manifold loop: plane-box with a vertex below the plane, or a face contact
    (whether or not the clipped polygon keeps a penetrating vertex)"""
    return r["kind"] in ("plane", "face") or (r["kind"] == "none" and "pass_counts" in r)


LABELS = ("kind", "wi", "wj", "face_code", "nref_sign", "mq", "nvert", "count", "emptied", "in_band")
KIND_CODE = {"sep": 0, "none": 0, "edge": 1, "face": 2, "plane": 3}


def labels(r):
    """the class labels of one pair's result, as the integers of LABELS (-1 / 0 where a label does not apply)"""
    lab = dict(kind=KIND_CODE[r["kind"]], wi=-1, wj=-1, face_code=-1, nref_sign=0, mq=-1, nvert=-1, count=0, emptied=0, in_band=0)
    if r["kind"] == "edge":
        lab.update(wi=r["wi"], wj=r["wj"], count=1)
    if "pass_counts" in r:
        lab.update(face_code=r["face_code"], nref_sign=r["nref_sign"], mq=r["mq"], nvert=len(r["poly_x"]),
                   emptied=int(0 in r["pass_counts"]), count=len(r.get("sel", ())))
    if r["kind"] == "plane":
        lab.update(count=len(r["sel"]), in_band=int(r["mask"].sum()))
    return [lab[k] for k in LABELS]


def census(rows):
    """class -> number of cases, from label rows (lists in the order of LABELS)"""
    L = {k: np.array([r[i] for r in rows]) for i, k in enumerate(LABELS)}
    edge, face, plane = L["kind"] == 1, (L["face_code"] >= 0), L["kind"] == 3
    out = {}
    for i in range(3):
        for j in range(3):
            out[f"edge {i}{j}"] = int((edge & (L["wi"] == i) & (L["wj"] == j)).sum())
    for code in range(6):
        for sg in (1, -1):
            out[f"face {code} nref {'+' if sg > 0 else '-'}"] = int((face & (L["kind"] == 2) & (L["face_code"] == code) & (L["nref_sign"] == sg)).sum())
    for mq in range(3):
        out[f"mq {mq}"] = int((face & (L["kind"] == 2) & (L["mq"] == mq)).sum())
    for nv in range(3, 9):
        out[f"polygon {nv}"] = int((face & (L["nvert"] == nv)).sum())
    for c in range(1, 5):
        out[f"face count {c}"] = int(((L["kind"] == 2) & (L["count"] == c)).sum())
    out["clip emptied"] = int(L["emptied"].sum())
    for c in (1, 2, 4):
        out[f"plane count {c}"] = int((plane & (L["count"] == c)).sum())
    for c in (1, 2, 4):
        out[f"plane band {c}"] = int((plane & (L["in_band"] == c)).sum())
    return out


# ---- helpers shared by the CPU and the GPU test: contact lists per pair, set matching, the fixture's states ----
def by_pair(pair_ids, dist, pos, normal):
    """{pair: (dist[k], pos[k, 3], normal[3])} from a contact list in pair order"""
    out = {}
    pair_ids = np.asarray(pair_ids).astype(int)
    for p in dict.fromkeys(pair_ids.tolist()):
        m = pair_ids == p
        out[p] = (np.asarray(dist, float)[m], np.asarray(pos, float)[m], np.asarray(normal, float)[m][0])
    return out


def oracle_contacts(orc, qpos, nv, nu, cap=1 << 20):
    """(contacts per pair, uncapped count, geom_xpos, geom_xmat) of one oracle forward at zero qvel and ctrl"""
    orc.set_ncon_cap(1 << 20)
    orc.forward(qpos, np.zeros(nv), np.zeros(nu), None)
    total = int(orc.get("counts")[3])
    if total > cap:
        orc.set_ncon_cap(cap)
        orc.forward(qpos, np.zeros(nv), np.zeros(nu), None)
    c = orc.get("contacts").reshape(-1, 10)
    return by_pair(c[:, 9], c[:, 0], c[:, 1:4], c[:, 4:7]), total, orc.get("geom_xpos").reshape(-1, 3), orc.get("geom_xmat").reshape(-1, 9)


def match_sets(pos_a, pos_b):
    """the permutation of b's points (same count as a's) closest to a's in the largest coordinate difference, and that difference"""
    import itertools
    best, arg = np.inf, None
    for perm in itertools.permutations(range(len(pos_b))):
        d = np.abs(pos_a - pos_b[list(perm)]).max() if len(pos_a) else 0.0
        if d < best:
            best, arg = d, list(perm)
    return arg, best


def is_tie(c32, c64):
    """a pair in contact is a selection tie if the f32 and f64 oracles disagree on its point count or, set-matched, by more than
    1e-4 in pos (c32 / c64: the pair's entry of by_pair, or None)"""
    n32, n64 = (0 if c is None else len(c[0]) for c in (c32, c64))
    if n32 != n64:
        return True
    return n64 > 0 and match_sets(c64[1], c32[1])[1] > 1e-4


def pair_classes(r):
    """the census classes one pair's reference result belongs to"""
    return [k for k, v in census([labels(r)]).items() if v]
