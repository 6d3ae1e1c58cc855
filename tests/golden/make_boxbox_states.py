"""States that put the free body of the two Airbot scenes into chosen box-box and plane-box contacts, one targeted pair per state,
written to tests/golden/boxbox_states.npz (inputs and fp64 class labels only; qvel = ctrl = 0).

Placement: fix an arm qpos, run the f64 oracle's forward, read geom_xpos / geom_xmat of the arm or table geom `ga`, choose a relative
pose of box `gb` of the free body (a signed axis permutation, a spin about the contact axis and a random rotation at one of three
scales; then a bisection along the contact axis to a penetration of 0.1 .. 3 mm) and write the body pose into qpos rounded to
float32.  Labels come from tests/boxbox_ref.py (numpy fp64) on the oracle's geom poses of the ROUNDED state.  A state is rejected if
in fp64 any near pair has a threshold quantity within 1e-5 of its threshold (separating values, clip-vertex depths, plane-box
supports at the band edge, the edge-over-face preference), if a pick of the manifold selection of any pair is within 1e-4 of the
winning value while it would change the reported set, or if its uncapped contact count exceeds the kernel's capacity (except the
class of states with 9 or more pending pairs, which may).  Seeded; numpy and the oracle only.

tests/test_boxbox_manifold.py asserts the census of the labels; tests/test_boxbox_manifold_gpu.py runs the kernels on the states."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import boxbox_cases as BC
import boxbox_ref as BR
from conftest import make_blob
from oracle import oracle as O
from rsr_mjx_amd import mjcf
from rsr_mjx_amd.mjcf import CompiledModel

MARGIN = 1e-5
SELECTION_MARGIN = 1e-4          # relative to the winning value of a pick
SCALES = (0.02, 0.3, 1.0)
HOME = np.array([0, -0.5422302, 0.45173569, 1.5718, -1.4794435, 1.1731174])
SCENES = dict(
    tshape=dict(asset="airbot_tshape.npz", free=8, boxes=(23, 24), n=2048, n_plane=288, n_pend=96, cap=32, fingers=(0.0, 0.0)),
    cube=dict(asset="airbot_cube.npz", free=15, boxes=(22,), n=512, n_plane=96, n_pend=32, cap=24, fingers=(0.033, -0.033)),
)
GA = (16, 3, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 1, 9, 2, 4)
# the 24 proper signed axis permutations
PERMS = [P for P in (np.array([[s0 * (p0 == c), s1 * (p1 == c), s2 * (p2 == c)] for c in range(3)], float)
                     for p0, p1, p2 in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))
                     for s0 in (1, -1) for s1 in (1, -1) for s2 in (1, -1)) if np.linalg.det(P) > 0]


def rand_rot(rng, scale):
    q = np.array([1.0, 0, 0, 0]) + scale * rng.normal(size=4)
    return mjcf.quat_to_mat(q / np.linalg.norm(q))


def axis_rot(axis, ang):
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def mat_to_quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 0.1:
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    else:                                          # near a half turn: from the largest diagonal element
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(max(0.0, 1 + R[i, i] - R[j, j] - R[k, k])) * 2
        q = np.zeros(4)
        q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


class Scene:
    def __init__(self, name):
        self.name, self.cfg = name, SCENES[name]
        self.m = CompiledModel.load(os.path.join(ROOT, "rsr_mjx_amd", "assets", self.cfg["asset"]))
        self.A = self.m.arrays
        self.orc = O.Oracle(make_blob(self.m, name), "f64")
        self.size = np.asarray(self.A["geom_size"], np.float32).astype(float)
        self.pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(self.A["pair_geom1"], self.A["pair_geom2"]))}

    def base_qpos(self, arm):
        q = np.asarray(self.A["qpos0"], float).copy()
        q[:6] = arm
        q[6], q[7] = self.cfg["fingers"]
        if self.name == "cube":                    # the second cube: sunk 1 mm into the table top at a small tilt (never exactly resting)
            q[8:15] = [0.55, -0.2, 0.819, *mat_to_quat(rand_rot(np.random.default_rng(1), 0.004))]
        return q

    def forward(self, q):
        self.orc.set_ncon_cap(1 << 20)
        self.orc.forward(q, np.zeros(self.m.nv), np.zeros(self.m.nu), None)
        return self.orc.get("geom_xpos").reshape(-1, 3), self.orc.get("geom_xmat").reshape(-1, 9), int(self.orc.get("counts")[3])

    def place(self, q, gb, pb, Rb):
        """qpos (float32) with the free body posed so that its box gb sits at (pb, Rb)"""
        f = self.cfg["free"]
        q = q.copy()
        q[f:f + 3] = pb - Rb @ np.asarray(self.A["geom_pos"][gb], float)
        q[f + 3:f + 7] = mat_to_quat(Rb)
        return q.astype(np.float32)

    def analyse(self, q32):
        gpos, gmat, ncon = self.forward(q32.astype(np.float64))
        res = BC.pair_results(self.A, gpos, gmat)
        return res, ncon, min((r["margin"] for r in res.values()), default=1.0)


def sink(pa, Ra, sa, p0, d, Rb, sb, depth):
    """the position p0 + r d of box B at which the largest separating value is -depth (bisection from outside)"""
    def worst(r):
        face, edge, *_ = BR.sat(pa, Ra, sa, p0 + r * d, Rb, sb)
        return max(face.max(), np.nanmax(edge) if not np.isnan(edge).all() else -1.0)
    hi = np.linalg.norm(sa) + np.linalg.norm(sb) + np.linalg.norm(p0 - pa)
    lo = 0.0
    if worst(hi) <= -depth:
        return None
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if worst(mid) > -depth:
            hi = mid
        else:
            lo = mid
    return p0 + hi * d


def boxbox_candidate(sc, rng, gpos, gmat, ga, gb, scale, want_edge, octagon=False):
    pa, Ra, sa, sb = gpos[ga], gmat[ga].reshape(3, 3), sc.size[ga], sc.size[gb]
    Rb = Ra @ PERMS[rng.integers(24)] @ rand_rot(rng, scale)
    A, B = Ra.T, Rb.T
    if octagon:
        # two faces of similar size, one turned by about 45 degrees in the contact plane: all four corners are clipped (8 vertices),
        # or all but one when the faces are offset (7)
        k = rng.integers(3)
        n = A[k] * rng.choice((-1.0, 1.0))
        Rb = axis_rot(n, np.pi / 4 + rng.uniform(-0.15, 0.15)) @ Ra @ PERMS[rng.integers(24)] @ rand_rot(rng, 0.01)
        lat = (rng.uniform(-1, 1, 3) * rng.choice((0.002, 0.012))) @ A
        p0, d = pa + lat - n * (n @ lat), n
    elif want_edge:
        i, j = rng.integers(3), rng.integers(3)
        d = np.cross(A[i], B[j])
        if np.linalg.norm(d) < 0.05:
            return None
        d = d / np.linalg.norm(d) * rng.choice((-1.0, 1.0))
        # the two supporting edges cross near a random point of each
        ea = sum((1.0 if d @ A[k] > 0 else -1.0) * sa[k] * A[k] for k in range(3) if k != i) + rng.uniform(-0.9, 0.9) * sa[i] * A[i]
        eb = sum((1.0 if d @ B[k] > 0 else -1.0) * sb[k] * B[k] for k in range(3) if k != j) + rng.uniform(-0.9, 0.9) * sb[j] * B[j]
        p0 = pa + ea + eb - d * (d @ (ea + eb))
    else:
        use_a = rng.random() < 0.5
        k = rng.integers(3)
        n = (A[k] if use_a else B[k]) * rng.choice((-1.0, 1.0))
        if rng.random() < 0.5:                     # spin about the contact axis: clipped polygons with 5 .. 8 vertices
            Rb = axis_rot(n, rng.uniform(0, 2 * np.pi)) @ Rb
            B = Rb.T
        reach = sa + np.abs(A @ B.T) @ sb * rng.choice((0.2, 1.0))
        lat = (rng.uniform(-1, 1, 3) * reach) @ A
        p0, d = pa + lat - n * (n @ lat), n
    pb = sink(pa, Ra, sa, p0, d, Rb, sb, rng.uniform(1e-4, 3e-3))
    return None if pb is None else (pb, Rb)


def plane_candidate(sc, rng, gb, cls):
    """box gb on the floor with 1 (vertex), 2 (edge) or 4 (face) vertices inside the 1 mm band"""
    sb = sc.size[gb]
    R = PERMS[rng.integers(24)].copy()
    if cls == 2:                                   # an edge down: roll about a horizontal box axis
        R = axis_rot(np.array([1.0, 0, 0]), rng.uniform(0.3, np.pi / 2 - 0.3)) @ R
    if cls == 1:
        R = rand_rot(rng, 1.0)
    extent = 2 * np.linalg.norm(sb)
    tilt = rng.uniform(0.02, 0.6) * 1e-3 / extent if cls != 1 else 0.0
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    R = axis_rot(ax, tilt + 1e-4) @ R
    R = axis_rot(np.array([0, 0, 1.0]), rng.uniform(0, 2 * np.pi)) @ R
    low = BR.box_vertices(np.zeros(3), R, sb)[:, 2].min()
    pb = np.array([rng.uniform(1.2, 2.0), rng.uniform(-1.5, 1.5), -low - rng.uniform(1e-4, 3e-3)])
    return pb, R


def generate(name, seed):
    sc = Scene(name)
    cfg, rng = sc.cfg, np.random.default_rng(seed)
    arms = []
    while len(arms) < 12:                          # arm poses that touch nothing on their own
        arm = HOME + rng.uniform(-0.5, 0.5, 6)
        q = sc.base_qpos(arm)
        q[cfg["free"]:cfg["free"] + 3] = [1.5, 1.5, 2.0]
        res, ncon, margin = sc.analyse(q.astype(np.float32))
        if ncon == (4 if name == "cube" else 0) and margin > 1e-4:
            arms.append(arm)
    rows, counts = [], {}
    quota = 30 if name == "tshape" else 8         # (the census asks for 24 in the T-shape set, 4 in the cube set)
    need = lambda c: c != ("emptied",) and counts.get(c, 0) < quota
    short_trials = 0

    def classes(lab):
        L = dict(zip(BC.LABELS, lab))
        out = []
        if L["kind"] == 1:
            out.append(("edge", L["wi"], L["wj"]))
        if L["kind"] == 2:
            out += [("face", L["face_code"], L["nref_sign"]), ("mq", L["mq"]), ("count", L["count"])]
        if L["face_code"] >= 0:
            out += [("poly", L["nvert"])] + ([("emptied",)] if L["emptied"] else [])
        return out

    def accept(q32, pair, scale_i, pend_class=False):
        res, ncon, margin = sc.analyse(q32)
        if margin < MARGIN or pair not in res:
            return None
        # a selection within 1e-4 of a tie in fp64 (another pick would change the reported set) is left to neither implementation
        for r in res.values():
            if r["kind"] in ("face", "plane"):
                x, y = (r["poly_x"], r["poly_y"]) if r["kind"] == "face" else (r["x"], r["y"])
                if len(BR.selection_outcomes(x, y, r["mask"], rel=SELECTION_MARGIN)) != 1:
                    return None
        npend = sum(BC.is_pending(r) for r in res.values())
        if (npend >= 9) != pend_class or (not pend_class and ncon > cfg["cap"]):
            return None
        return BC.labels(res[pair]) + [npend, ncon, scale_i]

    # ---- box-box: every state until the classes are filled, then only states of a class still short, then every state again
    n_bb = cfg["n"] - cfg["n_plane"] - cfg["n_pend"]
    trial = 0
    while len(rows) < n_bb:
        trial += 1
        ga, gb = GA[trial % len(GA)], cfg["boxes"][(trial // len(GA)) % len(cfg["boxes"])]
        if (ga, gb) not in sc.pair_of:
            continue
        scale_i = trial % 3 if rng.random() < 0.7 else 2
        q = sc.base_qpos(arms[trial % len(arms)])
        gpos, gmat, _ = sc.forward(q)
        octagon = (need(("poly", 7)) or need(("poly", 8))) and len(rows) >= 0.55 * n_bb and rng.random() < 0.6
        if octagon:
            ga, scale_i = (6, 7, 8, 5, 9, 2, 4)[trial % 7], 0
        cand = boxbox_candidate(sc, rng, gpos, gmat, ga, gb, SCALES[scale_i], want_edge=rng.random() < 0.45, octagon=octagon)
        if cand is None:
            continue
        q32 = sc.place(q, gb, *cand)
        lab = accept(q32, sc.pair_of[(ga, gb)], scale_i)
        if lab is None or (lab[0] == 0 and not lab[BC.LABELS.index("emptied")]):
            continue
        cl = classes(lab)
        short_phase = 0.55 * n_bb <= len(rows) < 0.9 * n_bb
        if short_phase and not any(need(c) for c in cl) and short_trials < 6000:
            short_trials += 1
            continue
        for c in cl:
            counts[c] = counts.get(c, 0) + 1
        rows.append((q32, sc.pair_of[(ga, gb)], lab))
        if len(rows) % 100 == 0:
            print(name, len(rows), "states,", trial, "trials", flush=True)
    print(name, "box-box", len(rows), "states from", trial, "trials")
    # ---- plane-box: 1, 2 or 4 vertices inside the band
    trial = 0
    while len(rows) < n_bb + cfg["n_plane"]:
        trial += 1
        gb, cls = cfg["boxes"][trial % len(cfg["boxes"])], (1, 2, 4)[(trial // 2) % 3]
        q = sc.base_qpos(arms[trial % len(arms)])
        q32 = sc.place(q, gb, *plane_candidate(sc, rng, gb, cls))
        pair = sc.pair_of[(0, gb)]
        lab = accept(q32, pair, 0 if cls != 1 else 2)
        if lab is None or lab[0] != 3 or lab[BC.LABELS.index("in_band")] != cls:
            continue
        rows.append((q32, pair, lab))
    # ---- 9 or more pending pairs: the free body inside the gripper
    trial = 0
    while len(rows) < cfg["n"]:
        trial += 1
        ga, gb = (9, 11, 12, 14, 15)[trial % 5], cfg["boxes"][trial % len(cfg["boxes"])]
        q = sc.base_qpos(arms[trial % len(arms)])
        gpos, gmat, _ = sc.forward(q)
        scale_i = trial % 3
        Rb = gmat[ga].reshape(3, 3) @ PERMS[rng.integers(24)] @ rand_rot(rng, SCALES[scale_i])
        centre = gpos[[9, 11, 12, 14, 15]].mean(0) + rng.normal(size=3) * 0.02
        q32 = sc.place(q, gb, centre + Rb @ np.asarray(sc.A["geom_pos"][gb], float) * rng.uniform(0, 1), Rb)
        lab = accept(q32, sc.pair_of[(ga, gb)], scale_i, pend_class=True)
        if lab is not None:
            rows.append((q32, sc.pair_of[(ga, gb)], lab))
    return rows


if __name__ == "__main__":
    out = {}
    for name, seed in (("tshape", 0), ("cube", 1)):
        rows = generate(name, seed)
        out[f"{name}_qpos"] = np.array([r[0] for r in rows], np.float32)
        out[f"{name}_pair"] = np.array([r[1] for r in rows], np.int16)
        out[f"{name}_labels"] = np.array([r[2] for r in rows], np.int16)
        lab = out[f"{name}_labels"]
        for k, v in BC.census([list(r) for r in lab[:, :len(BC.LABELS)]]).items():
            print(name, k, v)
        print(name, "states with >= 9 pending pairs", int((lab[:, len(BC.LABELS)] >= 9).sum()))
    out["label_names"] = np.array(BC.LABELS + ("npend", "ncon", "scale"))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "boxbox_states.npz"), **out)
