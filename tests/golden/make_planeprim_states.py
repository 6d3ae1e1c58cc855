"""States that put one chosen geom of the Footstand model (and, as a second scene, one foot of the flat-terrain Go2) into a chosen
class of plane-capsule / plane-cylinder / plane-sphere contact, one targeted pair per state, written to
tests/golden/planeprim_states.npz (inputs, the targeted pair and fp64 labels only; qvel = ctrl = 0 in the contact tests).

Construction: draw the twelve joint angles uniformly inside jnt_range shrunk by 0.02; read the target geom's pose with the trunk at
identity from the f64 oracle's kinematics; choose the geom's world axis for the class (its angle from the floor's normal, a random
heading and a random spin about the axis); set the trunk quaternion to R_world R_trunk->geom^T and the trunk height so that the
target's deepest point is 0.5 .. 4 mm inside the floor; round to float32.  Labels come from tests/planeprim_ref.py (numpy fp64) on
the f64 oracle's geom poses of the ROUNDED state.  A state is kept if the f64 oracle has the target pair in contact, every contact
of the target is among the first ncon_max of the uncapped pair-order sequence, the target is of the wanted class, and every near
pair is clear of each threshold by 1e-5 in fp64 (in the aligned class: all but `len`); otherwise it is redrawn.

The device's exact branch `len < 1e-12`: for every cylinder the generator tries trunk poses that would put its axis on the normal
with every matrix entry exact (quarter turns about the normal, hip angle zero) and asks planeprim_cases.exact_branch_f32 on the
f32 oracle's geom_xmat; what it finds is stored with the flag `exact` and printed.  Seeded; numpy and the oracle only.

The floor's normal is (0, 0, 1) in every shipped model, so the capsule's (0, 0, 1) fallback tangent (|n_y| >= 0.5) cannot be reached.

tests/test_planeprim.py asserts the census of the labels; tests/test_planeprim_gpu.py runs the kernels on the states."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import planeprim_cases as PC
from make_boxbox_states import axis_rot, mat_to_quat
from model_variants import blob_of, envdef_of
from oracle import oracle as O

MARGIN = 1e-5
SCENES = dict(footstand=dict(cap=12, seed=0), go2flat=dict(cap=4, seed=1))
PER_PAIR = {"capsule": 2, "cylinder": 5, "sphere": 8}          # states per pair and class
# the angle of the geom's axis from the floor's normal per class: draw(rng, r, hl, depth) -> theta in [0, pi]
up_or_down = lambda rng, t: t if rng.random() < 0.5 else np.pi - t
DRAW = {
    "capsule axis tangent +": lambda rng, r, hl, depth: np.pi - np.radians(rng.uniform(35.5, 88.0)),
    "capsule axis tangent -": lambda rng, r, hl, depth: np.radians(rng.uniform(35.5, 88.0)),
    "capsule fallback tangent": lambda rng, r, hl, depth: up_or_down(rng, np.radians(rng.uniform(0.5, 29.9))),
    "capsule upright": lambda rng, r, hl, depth: up_or_down(rng, 0.0),
    "capsule lying flat": lambda rng, r, hl, depth: up_or_down(rng, np.arccos(rng.uniform(2e-5, depth - 5e-5) / (2 * hl))),
    "cylinder tilt +": lambda rng, r, hl, depth: rng.uniform(0.15, np.pi / 2 - 0.35),
    "cylinder tilt -": lambda rng, r, hl, depth: np.pi - rng.uniform(0.15, np.pi / 2 - 0.35),
    "cylinder flat": lambda rng, r, hl, depth: up_or_down(rng, np.arccos(rng.uniform(2e-5, 4.9e-4) / hl)),
    "cylinder just not flat": lambda rng, r, hl, depth: up_or_down(rng, np.arccos(rng.uniform(2.1e-3, 5.9e-3) / hl)),
    "cylinder small tilt": lambda rng, r, hl, depth: up_or_down(rng, rng.uniform(0.011, 0.099)),
    "cylinder near aligned": lambda rng, r, hl, depth: up_or_down(rng, np.exp(rng.uniform(np.log(1.2e-5), np.log(9e-4)))),
    "cylinder aligned": lambda rng, r, hl, depth: up_or_down(rng, 0.0),
    "sphere foot": lambda rng, r, hl, depth: rng.uniform(0, 0.6),
}
WANT = {k: k.rstrip(" +-") if k.startswith("capsule axis") else k for k in DRAW}
KINDS = {PC.PAIR_PLANE_SPHERE: "sphere", PC.PAIR_PLANE_CAPSULE: "capsule", PC.PAIR_PLANE_CYLINDER: "cylinder"}


def frame_about(axis, spin):
    """a rotation whose third column is `axis` (unit), turned about it by `spin`"""
    h = np.array([1.0, 0, 0]) if abs(axis[0]) < 0.9 else np.array([0, 1.0, 0])
    x = np.cross(h, axis); x /= np.linalg.norm(x)
    return axis_rot(axis, spin) @ np.stack([x, np.cross(axis, x), axis], 1)


class Scene:
    def __init__(self, name):
        self.name, self.cfg = name, SCENES[name]
        envdef = envdef_of(name)
        self.m, self.A = envdef.sys, envdef.sys.arrays
        blob = blob_of(envdef)
        self.o64, self.o32 = O.Oracle(blob, "f64"), O.Oracle(blob, "f32")
        self.size = np.asarray(self.A["geom_size"], np.float32).astype(float)
        self.lo, self.hi = self.A["jnt_range"][1:, 0] + 0.02, self.A["jnt_range"][1:, 1] - 0.02

    def forward(self, q, orc=None):
        orc = orc or self.o64
        return PC.oracle_contacts(orc, q, self.m.nv, self.m.nu)

    def pose(self, rng, pair, theta, joints=None, spin=None, heading=None, depth=None):
        """float32 qpos with the pair's geom at angle theta from the floor's normal, its deepest point `depth` inside the floor"""
        g = int(self.A["pair_geom2"][pair])
        q = np.asarray(self.A["qpos0"], float).copy()
        q[7:] = rng.uniform(self.lo, self.hi) if joints is None else joints
        q[:7] = [0, 0, 1, 1, 0, 0, 0]
        _, _, gpos, gmat = self.forward(q)
        heading = rng.uniform(0, 2 * np.pi) if heading is None else heading
        axis = np.array([np.sin(theta) * np.cos(heading), np.sin(theta) * np.sin(heading), np.cos(theta)])
        if theta in (0.0, np.pi):
            axis = np.array([0, 0, np.cos(theta)])                 # exactly along the normal
        Rw = frame_about(axis, rng.uniform(0, 2 * np.pi) if spin is None else spin)
        R = Rw @ gmat[g].reshape(3, 3).T
        origin = np.array([0, 0, 1.0])
        world_p, world_R = (gpos - origin) @ R.T, np.einsum("ij,gjk->gik", R, gmat.reshape(-1, 3, 3)).reshape(-1, 9)
        world_p[0], world_R[0] = gpos[0], gmat[0]                    # the floor stays
        low = PC.pair_results(self.A, world_p, world_R, only={pair})[pair]["dist"].min()
        depth = rng.uniform(5e-4, 4e-3) if depth is None else depth
        q[:3] = [rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -low - depth]
        q[3:7] = mat_to_quat(R)
        return q.astype(np.float32)

    def rate(self, q32, pair, want, aligned=False):
        """the fixture's label row of a state, or None if it is not to be kept"""
        c64, total, gpos, gmat = self.forward(q32.astype(np.float64))
        if pair not in c64:
            return None
        seq = [p for p in sorted(c64) for _ in c64[p][0]]
        if max(i for i, p in enumerate(seq) if p == pair) >= self.cfg["cap"]:
            return None
        res = PC.pair_results(self.A, gpos, gmat)
        if pair not in res or (want is not None and want not in PC.classes_of(res[pair])):
            return None
        if min(PC.margin_of(r, aligned) for r in res.values()) < MARGIN:
            return None
        g1, g2 = int(self.A["pair_geom1"][pair]), int(self.A["pair_geom2"][pair])
        exact = 0
        if res[pair]["kind"] == "cylinder":
            gmat32 = self.forward(q32.astype(np.float64), self.o32)[3]
            exact = int(PC.exact_branch_f32(gmat32[g1], gmat32[g2]))
        return PC.labels(res[pair]) + [total, exact]


def generate(name):
    sc = Scene(name)
    rng = np.random.default_rng(sc.cfg["seed"])
    rows, short = [], []
    kinds = [KINDS[int(k)] for k in sc.A["pair_kind"]]
    for pair, kind in enumerate(kinds):
        r, hl = sc.size[int(sc.A["pair_geom2"][pair])][:2]
        for cls in (c for c in DRAW if c.startswith(kind)):
            if cls == "cylinder aligned" and int(sc.A["geom_bodyid"][int(sc.A["pair_geom2"][pair])]) == 1:
                # the trunk's cylinders lie along its x axis and the hip cylinders along its y axis at every hip angle: with the
                # trunk on end, the hip cylinders on the floor are exactly level, on the threshold that picks the facing disk,
                # and that is no declared tie class.  The aligned class is made of the hip cylinders.
                continue
            got = 0
            per_pair = PER_PAIR[kind] if name == "footstand" else 10
            for trial in range(600):
                if got == per_pair:
                    break
                depth = rng.uniform(5e-4, 4e-3)
                q32 = sc.pose(rng, pair, DRAW[cls](rng, r, hl, depth), depth=depth)
                lab = sc.rate(q32, pair, WANT[cls], aligned=cls == "cylinder aligned")
                if lab is not None:
                    rows.append((q32, pair, lab)); got += 1
            if got < per_pair:
                short.append((pair, cls, got))
        print(name, "pair", pair, kind, len(rows), "states", flush=True)
    # ---- the exact branch: axis on the normal with exact matrix entries (quarter-turn spins and headings, hip angle zero)
    found = 0
    for pair, kind in enumerate(kinds):
        if kind != "cylinder":
            continue
        got = 0
        for trial in range(64):
            joints = rng.uniform(sc.lo, sc.hi)
            joints[0::3] = 0.0                                      # the hip cylinders turn with the abduction joints
            q32 = sc.pose(rng, pair, (0.0, np.pi)[trial % 2], joints=joints, spin=(trial // 2 % 4) * np.pi / 2, heading=0.0)
            q32[3:7] = np.where(np.abs(q32[3:7]) < 1e-7, 0, q32[3:7])          # (the quaternion's zeros, exactly)
            lab = sc.rate(q32, pair, "cylinder aligned", aligned=True)
            if lab is not None and lab[-1] and got < 4:
                rows.append((q32, pair, lab)); got += 1
        found += got
    print(name, "exact-branch states found:", found)
    print(name, "classes short of their per-pair quota:", short)
    return rows


if __name__ == "__main__":
    out = {}
    for name in SCENES:
        rows = generate(name)
        out[f"{name}_qpos"] = np.array([r[0] for r in rows], np.float32)
        out[f"{name}_pair"] = np.array([r[1] for r in rows], np.int16)
        out[f"{name}_labels"] = np.array([r[2] for r in rows], np.int32)
        out[f"{name}_seed"] = np.array(SCENES[name]["seed"])
        lab = out[f"{name}_labels"]
        for k, v in PC.census([list(r) for r in lab[:, :len(PC.LABELS)]]).items():
            print(name, k, v)
        print(name, len(rows), "states;", int((lab[:, 3] > SCENES[name]["cap"]).sum()), "over the contact capacity;", int(lab[:, 4].sum()), "exact-branch")
    out["label_names"] = np.array(PC.LABELS + ("ncon", "exact"))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "planeprim_states.npz"), **out)
