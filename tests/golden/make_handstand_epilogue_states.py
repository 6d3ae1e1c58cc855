"""States for the by-branch test of the Go2 Handstand / Footstand step outside the physics (tests/test_handstand_epilogue.py and _gpu.py;
classes and variants in tests/handstand_epilogue_cases.py).  Seeded, CPU only.  Three sources:
  * the f32 oracle rolled out from its reset states (half of the envs start from the crouch) with small random actions;
  * floor poses by the recipe of tests/test_handstand.py::test_handstand_hip_parity (home joints + noise, trunk lowered and tilted);
  * constructed poses.  All 30 collision pairs are against the floor plane, so lowering the trunk by s lowers every narrow-phase point
    by s: one float64 forward pass with culling off gives every point's distance at z = 1, and for a pose (orientation, joints) the
    set of penetrating points at any height follows.  The trunk height is then chosen inside a gap of at least 2 x POSE_MARGIN between
    two consecutive point distances, so that every point is at least POSE_MARGIN clear of the floor's surface, and the pose is kept for
    the contact class its penetrating set belongs to (which geoms touch, how many points, which of them among the first twelve in
    pair order).
qpos, info, steps, done, the Episode words and the action are then edited per class.  Stored is what a step reads, the reset keys that
give every env its cached first state, the class each state was built for, and per state and pair the float64 oracle's contact data
with the cap off: least point distance, whether a penetrating point of the pair is among the first twelve / beyond them, and the
number of penetrating points -- float32 / small integers, compressed: tests/golden/handstand_epilogue_states.npz.

The script also writes tests/golden/handstand_epilogue_tolerances.json: per task, variant and compared quantity max |ref32 - ref64| of
tests/handstand_epilogue_ref.py over the fixture, both fed the same f32-oracle record (physics capped at the kernel's 12 contacts);
the contact band (4 x the largest float32-float64 difference of a pair distance over the fixture, not below the bound
tests/test_planeprim_gpu.py enforces), inside which no pair of any state may lie; and the share of the orientation bound that
reconstructing R[0], R[3] costs where the desired forward vector has x and y."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import handstand_epilogue_cases as CS
import handstand_epilogue_ref as R
from oracle import oracle as O
from rsr_mjx_amd import prng
from rsr_mjx_amd.envs import config
from rsr_mjx_amd.mjcf import CompiledModel
from rsr_mjx_amd.model import model_fields, pack_blob

f32 = np.float32
SEED, POOL, NCAND = 2025, 96, 12000
OUT = os.path.join(ROOT, "tests", "golden", "handstand_epilogue_states.npz")
TOL = os.path.join(ROOT, "tests", "golden", "handstand_epilogue_tolerances.json")
PER_CLASS = 10


def go2_model():
    return config.go2_apply_overrides(CompiledModel.load(os.path.join(ROOT, "rsr_mjx_amd", "assets", "go2_full.npz")), config.HANDSTAND_DEFAULT_CONFIG)


def variant_oracle(model, task, name, precision="f32", auto_reset=None, quiet=False):
    f = model_fields(model)
    f.update(CS.variant_fields(model, task, name, auto_reset, quiet)[1])
    return O.Oracle(pack_blob(f), precision)


def oracle_step(orc, fx, cap=CS.NCON_CAP):
    """one oracle step from the fixture's records, the physics capped at `cap` contacts: (before, after) oracle states"""
    n = len(fx["qpos"])
    st = orc.new_state(n)
    orc.set_ncon_cap(cap)
    orc.reset(st, fx["keys"])
    for k in CS.RECORD:
        st[k][...] = fx[k].reshape(st[k].shape)
    before = {k: (v.copy() if v is not None else None) for k, v in st.items()}
    orc.step(st, fx["action"])
    orc.set_ncon_cap(1 << 20)
    return before, st


def stepped(model, task, name, precision, fx, cap=CS.NCON_CAP):
    """One step of the fixture under a variant: (K, before, after, quiet twin's after, phys).  The physics results of the envs AutoReset
    restored come from the variant's twin without AutoReset."""
    K = CS.variant_constants(model, task, name)
    before, after = oracle_step(variant_oracle(model, task, name, precision), fx, cap)
    _, quiet = oracle_step(variant_oracle(model, task, name, precision, quiet=True), fx, cap)
    src, qsrc = after, quiet
    if K["autoreset"]:
        _, src = oracle_step(variant_oracle(model, task, name, precision, auto_reset=False), fx, cap)
        _, qsrc = oracle_step(variant_oracle(model, task, name, precision, auto_reset=False, quiet=True), fx, cap)
    return K, before, after, quiet, CS.phys_of(K, model, src, qsrc, fx, flags_from=after["metrics"])


def _quat(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def _tilt_to(up2, rng, n):
    """quaternions whose up vector has the given z (a roll about x by acos(up2), then a random yaw in front)"""
    out = np.zeros((n, 4))
    for e in range(n):
        a = np.arccos(up2[e]) * (1 if e % 2 else -1)
        out[e] = R.quat_mul(_quat(0, 0, rng.uniform(-3, 3))[None], _quat(a, 0, 0)[None])[0]
    return out


def pair_groups(model):
    """0 trunk, 1 hip, 2 thigh, 3 calf, 4 foot, per collision pair"""
    names = {v: k for k, v in model.names["geom"].items()}
    g = []
    for p in model.arrays["pair_geom2"]:
        nm = names[int(p)]
        g.append(1 if "hip" in nm else 2 if "thigh" in nm else 3 if "calf" in nm else 4 if nm in ("FR", "FL", "RR", "RL") else 0)
    return np.array(g, np.int8)


def contact_data(o64, qpos):
    """the float64 oracle's forward pass at each pose, cap off: least point distance per pair; whether a penetrating point of the pair
    is among the first NCON_CAP in pair order / beyond them; the number of penetrating points"""
    n = len(qpos)
    dist, seen, cut, npen = np.zeros((n, 30)), np.zeros((n, 30), np.int8), np.zeros((n, 30), np.int8), np.zeros(n, np.int16)
    o64.set_ncon_cap(1 << 20); o64.set_cull(True)
    for e in range(n):
        q = qpos[e].astype(np.float64)
        o64.forward(q, np.zeros(18), q[7:])
        dist[e] = o64.get("pair_dist")
        c = o64.get("contacts").reshape(-1, 10)
        pen = c[c[:, 0] < 0, 9].astype(int)                          # pairs of the penetrating points, in pair order
        npen[e] = len(pen)
        seen[e, pen[:CS.NCON_CAP]] = 1
        cut[e, pen[CS.NCON_CAP:]] = 1
    return dist, seen, cut, npen


def constructed(model, o64, rng, want):
    """{class: [qpos, ...]} by the construction of the module docstring.  `want`: {class: predicate(touch [30] bool, order: pairs of the
    penetrating points in pair order)}."""
    A = model.arrays
    home = A["key_qpos"][model.names["key"]["home"]].astype(np.float64)
    lo, hi = A["jnt_range"][1:, 0], A["jnt_range"][1:, 1]
    got = {k: [] for k in want}
    o64.set_ncon_cap(1 << 20); o64.set_cull(False)
    for e in range(NCAND):
        q = home.copy()
        q[2] = 1.0
        fam = e % 3
        if fam == 0:                                                 # any orientation the up vector allows, any joint angles
            q[3:7] = _quat(rng.uniform(-1.6, 1.6), rng.uniform(-1.2, 1.2), rng.uniform(-3, 3))
            q[7:] = rng.uniform(lo * 0.85 + hi * 0.15, hi * 0.85 + lo * 0.15)
        elif fam == 1:                                               # lying: the floor poses' tilt and joint noise, doubled
            t = rng.normal(size=4) * 0.3 + np.array([1, 0, 0, 0])
            q[3:7] = t / np.linalg.norm(t)
            q[7:] = home[7:] + rng.normal(size=12) * 0.4
        else:                                                        # lying on one end: pitched, one pair of legs folded, the other random
            q[3:7] = _quat(rng.normal() * 0.25, rng.uniform(-0.7, 0.7), rng.uniform(-3, 3))
            q[7:] = home[7:] + rng.normal(size=12) * 0.3
            legs = (0, 1) if e % 2 else (2, 3)
            for l in legs:
                q[7 + 3 * l + 1] = rng.uniform(-0.5, 3.5); q[7 + 3 * l + 2] = rng.uniform(-2.6, -1.0)
        q[7:] = np.clip(q[7:], lo + 0.02, hi - 0.02)
        if 1 - 2 * (q[4] ** 2 + q[5] ** 2) < -0.1:
            continue
        q = q.astype(f32).astype(np.float64)
        o64.forward(q, np.zeros(18), q[7:])
        c = o64.get("contacts").reshape(-1, 10)
        d, pair = c[:, 0], c[:, 9].astype(int)
        srt = np.sort(d)
        for k in range(1, min(len(srt), 36)):
            gap = srt[k] - srt[k - 1]
            if gap < 2.5 * CS.POSE_MARGIN:
                continue
            s = srt[k - 1] + 1.2 * CS.POSE_MARGIN                    # k points penetrate, the shallowest by 1.2 margins
            order = pair[d - s < 0]
            touch = np.zeros(30, bool); touch[order] = True
            for name, pred in want.items():
                if len(got[name]) < want[name].need and pred(touch, order):
                    qq = q.copy(); qq[2] = 1.0 - s
                    got[name].append(qq.astype(f32))
                    break
            else:
                continue
            break                                                    # one state per candidate
    o64.set_cull(True)
    return got


def _want(model):
    """the contact classes of both tasks in terms of a penetrating set"""
    grp = pair_groups(model)
    f = model_fields(model)
    cls = {t: R.constants(config.handstand_env_fields(model, config.HANDSTAND_DEFAULT_CONFIG, variant=v), model)["pair_class"] for t, v in CS.TASKS.items()}
    want = {}

    def add(name, pred, need=PER_CLASS):
        pred.need = need
        want[name] = pred

    for t, pc in cls.items():
        unw, feet = pc == 1, np.flatnonzero(pc == 2)
        for g in ("thigh", "hip", "calf"):                           # the rarest first: a candidate serves the first class it fits
            gi = CS.GROUPS[g]
            add(f"{t}/unwanted_{g}", (lambda unw, gi: lambda touch, order: (touch & unw & (grp == gi)).any() and not (touch & unw & (grp != gi)).any()
                                      and len(order) <= 8)(unw, gi))
        for k in (0, 1):
            add(f"{t}/cost_foot{k}", (lambda unw, a, b: lambda touch, order: touch[a] and not touch[b] and not (touch & unw).any() and len(order) <= 6)(unw, feet[k], feet[1 - k]))
        for c, nm in ((1, "unwanted"), (2, "foot")):
            mine = pc == c
            def late(touch, order, mine=mine):
                return len(order) > CS.NCON_CAP and (touch & mine).sum() == 1 and not mine[order[:CS.NCON_CAP]].any()
            def early(touch, order, mine=mine):
                return len(order) > CS.NCON_CAP and (touch & mine).sum() == 1 and not mine[order[CS.NCON_CAP:]].any()
            if not (t == "Go2Handstand" and c == 1):
                add(f"{t}/cap_{nm}_late", late, PER_CLASS + 2)
            add(f"{t}/cap_{nm}_early", early, PER_CLASS + 2)
    return want


def generate(verbose=False):
    O.build()
    m = go2_model()
    rng = np.random.default_rng(SEED)
    home = m.arrays["key_qpos"][m.names["key"]["home"]].astype(f32)
    K0 = CS.variant_constants(m, "Go2Handstand", "shipped_autoreset")
    soft = K0["soft"]
    # ---- rollout pool: half of the envs start from the crouch ----
    f = model_fields(m)
    c = config._merge(CS.variant_config("shipped_autoreset"), {"init_from_crouch": 0.5})
    f.update(config.handstand_env_fields(m, c, CS.EPISODE_LENGTH, True, variant="handstand"))
    orc = O.Oracle(pack_blob(f), "f32")
    orc.set_ncon_cap(CS.NCON_CAP)
    st = orc.new_state(POOL)
    orc.reset(st, prng.split(prng.PRNGKey(SEED), POOL))
    crouched = st["qpos"][:, 2] < 0.1
    snaps = []
    for t in range(30):
        a = np.clip(rng.normal(size=(POOL, 12)) * 0.3, -1, 1).astype(f32)
        orc.step(st, a)
        if t in (11, 29):
            snaps.append({k: st[k].copy() for k in CS.RECORD + ("priv_obs",)})
    orc.set_ncon_cap(1 << 20)
    allp = {k: np.concatenate([p[k] for p in snaps]) for k in snaps[0]}
    up2 = 1 - 2 * (allp["qpos"][:, 4] ** 2 + allp["qpos"][:, 5] ** 2)
    ok = (allp["done"] == 0) & (up2 > 0.9) & (allp["qpos"][:, 2] > 0.2) & ~np.tile(crouched, 2)
    pool = {k: v[ok] for k, v in allp.items()}
    low = {k: v[np.tile(crouched, 2)] for k, v in allp.items()}          # the crouch starts, wherever they got to
    npool = len(pool["qpos"])
    assert npool >= 32 and len(low["qpos"]) >= 16, (npool, len(low["qpos"]))
    cursor, chunks, names = [0], [], []

    def take(n):
        idx = (cursor[0] + np.arange(n)) % npool
        cursor[0] += n
        r = {k: v[idx].copy() for k, v in pool.items()}
        r["action"] = np.clip(rng.normal(size=(n, 12)) * 0.3, -1, 1).astype(f32)
        return r

    def add(name, r):
        r["cls"] = np.full(len(r["qpos"]), len(names), np.int32)
        names.append(name)
        chunks.append(r)

    def still(r):
        """at rest, the motor targets where the joints are, no episode behind it"""
        r["qvel"][:] = 0; r["qacc_warmstart"][:] = 0
        r["ctrl"][:] = r["qpos"][:, 7:]
        r["action"][:] = 0

    def posed(qpos):
        r = take(len(qpos))
        r["qpos"][:] = np.asarray(qpos, f32)
        still(r)
        return r

    def in_air(r, z=0.7):
        r["qpos"][:, 2] = f32(z)
        return r

    # ---- rollout states as they are, and the crouch starts ----
    add("rollout", take(24))
    r = {k: v[:16].copy() for k, v in low.items()}
    r["action"] = np.clip(rng.normal(size=(16, 12)) * 0.3, -1, 1).astype(f32)
    r["done"][:] = 0
    add("crouch_rollout", r)
    # ---- floor poses (tests/test_handstand.py) ----
    n = 24
    r = take(n)
    r["qpos"][:] = home
    r["qpos"][:, 2] = np.linspace(0.06, 0.2, n).astype(f32)
    tilt = rng.normal(size=(n, 4)).astype(f32) * 0.15 + np.array([1, 0, 0, 0], f32)
    r["qpos"][:, 3:7] = tilt / np.linalg.norm(tilt, axis=1, keepdims=True)
    r["qpos"][:, 7:] += rng.normal(size=(n, 12)).astype(f32) * 0.2
    still(r)
    add("floor_poses", r)
    # ---- constructed contact classes ----
    o64 = variant_oracle(m, "Go2Handstand", "shipped_autoreset", "f64")
    want = _want(m)
    got = constructed(m, o64, rng, want)
    if verbose:
        print({k: len(v) for k, v in got.items()})
    for name, qs in got.items():
        assert len(qs) >= want[name].need, (name, len(qs))
        add(name, posed(np.array(qs)))
    # ---- the up vector: far below, and just on either side of -0.25; in the air, no contact ----
    r = in_air(take(10)); still(r); r["qpos"][:, 3:7] = _tilt_to(rng.uniform(-0.95, -0.4, 10), rng, 10).astype(f32); add("up_far", r)
    for nm, sg in (("up_just_below", -1), ("up_just_above", 1)):
        r = in_air(take(12)); still(r)
        r["qpos"][:, 3:7] = _tilt_to(-0.25 + sg * rng.uniform(0.002, 0.007, 12), rng, 12).astype(f32)
        add(nm, r)
    # ---- energy: fast joints against a motor target half a radian away ----
    r = in_air(take(12))
    r["qvel"][:, 6:] = (rng.choice([-1.0, 1.0], (12, 12)) * rng.uniform(7, 9, (12, 12))).astype(f32)
    r["ctrl"][:] = r["qpos"][:, 7:] + (rng.choice([-1.0, 1.0], (12, 12)) * 0.5).astype(f32)
    r["action"][:] = 0
    add("energetic", r)
    # ---- imu height at or above z_des ----
    r = in_air(take(10), 0.9); add("high", r)
    # ---- soft joint limits: a joint 0.03 beyond, held there, robot in the air ----
    for kind, ji in (("hip", 0), ("thigh", 1), ("calf", 2)):
        for side in ("low", "high"):
            r = in_air(take(10)); still(r)
            for e in range(10):
                j = 3 * (e % 4) + ji
                r["qpos"][e, 7 + j] = soft[j] - f32(0.03) if side == "low" else soft[12 + j] + f32(0.03)
            still(r)
            add(f"limit_{kind}_{side}", r)
    # ---- reward total: standing, at rest, the action repeated (positive); torques and a changed action (negative) ----
    r = take(12); r["action"] = r["info_go2"][:, R.LAST_ACT:R.LAST_ACT + 12].copy(); add("reward_calm", r)
    r = take(12); r["ctrl"][:] += (rng.choice([-1.0, 1.0], (12, 12)) * 0.4).astype(f32); add("reward_torques", r)
    # ---- wrappers ----
    r = take(10); r["info_steps"][:] = CS.EPISODE_LENGTH - 1; add("last_step", r)
    r = in_air(take(10)); still(r); r["info_steps"][:] = CS.EPISODE_LENGTH - 1
    r["qpos"][:, 3:7] = _tilt_to(rng.uniform(-0.95, -0.4, 10), rng, 10).astype(f32); add("last_step_done", r)
    r = take(10); r["info_episode_done"][:] = 1; add("prev_episode_done", r)
    r = take(10); r["done"][:] = 1; r["info_episode_done"][:] = 1; r["info_steps"][:] = rng.integers(3, 400, 10); add("prev_done", r)

    fx = {k: np.concatenate([c[k] for c in chunks]).astype(f32) for k in CS.RECORD + ("action",)}
    fx["cls"] = np.concatenate([c["cls"] for c in chunks])
    n = len(fx["cls"])
    fx["keys"] = prng.split(prng.PRNGKey(SEED + 1), n)
    fx["class_names"] = np.array(names)
    fx["info_go2"][:, R.RNG:R.RNG + 2] = prng.split(prng.PRNGKey(SEED + 2), n).view(f32)
    fx["pair_group"] = pair_groups(m)
    # ---- the float64 contact data of every state, and the band no pair may lie in ----
    dist, seen, cut, npen = contact_data(o64, fx["qpos"])
    o32 = variant_oracle(m, "Go2Handstand", "shipped_autoreset", "f32")
    d32 = contact_data(o32, fx["qpos"])[0]
    near = np.abs(dist) < 1.0                                        # (a pair a metre away decides nothing)
    measured = float(np.abs(d32 - dist)[near].max())
    band = max(4 * measured, CS.PLANEPRIM_DIST_BOUND)
    keep = ~(np.abs(dist) < band).any(1)
    if verbose:
        print("max |d32 - d64| %.3e, band %.3e, %d states inside it dropped" % (measured, band, int((~keep).sum())))
    for k in list(fx):
        if k not in ("class_names", "pair_group"):
            fx[k] = fx[k][keep]
    fx["pair_dist"], fx["seen12"], fx["cut12"], fx["npen"] = dist[keep].astype(f32), seen[keep], cut[keep], npen[keep]
    assert ((fx["pair_dist"] < 0) == (dist[keep] < 0)).all()
    fx["contact_band"] = np.array([measured, band])
    return fx


def tolerances(fx):
    """{task: {variant: {quantity: max |ref32 - ref64| over the fixture}}}, both references fed the same f32-oracle record; the contact
    band; and per task the reconstruction's share of the orientation bound"""
    m = go2_model()
    worst = {"contact_band": {"max_f32_f64_pair_dist": float("%.3e" % fx["contact_band"][0]), "planeprim_dist_bound": CS.PLANEPRIM_DIST_BOUND,
                              "band": float("%.3e" % fx["contact_band"][1])}, "orientation_share": {}}
    for task in CS.TASKS:
        worst[task] = {}
        for name in CS.VARIANTS:
            K, before, after, quiet, phys = stepped(m, task, name, "f32", fx)
            pre = CS.before_of(before, fx["action"])
            r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
            q32, q64 = R.float_quantities(r32, K), R.float_quantities(r64, K)
            worst[task][name] = {nm: float("%.3e" % np.abs(q32[nm].astype(np.float64) - q64[nm]).max()) for nm in sorted(q64)}
            if K["general_fwd"]:
                # the float64 oracle's own orientation metric (its R is exact) against the reference's on the same step
                K, before, after, quiet, phys = stepped(m, task, name, "f64", fx)
                live = ~((after["done"].reshape(-1) != 0) & K["autoreset"])
                r = R.step(K, CS.before_of(before, fx["action"]), phys, np.float64)
                worst["orientation_share"][task] = float("%.3e" % np.abs(r["metrics"][:, R.HM_ORIENT] - after["metrics"][:, R.HM_ORIENT].astype(np.float64))[live].max())
    return worst


def main():
    fx = generate(verbose=True)
    np.savez_compressed(OUT, **fx)
    print("%d states, %d bytes; classes: %s" % (len(fx["cls"]), os.path.getsize(OUT), dict(zip(*np.unique(fx["cls"], return_counts=True)))))
    tol = tolerances(fx)
    json.dump(tol, open(TOL, "w"), indent=1)
    print(json.dumps({k: tol[k] for k in ("contact_band", "orientation_share")}))


if __name__ == "__main__":
    main()
