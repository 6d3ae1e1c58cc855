"""States for the by-branch test of the Airbot step's prologue / epilogue (tests/test_airbot_epilogue.py and _gpu.py; classes and variants
in tests/airbot_epilogue_cases.py).  Seeded, CPU only, per kind (cube, sf, tshape): the f32 oracle is rolled out from its reset
states to get a pool of settled arms, then the record words a step reads are edited per class.  Words the physics does not read
(info_target_pos for the reward, info_new_*_pos, info_target_*_pos, the stale xpos / site_xpos the aim is taken from, info_last_action,
the wrapper words) are set exactly; arm poses for the site-z, health and workspace classes are searched for with one oracle step per
candidate; words that are relative to where the step's physics ends up (target at 2 mm from the cube, push position inside the dead
zone, T-shape targets along the block's axis) are set from a first oracle pass and, where the target moves the wrist aim (cube, sf),
settled by two more.  Every gate has states within a few millimetres on both sides of it.
Stored is what a step reads, the reset keys that give every env its cached first state, the action and the class each state was
built for -- float32, compressed: tests/golden/airbot_epilogue_states.npz, keys "<kind>__<field>".

The script also writes tests/golden/airbot_epilogue_tolerances.json: per kind, variant, compared quantity and fixture class,
max |ref32 - ref64| of tests/airbot_epilogue_ref.py, both fed the same f32-oracle record (zeros are left out); xita also per angle
class ("xita@aligned", "xita@generic"); and per kind the distance between a float32 and a float64 kinematics of the fixture's poses
("kinematics")."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import airbot_epilogue_cases as CS
import airbot_epilogue_ref as R
from oracle import oracle as O
from rsr_mjx_amd import prng
from rsr_mjx_amd.mjcf import CompiledModel
from rsr_mjx_amd.model import model_fields, pack_blob

f32 = np.float32
SEED, POOL, TRIES = 2025, 64, 1536
OUT = os.path.join(ROOT, "tests", "golden", "airbot_epilogue_states.npz")
TOL = os.path.join(ROOT, "tests", "golden", "airbot_epilogue_tolerances.json")
ARM_LANES = [0, 1, 2, 4, 5]                   # actuator -> arm joint (actuator_trnid of the three models)


def model(kind):
    return CompiledModel.load(os.path.join(ROOT, "rsr_mjx_amd", "assets", CS.ASSET[kind]))


def variant_oracle(m, kind, name, precision="f32", auto_reset=None):
    f = model_fields(m)
    f.update(CS.variant_fields(m, kind, name, auto_reset))
    return O.Oracle(pack_blob(f), precision)


def oracle_step(orc, kind, fx):
    """one oracle step from a kind's fixture records: (before, after) oracle states"""
    n = len(fx["qpos"])
    st = orc.new_state(n)
    orc.reset(st, fx["keys"])
    for k in CS.RECORD[kind]:
        st[k][...] = fx[k].reshape(st[k].shape)
    before = {k: (v.copy() if v is not None else None) for k, v in st.items()}
    orc.step(st, fx["action"])
    return before, st


def _dirs(rng, n, lo=0.0, hi=2 * np.pi):
    a = rng.uniform(lo, hi, n)
    return np.stack([np.cos(a), np.sin(a)], 1)


def _unit3(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def generate_kind(kind, rng):
    m = model(kind)
    ts, sf = kind == "tshape", kind == "sf"
    K = CS.variant_constants(m, kind, "plain")
    ids, lo, hi = K["ids"], K["lo"], K["hi"]
    jq = ids[(R.TID_JOINTQ if ts else R.ID_JOINTQ):][:6]
    site = ids[R.TID_SITE if ts else R.ID_SITE]
    body = ids[R.TID_T if ts else R.ID_CUBE]
    A = m.arrays
    bq = int(A["jnt_qposadr"][A["body_jntadr"][body]])            # the pushed body's free joint
    new_pos, fields = R.NEW_POS[kind], CS.RECORD[kind]
    orc = variant_oracle(m, kind, "plain")
    orc.set_ncon_cap(CS.NCON_CAP[kind])
    st = orc.new_state(POOL)
    orc.reset(st, prng.split(prng.PRNGKey(SEED), POOL))
    for t in range(10):
        orc.step(st, np.clip(rng.normal(size=(POOL, 5)) * 0.3, -1, 1).astype(f32))
    assert (st["done"] == 0).all()
    pool = {k: st[k].copy() for k in fields}
    pool["qvel"][:] = 0; pool["qacc_warmstart"][:] = 0
    cursor = [0]
    chunks, names = [], []

    def hold(r):
        r["ctrl"][:] = r["qpos"][:, [jq[j] for j in ARM_LANES]]

    def take(n):
        idx = (cursor[0] + np.arange(n)) % POOL
        cursor[0] += n
        r = {k: v[idx].copy() for k, v in pool.items()}
        r["action"] = np.clip(rng.normal(size=(n, 5)) * 0.6, -1, 1).astype(f32)
        r["metrics"][:] = rng.uniform(-1, 1, r["metrics"].shape).astype(f32)           # the kept word must pass through
        r["info_steps"][:] = rng.integers(0, 4, n).astype(f32).reshape(r["info_steps"].shape)
        em = r["info_episode_metrics"]
        em[:] = rng.uniform(0, 30, em.shape).astype(f32)
        em[:, 1] = r["info_steps"].reshape(n)
        if sf:
            r["info_last_action"][:] = rng.uniform(-1, 1, n).astype(f32).reshape(r["info_last_action"].shape)
        # directives, resolved against an oracle pass (nan: leave the word as it is)
        r["_tp_off"] = np.full((n, 3), np.nan); r["_np_off"] = np.full((n, 2), np.nan)
        r["_tb_off"] = np.full((n, 3), np.nan); r["_tv_off"] = np.full((n, 3), np.nan); r["_axis_k"] = np.full(n, np.nan)
        hold(r)
        return r

    def add(name, r):
        r["cls"] = np.full(len(r["qpos"]), len(names), np.int32)
        names.append(name)
        chunks.append(r)

    def step_of(r):
        fx = {k: r[k] for k in fields}
        fx["keys"] = prng.split(prng.PRNGKey(SEED + 5), len(r["qpos"])); fx["action"] = r["action"]
        return oracle_step(orc, kind, fx)[1]

    def search(perturb, pred, n):
        """the first n of TRIES perturbed pool states whose oracle step satisfies pred (and stays finite, within contact capacity)"""
        r = take(TRIES)
        perturb(r)
        hold(r)
        a = step_of(r)
        sp, bp = a["site_xpos"][:, site], a["xpos"][:, body]
        ok = pred(sp, bp) & np.isfinite(a["qpos"]).all(1) & (a["stats"][:, 3] == 0) & (np.abs(a["qvel"]).max(1) < 50)
        w = np.flatnonzero(ok)[:n]
        assert len(w) == n, (kind, "pose search found", len(w), "of", n)
        return {k: v[w].copy() for k, v in r.items()}

    def stale_aim(r, dxy):
        """the words the wrist aim is taken from, so that (dx, dy) = dxy in float32"""
        dxy = np.asarray(dxy, np.float64)
        if ts:
            sx = r["site_xpos"].reshape(len(dxy), -1, 3)
            sx[:, ids[R.TID_TAIL], :2] = (sx[:, site, :2].astype(np.float64) + dxy).astype(f32)
        else:
            xp = r["xpos"].reshape(len(dxy), -1, 3)
            xp[:, body, :2] = (r["info_target_pos"][:, :2].astype(np.float64) - dxy).astype(f32)

    def lower(dj):
        def f(r):
            r["qpos"][:, jq[1]] += rng.uniform(*dj, len(r["qpos"])).astype(f32)
        return f

    # ---- generic ----
    add("generic", take(16))
    # ---- prologue: clamps ----
    for i in range(3):
        for side in ("low", "high"):
            r = take(8)
            r["ctrl"][:, i] = (lo[i] + f32(0.005)) if side == "low" else (hi[i] - f32(0.005))
            r["action"][:, i] = -1 if side == "low" else 1
            add(f"ctrl{i}_{side}", r)
    r = take(8); r["qpos"][:, jq[1]] = f32(-0.1); r["qpos"][:, jq[2]] = rng.uniform(0.5, 0.8, 8).astype(f32); add("ctrl3_low", r)
    r = take(8); r["qpos"][:, jq[1]] = f32(-2.9); r["qpos"][:, jq[2]] = -rng.uniform(0.45, 0.6, 8).astype(f32); add("ctrl3_high", r)
    r = take(8); stale_aim(r, 0.1 * _dirs(rng, 8, -2.9, -2.3)); add("ctrl4_high", r)
    r = take(8); stale_aim(r, 0.1 * _dirs(rng, 8, 2.9, 3.1)); r["ctrl"][:, 0] = f32(-2.2); add("ctrl4_low", r)
    # ---- prologue: aim ----
    for k in range(4):
        r = take(8); stale_aim(r, rng.uniform(0.02, 0.2, (8, 1)) * _dirs(rng, 8, k * np.pi / 2 + 0.15, (k + 1) * np.pi / 2 - 0.15))
        add(f"aim_quadrant{k + 1}", r)
    r = take(10); stale_aim(r, np.stack([-rng.uniform(2e-6, 8e-6, 10), rng.uniform(1e-6, 1e-4, 10) * np.where(np.arange(10) % 2, 1, -1)], 1))
    add("aim_epsilon_flips_sign", r)
    r = take(8); stale_aim(r, np.stack([-rng.uniform(0.02, 0.2, 8), np.zeros(8)], 1)); add("aim_edge_dy0_dx_negative", r)
    r = take(8)                                                       # dx = -1e-5f exactly, dy = 0: both atan2f arguments are zero
    if ts:
        sx = r["site_xpos"].reshape(8, -1, 3)
        sx[:, site, :2] = 0; sx[:, ids[R.TID_TAIL], 0] = f32(-0.00001); sx[:, ids[R.TID_TAIL], 1] = 0
    else:
        r["xpos"].reshape(8, -1, 3)[:, body, :2] = 0
        r["info_target_pos"][:, 0] = f32(-0.00001); r["info_target_pos"][:, 1] = 0
    add("aim_edge_both_zero", r)
    if sf:
        for nm, d in (("hold_taken", (0.004, 0.02)), ("hold_near_inside", (0.0285, 0.0296)), ("hold_near_outside", (0.0304, 0.0315))):
            r = take(10)
            v = _unit3(rng, 10) * rng.uniform(*d, (10, 1))
            r["xpos"].reshape(10, -1, 3)[:, body] = (r["info_target_pos"].astype(np.float64) - v).astype(f32)
            add(nm, r)
    # ---- epilogue: distance to the target (cube / sf), relative to where the cube ends up ----
    if not ts:
        bands = {"btd_below": (0.0005, 0.0025) if sf else (0.001, 0.004)}
        if sf:
            bands["btd_sf_band"] = (0.0035, 0.0045)
        bands["btd_just_above_005"] = (0.0055, 0.007)
        for nm, d in bands.items():
            r = take(12); r["_tp_off"][:] = _unit3(rng, 12) * rng.uniform(*d, (12, 1)); add(nm, r)
        for k in range(4):
            r = take(8); r["_tp_off"][:, :2] = rng.uniform(0.03, 0.2, (8, 1)) * _dirs(rng, 8, k * np.pi / 2 + 0.15, (k + 1) * np.pi / 2 - 0.15)
            r["_tp_off"][:, 2] = 0
            add(f"new_cube_pos_quadrant{k + 1}", r)
    # ---- epilogue: site height gates (arm poses found by search) ----
    # (each gate gets states within 8 mm on either side of it: a threshold off by a centimetre must not pass)
    win = lambda lo_, hi_: (lambda z: (z > lo_) & (z < hi_))
    gz, mz = CS.GATE_Z[kind], float(K["W"][3])
    zs = {"site_z_just_below_gate": win(gz - 0.008, gz - 0.001), "site_z_just_above_gate": win(gz + 0.001, gz + 0.008),
          "min_z_just_below": win(mz - 0.008, mz - 0.001), "min_z_just_above": win(mz + 0.001, mz + 0.008)}
    if ts:
        zs.update({"z_reward_just_below_0805": win(0.797, 0.804), "z_reward_just_above_0805": win(0.806, 0.813)})
    for nm, zp in zs.items():
        add(nm, search(lower((-0.3, 0.4)), lambda sp, bp, zp=zp: zp(sp[:, 2]), 10))
    # ---- epilogue: push-position dead zone, relative to where the site ends up ----
    dead = 0.02 if ts else 0.042
    r = take(12); r["_np_off"][:] = rng.uniform(0.1 * dead, 0.9 * dead, (12, 1)) * _dirs(rng, 12); add("s2c_inside", r)
    r = take(12); r["_np_off"][:] = rng.uniform(dead + 0.002, dead + 0.008, (12, 1)) * _dirs(rng, 12); add("s2c_just_outside", r)
    # ---- epilogue: workspace bounds (sf), termination ----
    def fell(r, z=(0.25, 0.35)):
        n = len(r["qpos"])
        r["qpos"][:, bq:bq + 2] = np.array([1.5, 1.0], f32) + rng.uniform(-0.05, 0.05, (n, 2)).astype(f32)
        r["qpos"][:, bq + 2] = rng.uniform(*z, n).astype(f32)
    if sf:
        def swing(r, yaw=(-3.1, 2.05)):
            n = len(r["qpos"])
            r["qpos"][:, jq[0]] = rng.uniform(*yaw, n).astype(f32)
            r["qpos"][:, jq[1]] = rng.uniform(-2.2, -0.3, n).astype(f32)
            r["qpos"][:, jq[2]] = rng.uniform(0.0, 2.4, n).astype(f32)
        up = lambda sp: (sp[:, 2] > 0.86) & (sp[:, 0] <= 0.99)
        add("oob_x_low_alone", search(lambda r: swing(r, (-3.1, -2.75)), lambda sp, bp: up(sp) & (sp[:, 0] < -0.61) & (sp[:, 0] > -0.70) & (np.abs(sp[:, 1]) < 0.29), 8))
        add("oob_y_high_alone", search(swing, lambda sp, bp: up(sp) & (sp[:, 0] > -0.59) & (sp[:, 1] > 0.31) & (sp[:, 1] < 0.40), 8))
        add("oob_y_low_alone", search(swing, lambda sp, bp: up(sp) & (sp[:, 0] > -0.59) & (sp[:, 1] < -0.31) & (sp[:, 1] > -0.40), 8))
        add("oob_cube_z_alone", search(lambda r: (lower((0.05, 0.2))(r), fell(r, (0.56, 0.59))), lambda sp, bp: (sp[:, 2] > 0.803) & (bp[:, 2] < 0.595), 8))
        r = take(10); fell(r, (0.61, 0.64)); add("cube_just_above_06", r)
    else:
        r = take(10); fell(r); add("done_T_fell" if ts else "done_cube_fell", r)
        r = take(10); fell(r, (0.56, 0.59)); add("fell_just_below_06", r)
        r = take(10); fell(r, (0.61, 0.64)); add("fell_just_above_06", r)
    # ---- T-shape: geom distances, angle, new_T_pos ----
    if ts:
        for nm, (sb, sv) in (("dis_base_snapped_only", (1, 0)), ("dis_vert_snapped_only", (0, 1)), ("dis_both_snapped", (1, 1))):
            r = take(10)
            if sb: r["_tb_off"][:] = _unit3(rng, 10) * rng.uniform(0.0005, 0.004, (10, 1))
            if sv: r["_tv_off"][:] = _unit3(rng, 10) * rng.uniform(0.0005, 0.004, (10, 1))
            add(nm, r)
        r = take(10); r["_tb_off"][:] = _unit3(rng, 10) * rng.uniform(0.0055, 0.007, (10, 1)); r["_tv_off"][:] = _unit3(rng, 10) * rng.uniform(0.0055, 0.007, (10, 1))
        add("dis_just_above_005", r)
        for nm, sgn in (("cosine_clamped_plus1", 1.0), ("cosine_clamped_minus1", -1.0)):
            r = take(16)
            r["_tb_off"][:] = np.array([0.03, 0.02, 0.004]) + rng.uniform(-0.01, 0.01, (16, 3))
            r["_axis_k"][:] = sgn * rng.uniform(0.5, 2.0, 16)
            add(nm, r)
        ttail_xy = pool["site_xpos"].reshape(POOL, -1, 3)[0, ids[R.TID_TTAIL], :2].astype(np.float64)
        for k in range(4):
            r = take(8)
            want = ttail_xy - rng.uniform(0.03, 0.12, (8, 1)) * _dirs(rng, 8, k * np.pi / 2 + 0.2, (k + 1) * np.pi / 2 - 0.2)
            now = r["site_xpos"].reshape(8, -1, 3)[:, ids[R.TID_TAIL], :2].astype(np.float64)
            r["qpos"][:, bq:bq + 2] = (r["qpos"][:, bq:bq + 2].astype(np.float64) + want - now).astype(f32)
            add(f"new_T_pos_quadrant{k + 1}", r)
    # ---- wrappers ----
    r = take(10); r["done"][:] = 1; r["info_episode_done"][:] = 1; r["info_steps"][:] = 3; add("done_prev", r)
    r = take(10); r["info_episode_done"][:] = 1; add("prev_episode_done", r)
    for nm, prev in (("nan_sum_prev_done", 1), ("nan_sum_kept", 0)):
        r = take(8); r["info_episode_done"][:] = prev
        r["info_episode_metrics"][np.arange(8), np.arange(8) % r["info_episode_metrics"].shape[1]] = np.nan
        r["info_episode_metrics"][4:, 0] = np.nan
        add(nm, r)
    r = take(10); r["info_steps"][:] = CS.EPISODE_LENGTH - 1; add("last_step", r)
    r = take(10); r["info_steps"][:] = CS.EPISODE_LENGTH - 1
    if sf: r["_tp_off"][:] = _unit3(rng, 10) * rng.uniform(0.0005, 0.0025, (10, 1))
    else: fell(r)
    add("last_step_done", r)

    fx = {k: np.concatenate([c[k] for c in chunks]).astype(f32) for k in fields + ("action",)}
    di = {k: np.concatenate([c[k] for c in chunks]) for k in ("_tp_off", "_np_off", "_tb_off", "_tv_off", "_axis_k")}
    fx["cls"] = np.concatenate([c["cls"] for c in chunks])
    n = len(fx["cls"])
    fx["keys"] = prng.split(prng.PRNGKey(SEED + 1), n)
    fx["class_names"] = np.array(names)
    # ---- resolve the relative words against oracle passes (the target moves the wrist aim, hence three for cube / sf) ----
    for _ in range(1 if ts else 3):
        a = oracle_step(orc, kind, fx)[1]
        sp, bp = a["site_xpos"][:, site].astype(np.float64), a["xpos"][:, body].astype(np.float64)
        w = ~np.isnan(di["_np_off"][:, 0])
        fx[new_pos][w] = (sp[w, :2] + di["_np_off"][w]).astype(f32)
        if not ts:
            w = ~np.isnan(di["_tp_off"][:, 0])
            fx["info_target_pos"][w] = (bp[w] + di["_tp_off"][w]).astype(f32)
        else:
            tb0, tv0 = fx["info_target_base_pos"].astype(np.float64), fx["info_target_vertical_pos"].astype(np.float64)
            gb, gv = tb0 - a["obs"][:, 7:10].astype(np.float64), tv0 - a["obs"][:, 10:13].astype(np.float64)
            w = ~np.isnan(di["_tb_off"][:, 0])
            fx["info_target_base_pos"][w] = (gb[w] + di["_tb_off"][w]).astype(f32)
            w = ~np.isnan(di["_tv_off"][:, 0])
            fx["info_target_vertical_pos"][w] = (gv[w] + di["_tv_off"][w]).astype(f32)
            w = ~np.isnan(di["_axis_k"])
            fx["info_target_vertical_pos"][w] = (fx["info_target_base_pos"][w].astype(np.float64) + di["_axis_k"][w, None] * (gv[w] - gb[w])).astype(f32)
    return fx


def generate():
    O.build()
    out = {}
    for i, kind in enumerate(CS.KINDS):
        for k, v in generate_kind(kind, np.random.default_rng(SEED + i)).items():
            out[f"{kind}__{k}"] = v
    return out


def of_kind(fx, kind):
    return {k.split("__", 1)[1]: v for k, v in fx.items() if k.startswith(kind + "__")}


# ---- kinematics at float32 and float64 (the n_frames = 1 variant publishes the forward pass at the pre-step pose) ----
def kinematics(m, qpos, T):
    """(xpos [nbody, 3], site_xpos [nsite, 3], geom_xpos [ngeom, 3]) of one pose, every operation at precision T"""
    A = m.arrays
    c = lambda x: np.asarray(x, np.float64).astype(T)

    def qmul(a, b):
        return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], T)

    def rot(v, q):
        w, x, y, z = q
        two = T(2)
        M = np.array([[T(1) - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                      [two * (x * y + w * z), T(1) - two * (x * x + z * z), two * (y * z - w * x)],
                      [two * (x * z - w * y), two * (y * z + w * x), T(1) - two * (x * x + y * y)]], T)
        return M @ v

    q = c(qpos)
    nb = m.nbody
    xpos, xquat = np.zeros((nb, 3), T), np.zeros((nb, 4), T)
    xquat[:, 0] = 1
    for b in range(1, nb):
        p = A["body_parentid"][b]
        pos = xpos[p] + rot(c(A["body_pos"][b]), xquat[p])
        quat = qmul(xquat[p], c(A["body_quat"][b]))
        for k in range(A["body_jntnum"][b]):
            j = A["body_jntadr"][b] + k
            jt, qa = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j])
            if jt == 0:
                pos = q[qa:qa + 3].copy()
                quat = q[qa + 3:qa + 7] / np.sqrt((q[qa + 3:qa + 7] ** 2).sum())
            else:
                anchor = rot(c(A["jnt_pos"][j]), quat) + pos
                axis = c(A["jnt_axis"][j])
                d = q[qa] - c(A["qpos0"][qa])
                if jt == 3:
                    h = d / T(2)
                    quat = qmul(quat, np.concatenate([[np.cos(h)], np.sin(h) * axis / np.sqrt((axis * axis).sum())]).astype(T))
                    pos = anchor - rot(c(A["jnt_pos"][j]), quat)
                else:
                    pos = pos + rot(axis, quat) * d
        xpos[b], xquat[b] = pos, quat / np.sqrt((quat * quat).sum())
    sites = np.array([xpos[A["site_bodyid"][s]] + rot(c(A["site_pos"][s]), xquat[A["site_bodyid"][s]]) for s in range(m.nsite)], T)
    geoms = np.array([xpos[A["geom_bodyid"][g]] + rot(c(A["geom_pos"][g]), xquat[A["geom_bodyid"][g]]) for g in range(m.ngeom)], T)
    return xpos, sites, geoms


def kinematics_batch(m, qpos, T):
    out = [kinematics(m, q, T) for q in qpos]
    return tuple(np.stack([o[i] for o in out]).astype(np.float64) for i in range(3))


def tolerances(fx):
    """{kind: {variant: {quantity: {class: max |ref32 - ref64|}}, "kinematics": ...}}, both references fed the same f32-oracle record"""
    worst = {}
    for kind in CS.KINDS:
        m, f = model(kind), of_kind(fx, kind)
        names, cls = [str(s) for s in f["class_names"]], f["cls"]
        worst[kind] = {}
        for name in CS.VARIANTS:
            K = CS.variant_constants(m, kind, name)
            orc = variant_oracle(m, kind, name); orc.set_ncon_cap(CS.NCON_CAP[kind])
            before, after = oracle_step(orc, kind, f)
            if K["autoreset"]:                                      # the physics results come from the twin without AutoReset
                twin = variant_oracle(m, kind, name, auto_reset=False); twin.set_ncon_cap(CS.NCON_CAP[kind])
                after = oracle_step(twin, kind, f)[1]
            pre, phys = CS.before_of(before, f["action"]), CS.phys_of(kind, after)
            r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
            table = {}
            for nm, d in CS.distances(K, r32, r64).items():
                table[nm] = {names[c]: float("%.3e" % d[cls == c].max()) for c in range(len(names)) if d[cls == c].max() > 0}
                if nm == "xita":
                    xc = CS.xita_class(r64)
                    for i, cn in enumerate(CS.XITA_CLASSES):
                        table["xita@" + cn] = float("%.3e" % d[xc == i].max())
            worst[kind][name] = table
        k32, k64 = kinematics_batch(m, f["qpos"], np.float32), kinematics_batch(m, f["qpos"], np.float64)
        worst[kind]["kinematics"] = {nm: float("%.3e" % np.abs(a - b).max()) for nm, a, b in zip(("xpos", "site_xpos", "geom_xpos"), k32, k64)}
    return worst


def main():
    fx = generate()
    np.savez_compressed(OUT, **fx)
    print("%d bytes; states per kind: %s" % (os.path.getsize(OUT), {k: len(fx[k + "__cls"]) for k in CS.KINDS}))
    tol = tolerances(fx)
    json.dump(tol, open(TOL, "w"), indent=0, sort_keys=True)
    print("tolerance table: %d bytes" % os.path.getsize(TOL))


if __name__ == "__main__":
    main()
