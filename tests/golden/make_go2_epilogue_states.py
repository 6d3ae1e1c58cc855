"""States for the by-branch test of the Go2 joystick step's prologue / epilogue (tests/test_go2_epilogue.py and _gpu.py; classes and
variants in tests/go2_epilogue_cases.py).  Seeded, CPU only: the f32 oracle is rolled out from its reset states with small random
actions to get standing / shuffling robots, then info_go2, qpos and the action are edited per class.  Stored is what a step reads
(qpos, qvel, ctrl, warm start, time, info_go2, steps, done, Episode words, action), the reset keys that give every env its cached
first state, and the class each state was built for -- float32, compressed: tests/golden/go2_epilogue_states.npz.

The PRNG key of every state is drawn until each exponential timer draw the state can take (with and without the kick's split)
has t1 / dt at least 10 * HALF_MARGIN from a half-integer, so the new timer is the same integer at any precision.  The script also
writes tests/golden/go2_epilogue_tolerances.json: per variant and compared quantity, max |ref32 - ref64| of tests/go2_epilogue_ref.py
over the fixture, both fed the same f32-oracle record."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import go2_epilogue_cases as CS
import go2_epilogue_ref as R
from oracle import oracle as O
from rsr_mjx_amd import prng
from rsr_mjx_amd.envs import config
from rsr_mjx_amd.mjcf import CompiledModel
from rsr_mjx_amd.model import model_fields, pack_blob

f32 = np.float32
G = R.G
SEED, POOL = 2024, 96
OUT = os.path.join(ROOT, "tests", "golden", "go2_epilogue_states.npz")
TOL = os.path.join(ROOT, "tests", "golden", "go2_epilogue_tolerances.json")


def go2_model(task="flat"):
    return config.go2_apply_overrides(CompiledModel.load(os.path.join(ROOT, "rsr_mjx_amd", "assets", f"go2_{task}.npz")), config.GO2_DEFAULT_CONFIG)


def variant_oracle(model, name, precision="f32", auto_reset=None):
    f = model_fields(model)
    f.update(CS.variant_fields(model, name, auto_reset)[1])
    return O.Oracle(pack_blob(f), precision)


def oracle_step(orc, fx):
    """one oracle step from the fixture's records: (before, after) oracle states"""
    n = len(fx["qpos"])
    st = orc.new_state(n)
    orc.reset(st, fx["keys"])
    for k in CS.RECORD:
        st[k][...] = fx[k].reshape(st[k].shape)
    before = {k: (v.copy() if v is not None else None) for k, v in st.items()}
    orc.step(st, fx["action"])
    return before, st


def _rot_x(q, angle):
    """world-frame rotation about x in front of quaternion(s) q (w, x, y, z)"""
    c, s = np.cos(angle / 2), np.sin(angle / 2)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([c * w - s * x, c * x + s * w, c * y - s * z, c * z + s * y], 1)


def generate():
    O.build()
    m = go2_model()
    rng = np.random.default_rng(SEED)
    home = m.arrays["key_qpos"][m.names["key"]["home"]].astype(f32)
    K0 = CS.variant_constants(m, "d33_autoreset")
    soft = K0["soft"]
    orc = variant_oracle(m, "d33_autoreset")
    st = orc.new_state(POOL)
    orc.reset(st, prng.split(prng.PRNGKey(SEED), POOL))
    pool = []
    for t in range(30):
        a = np.clip(rng.normal(size=(POOL, 12)) * 0.3, -1, 1).astype(f32)
        orc.step(st, a)
        if t in (11, 29):
            pool.append({k: st[k].copy() for k in CS.RECORD + ("priv_obs",)})
    pool = {k: np.concatenate([p[k] for p in pool]) for k in pool[0]}
    ok = (pool["done"] == 0) & (pool["priv_obs"][:, 56] < -0.95) & (pool["info_go2"][:, G["STEPS_CMD"]] > 5)
    pool = {k: v[ok] for k, v in pool.items()}
    npool = len(pool["qpos"])
    assert npool >= 64, npool
    cursor = [0]
    chunks = []

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

    def hold(r, joints):
        """the delayed actions, the last action and the new one all ask for the pose the joints are in; they start at rest"""
        a = ((r["qpos"][:, 7:] - home[7:]) / f32(0.5)).astype(f32)
        for j in joints:
            for s in range(4):
                r["info_go2"][:, G["ACT_BUF"] + 12 * s + j] = a[:, j]
            r["info_go2"][:, G["LAST_ACT"] + j] = a[:, j]
            r["action"][:, j] = a[:, j]
            r["qvel"][:, 6 + j] = 0
            r["ctrl"][:, j] = r["qpos"][:, 7 + j]

    def lift(r, dz=0.3):
        r["qpos"][:, 2] += f32(dz)

    def retract(r, legs):
        for l in legs:
            r["qpos"][:, 7 + 3 * l + 1] = f32(1.5)
            r["qpos"][:, 7 + 3 * l + 2] = f32(-2.5)
        hold(r, [3 * l + i for l in legs for i in (1, 2)])

    def flip(r, angle):
        r["qpos"][:, 3:7] = _rot_x(r["qpos"][:, 3:7].astype(np.float64), np.asarray(angle, np.float64)).astype(f32)
        r["qpos"][:, 2] = f32(0.6)
        r["qvel"][:] *= f32(0.1)

    def unit(n):
        v = rng.normal(size=(n, 3)); v[:, 1] *= 0.3
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def touch_down(r, k):
        """the first k states (on the ground) come out of a swing: the feet_air_time / feet_height terms have something to gate"""
        r["info_go2"][:k, G["AIR"]:G["AIR"] + 4] = rng.uniform(0.15, 0.5, (k, 4)).astype(f32)
        r["info_go2"][:k, G["SWING"]:G["SWING"] + 4] = rng.uniform(0.03, 0.2, (k, 4)).astype(f32)
        r["info_go2"][:k, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4] = 0

    names = []
    # ---- command norm ----
    r = take(16); r["info_go2"][:, 0:3] = 0
    r["qpos"][8:, 2] += f32(0.3)                                  # half of them in the air: feet_off_ground_when_still counts four
    touch_down(r, 8)
    add("cmd_zero", r)
    # (0.0099 and 0.0101 less a float32 rounding would sit a hair inside the 1e-4 margin)
    for nm, val in (("cmd_just_still", 0.00989), ("cmd_just_moving", 0.01011)):
        r = take(12); r["info_go2"][:, 0:3] = (unit(12) * val).astype(f32); r["qpos"][6:, 2] += f32(0.3)
        touch_down(r, 6)
        add(nm, r)
    r = take(16); add("cmd_moving", r)
    # a command whose float32 norm is 0.01f exactly: neither gate is open
    exact = []
    for _ in range(20000):
        c = (unit(1)[0] * 0.01).astype(f32)
        if np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2], dtype=f32) == f32(0.01):
            exact.append(c)
        if len(exact) == 10:
            break
    if exact:
        r = take(len(exact)); r["info_go2"][:, 0:3] = np.array(exact, f32); r["qpos"][len(exact) // 2:, 2] += f32(0.3)
        touch_down(r, len(exact) // 2)
        add("cmd_exactly_threshold", r)
    # ---- command timer ----
    for k in (0, 1, 2):
        for done in (False, True):
            r = take(10); r["info_go2"][:, G["STEPS_CMD"]] = k
            if done:
                flip(r, np.pi + rng.uniform(-0.3, 0.3, 10))
            add(f"steps_cmd_{k}{'_done' if done else ''}", r)
    # ---- feet ----
    r = take(12); r["info_go2"][:, G["AIR"]:G["AIR"] + 4] = rng.uniform(0.05, 0.5, (12, 4)).astype(f32)
    r["info_go2"][:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4] = 0; r["info_go2"][:, G["CONTACT_T"]:G["CONTACT_T"] + 4] = 0
    r["info_go2"][:, G["SWING"]:G["SWING"] + 4] = rng.uniform(0.03, 0.2, (12, 4)).astype(f32)
    add("feet_first_touch", r)
    r = take(12); lift(r); r["info_go2"][:, G["AIR"]:G["AIR"] + 4] = rng.uniform(0.05, 0.5, (12, 4)).astype(f32)
    r["info_go2"][:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4] = 1
    add("feet_filter", r)
    r = take(12); r["info_go2"][:, G["AIR"]:G["AIR"] + 4] = 0; r["info_go2"][:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4] = 1
    r["info_go2"][:, G["CONTACT_T"]:G["CONTACT_T"] + 4] = rng.uniform(0.02, 0.6, (12, 4)).astype(f32)
    add("feet_ground", r)
    r = take(12); retract(r, (0, 3)); r["info_go2"][:, G["AIR"]:G["AIR"] + 4] = rng.uniform(0.0, 0.3, (12, 4)).astype(f32)
    add("nair_2", r)
    r = take(12); retract(r, (0, 1, 3)); add("nair_3", r)
    r = take(12); lift(r); r["info_go2"][:, G["SWING"]:G["SWING"] + 4] = rng.uniform(0.0, 0.5, (12, 4)).astype(f32)
    add("nair_4", r)
    # ---- soft joint limits: a joint 0.03 beyond, held there, robot in the air ----
    for kind, ji in (("hip", 0), ("thigh", 1), ("calf", 2)):
        for side in ("low", "high"):
            r = take(10); lift(r)
            for e in range(10):
                j = 3 * (e % 4) + ji
                r["qpos"][e, 7 + j] = soft[j] - f32(0.03) if side == "low" else soft[12 + j] + f32(0.03)
            hold(r, range(12))
            add(f"limit_{kind}_{side}", r)
    # ---- termination ----
    r = take(12); flip(r, np.pi + rng.uniform(-0.4, 0.4, 12)); add("upside_down", r)
    r = take(10); flip(r, np.where(np.arange(10) % 2 == 0, 1, -1) * (np.pi / 2 - rng.uniform(0.05, 0.3, 10))); add("side_up", r)
    r = take(10); flip(r, np.where(np.arange(10) % 2 == 0, 1, -1) * (np.pi / 2 + rng.uniform(0.05, 0.3, 10))); add("side_down", r)
    # ---- reward total: the command is what the robot does (positive; beyond the upper clamp at the large scale) ----
    r = take(12); r["info_go2"][:, 0:2] = r["priv_obs"][:, 57:59]; r["info_go2"][:, 2] = r["priv_obs"][:, 50]
    r["action"] = r["info_go2"][:, G["LAST_ACT"]:G["LAST_ACT"] + 12].copy()
    add("reward_tracked", r)
    # ---- kicks ----
    def kick(r, since, until, psteps, dur):
        n = len(r["qpos"])
        g = r["info_go2"]
        g[:, G["SINCE_PERT"]], g[:, G["STEPS_PERT"]], g[:, G["PERT_STEPS"]], g[:, G["PERT_DUR"]] = since, until, psteps, dur
        g[:, G["PERT_DUR_S"]] = (np.asarray(dur, f32) * f32(0.02) + rng.uniform(-0.009, 0.009, n).astype(f32)).astype(f32)
        g[:, G["PERT_MAG"]] = rng.uniform(1.0, 4.0, n).astype(f32)
        ang = rng.uniform(0, 2 * np.pi, n)
        g[:, G["PERT_DIR"]], g[:, G["PERT_DIR"] + 1], g[:, G["PERT_DIR"] + 2] = np.cos(ang).astype(f32), np.sin(ang).astype(f32), 0
    r = take(10); kick(r, rng.integers(0, 10, 10), 20, 0, 6); add("kick_waiting", r)
    r = take(10); kick(r, 19, 20, 3, 6); add("kick_start", r)
    r = take(10); kick(r, 20 + rng.integers(0, 3, 10), 20, rng.integers(0, 6, 10), 6); r["info_go2"][:5, G["PERT_STEPS"]] = np.arange(5)
    add("kick_mid", r)
    r = take(10); kick(r, 26, 20, np.where(np.arange(10) < 7, 6, 7), 6); add("kick_last", r)
    r = take(10); kick(r, 22, 20, rng.integers(1, 6, 10), 6); flip(r, np.pi + rng.uniform(-0.3, 0.3, 10)); add("kick_done", r)
    # ---- wrappers ----
    r = take(10); r["info_steps"][:] = CS.EPISODE_LENGTH - 1; add("last_step", r)
    r = take(10); r["info_steps"][:] = CS.EPISODE_LENGTH - 1; flip(r, np.pi + rng.uniform(-0.3, 0.3, 10)); add("last_step_done", r)
    r = take(10); r["info_episode_done"][:] = 1; add("prev_episode_done", r)
    r = take(10); r["done"][:] = 1; r["info_episode_done"][:] = 1; add("prev_done", r)

    fx = {k: np.concatenate([c[k] for c in chunks]).astype(f32) for k in CS.RECORD + ("action",)}
    fx["cls"] = np.concatenate([c["cls"] for c in chunks])
    n = len(fx["cls"])
    fx["keys"] = prng.split(prng.PRNGKey(SEED + 1), n)
    fx["class_names"] = np.array(names)
    # ---- PRNG keys with the timer draws clear of half-integers ----
    F = K0["F"]
    cand = prng.split(prng.PRNGKey(SEED + 2), 8 * n).reshape(n, 8, 2)
    chosen = np.zeros((n, 2), np.uint32)
    for e in range(n):
        for c in cand[e]:
            good = True
            for pre_split in (False, True):
                key = prng.split(c, 2)[0] if pre_split else c
                for _ in range(5):
                    key = prng.split(key, 2)[0]
                uu = np.float64(prng.uniform(prng.split(key, 3)[2], (), 0.0, 1.0))
                x = -np.log1p(-uu) * np.float64(F[16]) / np.float64(F[0])
                good &= abs((x % 1.0) - 0.5) > 10 * CS.HALF_MARGIN
            if good:
                chosen[e] = c
                break
        else:
            raise AssertionError("no key with a clear timer draw")
    fx["info_go2"][:, G["RNG"]:G["RNG"] + 2] = chosen.view(f32)
    return fx


def tolerances(fx):
    """{variant: {quantity: max |ref32 - ref64| over the fixture}}, both references fed the same f32-oracle record"""
    m = go2_model()
    worst = {}
    for name in CS.VARIANTS:
        K = CS.variant_constants(m, name)
        before, after = oracle_step(variant_oracle(m, name), fx)
        # the physics inputs come from an Episode-only twin where AutoReset would have restored them
        if K["autoreset"]:
            _, after = oracle_step(variant_oracle(m, name, auto_reset=False), fx)
        feet = CS.variant_fields(m, name)[1]["env_ids"][1:5]
        pre, phys = CS.before_of(before, fx["action"]), CS.phys_of(after, feet)
        r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
        q32, q64 = R.float_quantities(r32, K), R.float_quantities(r64, K)
        worst[name] = {nm: float("%.3e" % np.abs(q32[nm].astype(np.float64) - q64[nm]).max()) for nm in sorted(q64)}
    return worst


def main():
    fx = generate()
    np.savez_compressed(OUT, **fx)
    print("%d states, %d bytes; classes: %s" % (len(fx["cls"]), os.path.getsize(OUT), dict(zip(*np.unique(fx["cls"], return_counts=True)))))
    tol = tolerances(fx)
    json.dump(tol, open(TOL, "w"), indent=1)
    names = sorted(set().union(*tol.values()))
    print("| quantity | " + " | ".join(tol) + " |")
    for k in names:
        print("| %s | " % k + " | ".join("%.1e" % tol[v][k] if k in tol[v] else "-" for v in tol) + " |")


if __name__ == "__main__":
    main()
