"""Plain numpy restatement of what the Airbot step does around the physics (csrc/rsr_airbot.hpp step_kernel<C, ENV>, oracle/rsr_oracle.c
step_env / tshape_step_env; cube_env.py:145-229, test/airbot.py:165-252, T_shape_env.py:139-234, plus the brax Episode / AutoReset
wrappers) for the three kinds "cube", "sf" and "tshape".

The physics is an INPUT: the reference is fed what a step publishes after it ran (qpos, xpos, site_xpos -- store_pipeline writes the
last forward pass's values, the very ones the epilogue used) together with the record from before the step, and recomputes
everything else the step writes.  It is parameterised by dtype: float64 is the reference, float32 the same algebra at the kernel's
precision, op by op in the kernel's order (the kernel sets `fp contract(off)` for the env algebra, so away from libm the float32
restatement has to give the kernel's bits).  Config constants and the kernel's literals (0.042f, 1.5708f, ...) are float32 values in
either mode.

Gates.  `q < threshold` on a computed quantity (btd, s2c, the sf hold's 3 cm distance, dis_base, dis_vert) is a decision: it is taken
on the float32 value in either mode -- every such quantity is +, * and sqrt of published float32 words, which are IEEE on the device
and here, so the float32 value IS the kernel's -- and `bands` says which states sit within BAND_ULPS ulp32 of a threshold, where a
test leaves the verdict to the step.  Comparisons of published words (site z < 0.82f, ...) see the same float32 on both sides.

T-shape geoms.  s.egeom (base_block, vertical_block world positions) is not published.  dis_base / dis_vert are computed from the
published obs[7:13], the very float32 differences tb - gb and tv - gv the kernel squares; for ba = gv - gb the geoms are
reconstructed in float64 as gb = tb - obs[7:10], gv = tv - obs[10:13], which is off by up to one ulp32 of tb / tv per component:
`xita_allowance` propagates that through the angle.  What follows xita (push_w, obs[13], info_xita's copy) is computed from the xita
the step itself published (phys["xita"]), so that it can be held bitwise."""
import numpy as np

f32 = np.float32
ID_CUBE, ID_TARGET, ID_SITE, ID_BOXQ, ID_SITEQ, ID_FINGERQ, ID_JOINTQ = range(7)
TID_T, TID_TARGET, TID_SITE, TID_TAIL, TID_TTAIL, TID_GBASE, TID_GVERT, TID_GTBASE, TID_GTVERT, TID_JOINTQ = range(10)
KINDS = ("cube", "sf", "tshape")
BAND_ULPS = 8               # a sum of three squares and a sqrt carry <= 2 ulp32; 8 leaves room for a differently ordered sum
NEW_POS = {"cube": "info_new_cube_pos", "sf": "info_new_cube_pos", "tshape": "info_new_T_pos"}
BODY_POS = {"cube": "info_cube_pos", "sf": "info_cube_pos", "tshape": "info_T_pos"}
METRIC_NAMES = {"cube": ("push_reward", "ctrl_cost", "siet_to_box_reward"), "sf": ("push_reward", "ctrl_cost", "siet_to_box_reward"),
                "tshape": ("push_reward", "siet2cube_reward", "health_reward", "task_complete_reward", "site_z_reward")}
KEPT = {"cube": 1, "sf": 1, "tshape": 3}            # the metric word the step never writes


def constants(kind, fields):
    """The env constants of a blob's fields (config.cube_env_fields / sf_env_fields / tshape_env_fields) as the reference reads them."""
    ei = np.asarray(fields["env_int"]).astype(int)
    return dict(kind=kind, ids=np.asarray(fields["env_ids"]).astype(int), scale=np.asarray(fields["env_action_scale"], f32),
                lo=np.asarray(fields["env_ctrl_lo"], f32), hi=np.asarray(fields["env_ctrl_hi"], f32),
                W=np.asarray(fields["env_reward"], f32), n_frames=int(ei[1]), L=int(ei[2]), episode=bool(ei[3] & 1),
                autoreset=bool(ei[3] & 2), nmet=int(ei[5]))


def _clamp(x, lo, hi):
    """clampf of the kernel: x < lo ? lo : (x > hi ? hi : x) (a NaN passes through)"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _norm3(a, b, c):
    return np.sqrt((a * a + b * b) + c * c)


def step(K, pre, phys, dtype=np.float64, verdicts=None):
    """pre: the record before the step (ctrl, qpos, xpos, site_xpos, info_*, done, metrics, ...) and `action`; phys: qpos, xpos,
    site_xpos after the step, for the T-shape also obs (elements 7:13 are read) and xita.  Returns every word the step writes."""
    T = dtype
    if verdicts is None and T is not np.float32:
        verdicts = step(K, pre, phys, np.float32)["verdicts"]
    c = lambda x: T(f32(x))
    A = lambda x: np.asarray(x, f32).astype(T)
    kind, ids, W = K["kind"], K["ids"], K["W"].astype(T)
    ts, sf = kind == "tshape", kind == "sf"
    n = len(pre["ctrl"])
    col = lambda k: A(pre[k]).reshape(n, -1)[:, 0]
    out, quant, verd = {}, {}, {}

    def gate(name, q, thr):
        quant[name] = (np.asarray(q, np.float64), float(f32(thr)))
        verd[name] = (q < T(f32(thr))) if verdicts is None else verdicts[name]
        return verd[name]

    # ---- prologue: ctrl shaping from the record before the step (stale xpos / site_xpos) ----
    jq = ids[(TID_JOINTQ if ts else ID_JOINTQ):][:6]
    ctrl0, qpos0, action = A(pre["ctrl"]), A(pre["qpos"]), A(pre["action"])
    xpos0, sx0 = A(pre["xpos"]).reshape(n, -1, 3), A(pre["site_xpos"]).reshape(n, -1, 3)
    act = ctrl0 + K["scale"].astype(T) * action
    act0 = act[:, 0].copy()
    act[:, 3] = -((c(1.57) + qpos0[:, jq[1]]) + qpos0[:, jq[2]])
    if ts:
        dx = sx0[:, ids[TID_TAIL], 0] - sx0[:, ids[TID_SITE], 0]
        dy = sx0[:, ids[TID_TAIL], 1] - sx0[:, ids[TID_SITE], 1]
    else:
        tp = A(pre["info_target_pos"])
        dx, dy = tp[:, 0] - xpos0[:, ids[ID_CUBE], 0], tp[:, 1] - xpos0[:, ids[ID_CUBE], 1]
    ang = np.arctan2(dy, dx + c(0.00001))
    a4 = (-ang + act0) + c(1.5708)
    out["aim_scale"] = np.maximum(np.maximum(np.abs(ang), np.abs(act0)), np.abs(-ang + act0)).astype(np.float64) + 1.5708
    if sf:
        dz = tp[:, 2] - xpos0[:, ids[ID_CUBE], 2]
        hold = gate("hold", _norm3(dx, dy, dz), 0.03)
        a4 = np.where(hold, col("info_last_action"), a4)
        out["info_last_action"] = a4.copy()                    # written before the clamp
    act[:, 4] = a4
    out["ctrl"] = _clamp(act, K["lo"].astype(T), K["hi"].astype(T))

    # ---- epilogue: reward, done, obs, info from the last forward pass ----
    qpos, xpos, sx = A(phys["qpos"]), A(phys["xpos"]).reshape(n, -1, 3), A(phys["site_xpos"]).reshape(n, -1, 3)
    aux_old = A(pre[NEW_POS[kind]])
    met_kept = A(pre["metrics"])[:, KEPT[kind]]
    one, zero = T(1), T(0)
    obs = np.zeros((n, 16 if ts else 23), T)
    obs[:, :6] = qpos[:, jq]
    if ts:
        sp, tbody = sx[:, ids[TID_SITE]], xpos[:, ids[TID_T]]
        tb, tv = A(pre["info_target_base_pos"]), A(pre["info_target_vertical_pos"])
        og = A(phys["obs"])[:, 7:13]                           # tb - gb, tv - gv as the step computed them
        snap_b = gate("dis_base", _norm3(og[:, 0], og[:, 1], og[:, 2]), 0.005)
        dis_base = np.where(snap_b, zero, _norm3(og[:, 0], og[:, 1], og[:, 2]))
        push_base = one / (one + c(10) * dis_base)
        snap_v = gate("dis_vert", _norm3(og[:, 3], og[:, 4], og[:, 5]), 0.005)
        dis_vert = np.where(snap_v, zero, _norm3(og[:, 3], og[:, 4], og[:, 5]))
        push_vert = one / (one + c(10) * dis_vert)
        tb64, tv64 = np.asarray(pre["info_target_base_pos"], np.float64), np.asarray(pre["info_target_vertical_pos"], np.float64)
        og64 = np.asarray(phys["obs"], np.float64)[:, 7:13]
        gb64, gv64 = tb64 - og64[:, 0:3], tv64 - og64[:, 3:6]
        ba, ta = (gv64 - gb64).astype(T), tv - tb
        dotp = (ba[:, 0] * ta[:, 0] + ba[:, 1] * ta[:, 1]) + ba[:, 2] * ta[:, 2]
        nb, nt = _norm3(ba[:, 0], ba[:, 1], ba[:, 2]), _norm3(ta[:, 0], ta[:, 1], ta[:, 2])
        cosv = _clamp(dotp / (nb * nt), -one, one)
        out["xita_own"] = np.arccos(cosv)
        out["cosine"] = np.asarray(dotp / (nb * nt), np.float64)
        out["xita_allowance"] = _xita_allowance(gb64, gv64, tb64, tv64)
        xita = A(phys["xita"]).reshape(n)                      # what the step published: everything below follows from it
        push_w = one / (one + c(6) * xita)
        push = ((c(0.1515) * push_base + c(0.1515) * push_vert) + c(0.66) * push_w) * W[0]
        site_z = np.where(sp[:, 2] < c(0.83), one, zero)
        z_reward = c(4) / (one + c(3) * np.abs(sp[:, 2] - c(0.805)))
        site_z = site_z + z_reward
        tail, ttail = sx[:, ids[TID_TAIL]], sx[:, ids[TID_TTAIL]]
        dx, dy = ttail[:, 0] - tail[:, 0], ttail[:, 1] - tail[:, 1]
        ang = np.arctan2(dy, dx + c(0.00001))
        dist = np.sqrt(dx * dx + dy * dy) + c(0.025)
        y_, x_ = dist * np.sin(ang), dist * np.cos(ang)
        new_pos = np.stack([(dx - x_) + tail[:, 0], (dy - y_) + tail[:, 1]], 1)
        e0, e1 = sp[:, 0] - aux_old[:, 0], sp[:, 1] - aux_old[:, 1]
        s2c_raw = np.sqrt(e0 * e0 + e1 * e1)
        dead = gate("s2c", s2c_raw, 0.02)
        s2c = np.where(dead, zero, s2c_raw - c(0.02))
        siet = (one - np.tanh(c(5) * s2c)) * W[1]
        health = W[2] * np.abs(np.where(sp[:, 2] < W[3], one, zero) - one)
        terms = [push, siet, health, site_z]
        done = np.where(tbody[:, 2] < c(0.6), one, zero)
        obs[:, 6] = sp[:, 2]
        obs[:, 7:13] = og
        obs[:, 13] = xita
        obs[:, 14], obs[:, 15] = new_pos[:, 0] - sp[:, 0], new_pos[:, 1] - sp[:, 1]
        metrics = np.stack([push, siet, health, met_kept, site_z], 1)
        out.update(info_xita=xita, info_T_pos=tbody.copy())
    else:
        cp, sp = xpos[:, ids[ID_CUBE]], sx[:, ids[ID_SITE]]
        d0, d1, d2 = tp[:, 0] - cp[:, 0], tp[:, 1] - cp[:, 1], tp[:, 2] - cp[:, 2]
        btd_raw = _norm3(d0, d1, d2)
        snap = gate("btd_w4", btd_raw, K["W"][4])              # 0.005 (cube) / 0.003 (sf)
        btd = np.where(snap, zero, btd_raw)
        push = (one / (one + c(3) * btd)) * W[0]
        task_complete = np.where(snap, W[5], zero)             # btd < W[4] after the snap: 0 or >= W[4]
        site_z = np.where(sp[:, 2] < c(0.82), one, zero)
        ang = np.arctan2(d1, d0 + c(0.00001))
        dist = np.sqrt(d0 * d0 + d1 * d1) + c(0.04)
        y_, x_ = dist * np.sin(ang), dist * np.cos(ang)
        new_pos = np.stack([(d0 - x_) + cp[:, 0], (d1 - y_) + cp[:, 1]], 1)
        e0, e1 = sp[:, 0] - aux_old[:, 0], sp[:, 1] - aux_old[:, 1]
        s2c_raw = np.sqrt(e0 * e0 + e1 * e1)
        dead = gate("s2c", s2c_raw, 0.042)
        s2c = np.where(dead, zero, s2c_raw - c(0.042))
        siet = (one - np.tanh(c(5) * s2c)) * W[1]
        near = snap | gate("btd_005", btd_raw, 0.005)          # sf: the band [0.003, 0.005) overrides siet without the snap
        siet = np.where(near, W[1], siet)
        hd = np.where(sp[:, 2] < W[3], one, zero)
        if sf:
            oob = (sp[:, 0] > one) | (sp[:, 0] < c(-0.6)) | (sp[:, 1] > c(0.3)) | (sp[:, 1] < c(-0.3)) | (cp[:, 2] < c(0.6))
            hd = np.where(oob, one, hd)
        health = W[2] * np.abs(hd - one)
        terms = [push, siet, health, task_complete, site_z] if sf else [push, siet, health, site_z]
        done = np.where(snap, one, zero) if sf else np.where(cp[:, 2] < c(0.6), one, zero)
        for i in range(3):
            obs[:, 6 + i], obs[:, 9 + i], obs[:, 12 + i] = sp[:, i], tp[:, i], cp[:, i]
            obs[:, 17 + i], obs[:, 20 + i] = tp[:, i] - cp[:, i], cp[:, i] - sp[:, i]
        obs[:, 15:17] = new_pos
        metrics = np.stack([push, met_kept, siet], 1)
        out.update(info_cube_pos=cp.copy(), unpublished_terms=[health, task_complete, site_z] if sf else [health, site_z])
    xe, ye = (dx + c(0.00001), dy) if ts else (d0 + c(0.00001), d1)
    out["new_pos_quadrant"] = np.select([(xe > 0) & (ye > 0), (xe < 0) & (ye > 0), (xe < 0) & (ye < 0), (xe > 0) & (ye < 0)], [0, 1, 2, 3], -1)
    total = terms[0]
    for t in terms[1:]:
        total = total + t
    reward = _clamp(total, c(-100), c(100))
    out["reward_scale"] = np.max(np.abs(np.stack(terms + [total], 1)).astype(np.float64), 1)
    out["pos_scale"] = np.maximum(np.abs(dist), np.abs(new_pos).max(1)).astype(np.float64)

    # ---- Episode / AutoReset wrappers ----
    steps, done_prev = col("info_steps"), np.asarray(pre["done"], f32).reshape(n)
    if K["autoreset"]:
        steps = np.where(done_prev != 0, zero, steps)
    done_env = done.copy()
    trunc, epi_done, em = col("info_truncation"), col("info_episode_done"), A(pre["info_episode_metrics"])
    if K["episode"]:
        steps = steps + one
        over = steps >= T(K["L"])
        trunc = np.where(over, one - done_env, zero)
        add = np.concatenate([reward[:, None], np.ones((n, 1), T), metrics], 1)
        prev = np.asarray(pre["info_episode_done"], f32).reshape(n) != 0
        with np.errstate(invalid="ignore"):
            em = np.where(prev[:, None], zero, em + add)       # a select: a NaN sum with prev_done = 1 becomes 0, with 0 it stays
        done = np.where(over, one, done)
        epi_done = done
    restored = (done != 0) & K["autoreset"]
    out.update(obs=obs, metrics=metrics, reward=reward, raw_total=total, done_env=done_env, done=done, info_steps=steps,
               info_truncation=trunc, info_episode_done=epi_done, info_episode_metrics=em, info_site_pos=sp.copy(), new_pos=new_pos,
               restored=restored, verdicts=verd, quant=quant)
    return out


def _xita_allowance(gb, gv, tb, tv):
    """What one ulp32 of tb and tv per component (the defect of gb = tb - fl(tb - gb), and of gv) can move the angle by: the sum over
    the six components of |xita(perturbed) - xita|, float64, unclamped-safe."""
    def angle(gb_, gv_):
        ba, ta = gv_ - gb_, tv - tb
        cs = (ba * ta).sum(1) / np.sqrt((ba * ba).sum(1) * (ta * ta).sum(1))
        return np.arccos(np.clip(cs, -1.0, 1.0))
    base = angle(gb, gv)
    tot = np.zeros(len(gb))
    for i in range(3):
        for which, ref in ((0, tb), (1, tv)):
            d = np.zeros_like(gb)
            d[:, i] = np.spacing(np.abs(ref[:, i]).astype(f32)).astype(np.float64)
            both = [np.abs(angle(gb + s * d, gv) - base) if which == 0 else np.abs(angle(gb, gv + s * d) - base) for s in (-1.0, 1.0)]
            tot += np.maximum(both[0], both[1])
    return tot


def bands(K, r):
    """{gate: states whose float32 threshold quantity lies within BAND_ULPS ulp32 of its threshold} of a float32 result"""
    return {g: np.abs(q - thr) <= BAND_ULPS * float(np.spacing(f32(thr))) for g, (q, thr) in r["quant"].items()}


def from_record(K, rec):
    """a record a step left (oracle state or device views, numpy) in the terms of step()'s result"""
    kind = K["kind"]
    n = len(rec["ctrl"])
    a = lambda k: np.asarray(rec[k], f32).reshape(n, -1).astype(np.float64)
    o = dict(ctrl=a("ctrl"), obs=a("obs"), metrics=a("metrics"), reward=a("reward")[:, 0], done=a("done")[:, 0],
             info_steps=a("info_steps")[:, 0], info_truncation=a("info_truncation")[:, 0], info_episode_done=a("info_episode_done")[:, 0],
             info_episode_metrics=a("info_episode_metrics"), info_site_pos=a("info_site_pos"), new_pos=a(NEW_POS[kind]))
    o[BODY_POS[kind]] = a(BODY_POS[kind])
    if kind == "tshape":
        o["info_xita"] = a("info_xita")[:, 0]
        o["xita_own"] = o["info_xita"]
    if kind == "sf":
        o["info_last_action"] = a("info_last_action")[:, 0]
    return o


def float_quantities(o, K):
    """name -> array of every float-valued quantity a step computes (compared within a tolerance)"""
    kind = K["kind"]
    q = {"ctrl/shaped": o["ctrl"][:, :4], "ctrl/aim": o["ctrl"][:, 4], "reward": o["reward"], "new_pos": o["new_pos"]}
    for i, nm in enumerate(METRIC_NAMES[kind]):
        if i != KEPT[kind]:
            q["metrics/" + nm] = o["metrics"][:, i]
    if kind == "tshape":
        q.update({"xita": o["xita_own"], "obs/new_T_minus_site": o["obs"][:, 14:16]})
    else:
        q.update({"obs/new_cube_pos": o["obs"][:, 15:17], "obs/target_minus_cube": o["obs"][:, 17:20], "obs/cube_minus_site": o["obs"][:, 20:23]})
    if kind == "sf":
        q["info_last_action"] = o["info_last_action"]
    if K["episode"]:
        q.update({"episode/sum_reward": o["info_episode_metrics"][:, 0], "episode/metrics": o["info_episode_metrics"][:, 2:]})
    return q


def exact_quantities(o, K):
    """name -> array of everything that is integer-valued, a copy or a pass-through word (compared for equality)"""
    kind = K["kind"]
    q = {"done": o["done"], "info_steps": o["info_steps"], "info_truncation": o["info_truncation"], "info_episode_done": o["info_episode_done"],
         "episode/length": o["info_episode_metrics"][:, 1], "info_site_pos": o["info_site_pos"], BODY_POS[kind]: o[BODY_POS[kind]],
         "metrics/kept": o["metrics"][:, KEPT[kind]], "obs/joints": o["obs"][:, :6]}
    if kind == "tshape":
        q.update({"obs/site_z": o["obs"][:, 6], "obs/xita": o["obs"][:, 13], "info_xita": o["info_xita"]})
    else:
        q.update({"obs/site_target_cube": o["obs"][:, 6:15]})
    return q


def needs_phys(name):
    """whether a quantity of the two tables above is read from words AutoReset restores (obs, ctrl): those can be compared only for
    envs that still publish them.  Everything else a step writes (reward, metrics, info, wrapper words) survives AutoReset."""
    return name.split("/")[0] in ("obs", "ctrl")


def scale_of(name, r):
    """the magnitude a quantity's roundings happen at, where that is larger than the quantity itself (float64 result r)"""
    if name in ("ctrl/aim", "info_last_action"):
        return r["aim_scale"]
    if name in ("new_pos", "obs/new_cube_pos", "obs/new_T_minus_site"):
        return r["pos_scale"][:, None]
    if name in ("reward", "episode/sum_reward"):
        return r["reward_scale"]
    return None


def reward_from_metrics(K, metrics, extra):
    """The reward a step must publish given the metrics it published: their float32 sum in the kernel's order, clamped.  `extra`
    holds the terms that are no metric (float32, computed from published words without libm): cube / sf: health, [task_complete],
    site_z; T-shape: none."""
    m = np.asarray(metrics, f32)
    if K["kind"] == "tshape":
        total = ((m[:, 0] + m[:, 1]) + m[:, 2]) + m[:, 4]
    else:
        total = m[:, 0] + m[:, 2]
        for t in extra:
            total = total + np.asarray(t, f32)
    return _clamp(total, f32(-100), f32(100))


def episode_sums_from_outputs(K, pre, reward, metrics):
    """The Episode wrapper's sums given the reward and metrics the step published (float32, bit for bit)."""
    n = len(metrics)
    add = np.concatenate([np.asarray(reward, f32).reshape(-1, 1), np.ones((n, 1), f32), np.asarray(metrics, f32)], 1)
    prev = np.asarray(pre["info_episode_done"], f32).reshape(-1) != 0
    with np.errstate(invalid="ignore"):
        return np.where(prev[:, None], f32(0), np.asarray(pre["info_episode_metrics"], f32).reshape(n, -1) + add)
