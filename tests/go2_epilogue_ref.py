"""Plain numpy restatement of what the Go2 joystick step does around the physics (csrc/rsr_go2.hpp go2_step_kernel, oracle/rsr_oracle.c
go2_step_env; go2/joystick.py:204-280, rewards :367-593, kicks :594-644, sample_command :645-653, plus the Episode / AutoReset wrappers).

The physics is an INPUT: the reference is fed what a step publishes after it ran (privileged_obs[48:123], site_xpos, qpos, qvel, the
new LAST_CONTACT word) together with the record from before the step, and recomputes everything else the step writes.  It is
parameterised by dtype: float64 is the reference, float32 the same algebra at the kernel's precision (to measure rounding).  Draws
are jax.random's (rsr_mjx_amd.prng) and are float32 values in either mode, as are the config constants and the literals of the
kernel (0.1f, pi as float, ...).  Summation orders are the kernel's: 12-term sums in index order, the total in ORDER.

Two values the step does not publish follow from the gravity sensor (gravity = -(third row of R)):
    up[0]^2 + up[1]^2 = 1 - gravity[2]^2,  up[2] = -gravity[2],  glin[2] = -gravity . linvel_local.
"""
import numpy as np

from rsr_mjx_amd import prng

f32 = np.float32
G = dict(CMD=0, STEPS_CMD=3, LAST_ACT=4, LAST_LAST_ACT=16, AIR=28, CONTACT_T=32, LAST_CONTACT=36, SWING=40, ACT_BUF=44,
         GYRO_BUF=92, LINVEL_BUF=104, GRAV_BUF=116, STEPS_PERT=128, PERT_DUR_S=129, PERT_DUR=130, SINCE_PERT=131, PERT_STEPS=132,
         PERT_DIR=133, PERT_MAG=136, RNG=137, XFRC=139)
NINFO, NU, NMET, NPRIV = 144, 12, 22, 123
(RW_TRACK_LIN, RW_TRACK_ANG, RW_LIN_VEL_Z, RW_ANG_VEL_XY, RW_ORIENT, RW_DOF_LIMITS, RW_POSE, RW_TERM, RW_STAND_STILL, RW_TORQUES,
 RW_ACTION_RATE, RW_ENERGY, RW_FEET_CLEAR, RW_FEET_HEIGHT, RW_FEET_SLIP, RW_FEET_AIR, RW_ALL_FEET_AIR, RW_SYM_GAIT, RW_LR_SYM, RW_FB_SYM,
 RW_FEET_OFF_STILL) = range(21)
# sum(rewards.values()) in the insertion order of _get_reward's dict (joystick.py:378-423)
ORDER = (RW_TRACK_LIN, RW_TRACK_ANG, RW_LIN_VEL_Z, RW_ANG_VEL_XY, RW_ORIENT, RW_STAND_STILL, RW_TERM, RW_POSE, RW_TORQUES, RW_ACTION_RATE,
         RW_ENERGY, RW_FEET_SLIP, RW_FEET_CLEAR, RW_FEET_HEIGHT, RW_FEET_AIR, RW_DOF_LIMITS, RW_ALL_FEET_AIR, RW_SYM_GAIT, RW_LR_SYM,
         RW_FB_SYM, RW_FEET_OFF_STILL)
# privileged_state layout after the 48 of `state`
P = dict(gyro=(48, 51), accel=(51, 54), gravity=(54, 57), linvel=(57, 60), gang=(60, 63), jpos=(63, 75), jvel=(75, 87), aforce=(87, 99),
         last_contact=(99, 103), feet_vel=(103, 115), air=(115, 119), xfrc=(119, 122), kick=(122, 123))


def constants(fields, episode_length=0, auto_reset=False):
    """The env constants of a blob's fields (config.go2_env_fields) as the reference reads them."""
    return dict(F=np.asarray(fields["env_go2f"], f32), I=np.asarray(fields["env_go2i"]).astype(int), SC=np.asarray(fields["env_go2_scales"], f32),
                home=np.asarray(fields["env_go2_home"], f32), soft=np.asarray(fields["env_go2_soft"], f32),
                L=int(episode_length), episode=episode_length > 0, autoreset=bool(auto_reset))


def key_of(info):
    return np.ascontiguousarray(np.asarray(info, f32)[:, G["RNG"]:G["RNG"] + 2]).view(np.uint32)


def _split(key, n):
    return prng.split(key, n)            # [N, n, 2]


def _seq(x):
    """sum over the last axis in index order"""
    acc = x[..., 0] * 0
    for i in range(x.shape[-1]):
        acc = acc + x[..., i]
    return acc


def kick_update(K, info, key, T):
    """joystick.py:594-644: waiting (one split, direction drawn on the step the wait ends) or pulse (half sine; last step ends it)."""
    F = K["F"].astype(T)
    info = info.copy()
    if not K["I"][2]:
        return info, key
    dt = F[0]
    kicking = info[:, G["SINCE_PERT"]] >= info[:, G["STEPS_PERT"]]
    # pulse
    t = info[:, G["PERT_STEPS"]] * dt
    ph = T(f32(3.14159265358979323846)) * t
    u_t = T(0.5) * np.sin(ph / info[:, G["PERT_DUR_S"]])
    force = ((u_t * F[23]) * info[:, G["PERT_MAG"]]) / info[:, G["PERT_DUR_S"]]
    xf_pulse = force[:, None] * info[:, G["PERT_DIR"]:G["PERT_DIR"] + 3]
    since_pulse = np.where(info[:, G["PERT_STEPS"]] >= info[:, G["PERT_DUR"]], T(0), info[:, G["SINCE_PERT"]])
    # wait
    ks = _split(key, 2)
    angle = prng.uniform(ks[:, 1], (), 0.0, f32(6.2831855)).astype(T)
    since_wait = info[:, G["SINCE_PERT"]] + T(1)
    starts = ~kicking & (since_wait >= info[:, G["STEPS_PERT"]])
    out = info.copy()
    out[:, G["XFRC"]:G["XFRC"] + 3] = np.where(kicking[:, None], xf_pulse, T(0))
    out[:, G["SINCE_PERT"]] = np.where(kicking, since_pulse, since_wait)
    out[:, G["PERT_STEPS"]] = np.where(kicking, info[:, G["PERT_STEPS"]] + T(1), np.where(starts, T(0), info[:, G["PERT_STEPS"]]))
    d = np.stack([np.cos(angle), np.sin(angle), angle * 0], 1)
    out[:, G["PERT_DIR"]:G["PERT_DIR"] + 3] = np.where(starts[:, None], d, info[:, G["PERT_DIR"]:G["PERT_DIR"] + 3])
    key = np.where(kicking[:, None], key, ks[:, 0])
    return out, key


def action_fifo(K, info, action, T):
    """joystick.py:207-216: the applied action is the FIFO's head; ctrl = home + applied * action_scale."""
    adel = int(K["I"][0])
    info = info.copy()
    a0 = G["ACT_BUF"]
    if adel > 0:
        actual = info[:, a0:a0 + NU].copy()
        info[:, a0:a0 + adel * NU] = info[:, a0 + NU:a0 + NU + adel * NU].copy()
        info[:, a0 + adel * NU:a0 + (adel + 1) * NU] = action
    else:
        actual = action
    ctrl = K["home"].astype(T)[7:] + actual * K["F"].astype(T)[1]
    return info, ctrl


def imu_fifo(K, info, gyro, linvel, gravity):
    """joystick.py:220-235"""
    idel = int(K["I"][1])
    info = info.copy()
    if idel > 0:
        for b, cur in ((G["GYRO_BUF"], gyro), (G["LINVEL_BUF"], linvel), (G["GRAV_BUF"], gravity)):
            info[:, b:b + 3 * idel] = info[:, b + 3:b + 3 + 3 * idel].copy()
            info[:, b + 3 * idel:b + 3 * idel + 3] = cur
    return info


def noisy_obs(K, info, key, gyro, linvel, gravity, qpos, qvel, T):
    """joystick.py:284-340: five serial (split, uniform) draws in the order gyro, gravity, linvel, joint angles, joint velocities."""
    F = K["F"].astype(T)
    idel = int(K["I"][1]) > 0
    src = [info[:, G["GYRO_BUF"]:G["GYRO_BUF"] + 3] if idel else gyro, info[:, G["GRAV_BUF"]:G["GRAV_BUF"] + 3] if idel else gravity,
           info[:, G["LINVEL_BUF"]:G["LINVEL_BUF"] + 3] if idel else linvel, qpos[:, 7:], qvel[:, 6:]]
    scale, dst = (F[5], F[6], F[7], F[3], F[4]), (3, 6, 0, 9, 21)
    obs = np.zeros((info.shape[0], 48), T)
    for d in range(5):
        ks = _split(key, 2)
        key = ks[:, 0]
        n = src[d].shape[1]
        u = prng.uniform(ks[:, 1], (n,), 0.0, 1.0).astype(T)
        val = src[d] + (((T(2) * u) - T(1)) * F[2]) * scale[d]
        if d == 3:
            val = val - K["home"].astype(T)[7:]
        obs[:, dst[d]:dst[d] + n] = val
    obs[:, 33:45] = info[:, G["LAST_ACT"]:G["LAST_ACT"] + NU]
    obs[:, 45:48] = info[:, G["CMD"]:G["CMD"] + 3]
    return obs, key


def reward_terms(K, info, action, contact, first_contact, feet_z, gyro, linvel, gravity, gang, qpos, qvel, aforce, feet_vel, T):
    """The 21 unscaled terms (info: command, last_act, AIR after its first +dt, SWING after the max, CONTACT_T)."""
    F, home, soft = K["F"].astype(T), K["home"].astype(T), K["soft"].astype(T)
    cmd = info[:, G["CMD"]:G["CMD"] + 3]
    # the two gates are decisions, taken on the float32 norm in either mode like the draws: a command whose float32 norm is 0.01f
    # exactly opens neither, which no other precision reproduces (every other state of the fixture keeps 1e-4 from the threshold)
    c32 = cmd.astype(f32)
    cmd_norm = np.sqrt(c32[:, 0] * c32[:, 0] + c32[:, 1] * c32[:, 1] + c32[:, 2] * c32[:, 2])
    thr = f32(0.01)
    moving, still = (cmd_norm > thr).astype(T), (cmd_norm < thr).astype(T)
    rw = np.zeros((info.shape[0], 21), T)
    e0, e1 = cmd[:, 0] - linvel[:, 0], cmd[:, 1] - linvel[:, 1]
    rw[:, RW_TRACK_LIN] = np.exp(-(e0 * e0 + e1 * e1) / F[8])
    ea = cmd[:, 2] - gyro[:, 2]
    rw[:, RW_TRACK_ANG] = np.exp(-(ea * ea) / F[8])
    glin2 = -((gravity[:, 0] * linvel[:, 0] + gravity[:, 1] * linvel[:, 1]) + gravity[:, 2] * linvel[:, 2])
    rw[:, RW_LIN_VEL_Z] = glin2 * glin2
    rw[:, RW_ANG_VEL_XY] = gang[:, 0] * gang[:, 0] + gang[:, 1] * gang[:, 1]
    rw[:, RW_ORIENT] = T(1) - gravity[:, 2] * gravity[:, 2]
    done_env = (gravity[:, 2] > 0).astype(T)                      # up[2] = -gravity[2] < 0
    q = qpos[:, 7:]
    dq = q - home[7:]
    lo_, hi_ = q - soft[:12], q - soft[12:]
    w = np.where(np.arange(12) % 3 == 2, T(f32(0.1)), T(1))
    t = aforce
    dd = action - info[:, G["LAST_ACT"]:G["LAST_ACT"] + NU]
    rw[:, RW_STAND_STILL] = _seq(np.abs(dq)) * still
    rw[:, RW_DOF_LIMITS] = _seq(-np.where(lo_ < 0, lo_, T(0)) + np.where(hi_ > 0, hi_, T(0)))
    rw[:, RW_POSE] = np.exp(-_seq(dq * dq * w))
    rw[:, RW_TERM] = done_env
    rw[:, RW_TORQUES] = np.sqrt(_seq(t * t)) + _seq(np.abs(t))
    rw[:, RW_ENERGY] = _seq(np.abs(qvel[:, 6:]) * np.abs(t))
    rw[:, RW_ACTION_RATE] = _seq(dd * dd)
    c, fc = contact.astype(T), first_contact.astype(T)
    fv = feet_vel.reshape(-1, 4, 3)
    v2 = fv[:, :, 0] * fv[:, :, 0] + fv[:, :, 1] * fv[:, :, 1]
    air, swing, ct = info[:, G["AIR"]:G["AIR"] + 4], info[:, G["SWING"]:G["SWING"] + 4], info[:, G["CONTACT_T"]:G["CONTACT_T"] + 4]
    err = swing / F[9] - T(1)
    nair = _seq(T(1) - c)
    rw[:, RW_FEET_SLIP] = _seq(v2 * c) * moving
    rw[:, RW_FEET_CLEAR] = _seq(np.abs(feet_z - F[9]) * np.sqrt(np.sqrt(v2)))
    rw[:, RW_FEET_HEIGHT] = _seq(err * err * fc) * moving
    rw[:, RW_FEET_AIR] = _seq((air - T(f32(0.1))) * fc) * moving
    rw[:, RW_ALL_FEET_AIR] = (nair >= 3).astype(T) * moving
    rw[:, RW_FEET_OFF_STILL] = nair * still
    x, y = q[:, 3:6] - q[:, 6:9], q[:, 0:3] - q[:, 9:12]
    rw[:, RW_SYM_GAIT] = (_seq(x * x) + _seq(y * y)) * moving
    two = T(2)
    la, lc, ra, rc = (air[:, 1] + air[:, 3]) / two, (ct[:, 1] + ct[:, 3]) / two, (air[:, 0] + air[:, 2]) / two, (ct[:, 0] + ct[:, 2]) / two
    rw[:, RW_LR_SYM] = ((la - ra) * (la - ra) + (lc - rc) * (lc - rc)) * moving
    fa, fc_, ba, bc = (air[:, 0] + air[:, 1]) / two, (ct[:, 0] + ct[:, 1]) / two, (air[:, 2] + air[:, 3]) / two, (ct[:, 2] + ct[:, 3]) / two
    rw[:, RW_FB_SYM] = ((fa - ba) * (fa - ba) + (fc_ - bc) * (fc_ - bc)) * moving
    return rw, done_env, cmd_norm


def resample(K, info, key, done_env, T):
    """joystick.py:255-277 and sample_command: split(rng, 3); the command mixes in a fresh draw when the timer runs out; the
    timer is redrawn (exponential) then or on termination."""
    F = K["F"].astype(T)
    info = info.copy()
    steps_cmd = info[:, G["STEPS_CMD"]] - T(1)
    k3 = _split(key, 3)
    k4 = _split(k3[:, 1], 4)                                   # rng, y_rng, w_rng, z_rng
    amp = K["F"][10:13]
    y = prng.uniform(k4[:, 1], (3,), -amp, amp).astype(T)
    z = (prng.uniform(k4[:, 3], (3,), 0.0, 1.0) < K["F"][13:16]).astype(T)
    w = (prng.uniform(k4[:, 2], (3,), 0.0, 1.0) < f32(0.5)).astype(T)
    x = info[:, G["CMD"]:G["CMD"] + 3]
    run_out = steps_cmd <= 0
    info[:, G["CMD"]:G["CMD"] + 3] = np.where(run_out[:, None], x - w * (x - y * z), x)
    uu = prng.uniform(k3[:, 2], (), 0.0, 1.0).astype(T)
    t1 = -np.log1p(-uu) * F[16]
    info[:, G["STEPS_CMD"]] = np.where((done_env != 0) | run_out, np.rint(t1 / F[0]), steps_cmd)
    return info, k3[:, 0], t1 / F[0]


def step(K, pre, phys, dtype=np.float64):
    """pre: info_go2 [N,144] (float32, key as raw bits), steps, done, episode_done, episode_metrics [N,24], action [N,12].
    phys: priv [N,123] (elements 48: are read), qpos, qvel, feet_z [N,4], contact [N,4].  Returns every word the step writes
    (`info` without the key, which comes back as uint32 `key`)."""
    T = dtype
    F = K["F"].astype(T)
    dt = F[0]
    key = key_of(pre["info_go2"])
    info = np.asarray(pre["info_go2"], f32).astype(T)
    info[:, G["RNG"]:G["RNG"] + 2] = 0
    action = np.asarray(pre["action"], f32).astype(T)
    pv = np.asarray(phys["priv"], f32).astype(T)
    sl = lambda k: pv[:, P[k][0]:P[k][1]]
    gyro, linvel, gravity, gang, aforce, feet_vel = sl("gyro"), sl("linvel"), sl("gravity"), sl("gang"), sl("aforce"), sl("feet_vel")
    qpos, qvel = np.asarray(phys["qpos"], f32).astype(T), np.asarray(phys["qvel"], f32).astype(T)
    feet_z, contact = np.asarray(phys["feet_z"], f32).astype(T), np.asarray(phys["contact"]) != 0
    out = {}
    info, key = kick_update(K, info, key, T)
    out["xfrc_applied"] = info[:, G["XFRC"]:G["XFRC"] + 3].copy()
    info, out["ctrl"] = action_fifo(K, info, action, T)
    info = imu_fifo(K, info, gyro, linvel, gravity)
    filt = contact | (info[:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4] != 0)
    first_contact = (info[:, G["AIR"]:G["AIR"] + 4] > 0) & filt
    last_contact_old = info[:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4].copy()
    info[:, G["AIR"]:G["AIR"] + 4] += dt
    info[:, G["SWING"]:G["SWING"] + 4] = np.maximum(info[:, G["SWING"]:G["SWING"] + 4], feet_z)
    obs, key = noisy_obs(K, info, key, gyro, linvel, gravity, qpos, qvel, T)
    priv = pv.copy()
    priv[:, :48] = obs
    priv[:, P["jpos"][0]:P["jpos"][1]] = qpos[:, 7:] - K["home"].astype(T)[7:]
    priv[:, P["jvel"][0]:P["jvel"][1]] = qvel[:, 6:]
    priv[:, P["last_contact"][0]:P["last_contact"][1]] = last_contact_old
    priv[:, P["air"][0]:P["air"][1]] = info[:, G["AIR"]:G["AIR"] + 4]
    priv[:, P["xfrc"][0]:P["xfrc"][1]] = info[:, G["XFRC"]:G["XFRC"] + 3]
    priv[:, 122] = (info[:, G["SINCE_PERT"]] >= info[:, G["STEPS_PERT"]]).astype(T)
    rw, done_env, cmd_norm = reward_terms(K, info, action, contact, first_contact, feet_z, gyro, linvel, gravity, gang, qpos, qvel, aforce, feet_vel, T)
    if phys.get("done_env") is not None:                          # the step's own verdict where given (nan: the reference's):
        ov = np.asarray(phys["done_env"], np.float64)             # states inside the up[2] band, envs that AutoReset restored
        done_env = np.where(np.isnan(ov), done_env, (ov != 0).astype(T)).astype(T)
        rw[:, RW_TERM] = done_env
    met = rw * K["SC"].astype(T)
    total = met[:, 0] * 0
    for k in ORDER:
        total = total + met[:, k]
    reward = np.clip(total * dt, T(0), T(10000))
    info[:, G["LAST_LAST_ACT"]:G["LAST_LAST_ACT"] + NU] = info[:, G["LAST_ACT"]:G["LAST_ACT"] + NU]
    info[:, G["LAST_ACT"]:G["LAST_ACT"] + NU] = action
    info, key, t1_over_dt = resample(K, info, key, done_env, T)
    c = contact.astype(T)
    nc = T(1) - c
    info[:, G["AIR"]:G["AIR"] + 4] = (info[:, G["AIR"]:G["AIR"] + 4] + dt) * nc
    info[:, G["CONTACT_T"]:G["CONTACT_T"] + 4] = (info[:, G["CONTACT_T"]:G["CONTACT_T"] + 4] + dt) * c
    info[:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4] = c
    info[:, G["SWING"]:G["SWING"] + 4] *= nc
    sw = info[:, G["SWING"]:G["SWING"] + 4]
    metrics = np.concatenate([met, ((((sw[:, 0] + sw[:, 1]) + sw[:, 2]) + sw[:, 3]) / T(4))[:, None]], 1)
    # Episode / AutoReset wrappers
    steps = np.asarray(pre["steps"], f32).reshape(-1).astype(T)
    done_prev = np.asarray(pre["done"], f32).reshape(-1)
    if K["autoreset"]:
        steps = np.where(done_prev != 0, T(0), steps)
    done, trunc = done_env.copy(), done_env * 0
    em = np.asarray(pre["episode_metrics"], f32).astype(T)
    if K["episode"]:
        steps = steps + T(1)
        over = steps >= T(K["L"])
        trunc = np.where(over, T(1) - done_env, T(0))
        add = np.concatenate([reward[:, None], np.ones_like(reward)[:, None], metrics], 1)
        prev = np.asarray(pre["episode_done"], f32).reshape(-1) != 0
        em = np.where(prev[:, None], T(0), em + add)
        done = np.where(over, T(1), done)
    restored = (done != 0) if K["autoreset"] else np.zeros(done.shape, bool)
    info[restored, G["XFRC"]:G["XFRC"] + 3] = 0
    out.update(info=info, key=key, obs=obs, priv=priv, metrics=metrics, raw_total=total, reward=reward, done_env=done_env, done=done,
               steps=steps, truncation=trunc, episode_done=done, episode_metrics=em, restored=restored, cmd_norm=cmd_norm,
               first_contact=first_contact, t1_over_dt=t1_over_dt)
    return out


METRIC_NAMES = ("tracking_lin_vel", "tracking_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "dof_pos_limits", "pose", "termination",
                "stand_still", "torques", "action_rate", "energy", "feet_clearance", "feet_height", "feet_slip", "feet_air_time",
                "all_feet_air", "symmetric_gait", "lr_symmetry", "fb_symmetry", "feet_off_ground_when_still", "swing_peak")


def from_record(rec):
    """a record a step left (oracle state or device views, numpy) in the terms of step()'s result"""
    info = np.asarray(rec["info_go2"], f32)
    n = len(info)
    col = lambda k: np.asarray(rec[k], f32).reshape(n, -1)[:, 0].astype(np.float64)
    o = dict(info=info.astype(np.float64), key=key_of(info), obs=np.asarray(rec["obs"], f32).astype(np.float64),
             priv=np.asarray(rec["priv_obs"], f32).astype(np.float64), metrics=np.asarray(rec["metrics"], f32).astype(np.float64),
             reward=col("reward"), done=col("done"), steps=col("info_steps"), truncation=col("info_truncation"),
             episode_done=col("info_episode_done"), episode_metrics=np.asarray(rec["info_episode_metrics"], f32).astype(np.float64),
             ctrl=np.asarray(rec["ctrl"], f32).astype(np.float64))
    o["info"][:, G["RNG"]:G["RNG"] + 2] = 0
    return o


def float_quantities(o, K):
    """name -> array of every float-valued quantity a step computes (compared within a tolerance).  Those that need the step's
    physics results (needs_phys) can be compared only for envs that still publish them: AutoReset restores the obs, the privileged obs
    and ctrl of an env that is done."""
    i = o["info"]
    q = {f"metrics/{nm}": o["metrics"][:, k] for k, nm in enumerate(METRIC_NAMES)}
    q.update({"reward": o["reward"], "obs/noisy": o["obs"][:, :33], "priv/noisy": o["priv"][:, :33], "priv/joint_pos": o["priv"][:, 63:75],
              "priv/air_time": o["priv"][:, 115:119], "priv/xfrc": o["priv"][:, 119:122], "ctrl": o["ctrl"], "command": i[:, 0:3],
              "air_time": i[:, G["AIR"]:G["AIR"] + 4], "contact_time": i[:, G["CONTACT_T"]:G["CONTACT_T"] + 4],
              "swing_peak": i[:, G["SWING"]:G["SWING"] + 4], "kick_dir": i[:, G["PERT_DIR"]:G["PERT_DIR"] + 3],
              "kick_force": i[:, G["XFRC"]:G["XFRC"] + 3]})
    if K["episode"]:
        q.update({"episode/sum_reward": o["episode_metrics"][:, 0], "episode/metrics": o["episode_metrics"][:, 2:]})
    return q


def exact_quantities(o, K):
    """name -> array of everything that is PRNG, integer-valued or a copy (compared for equality)"""
    i = o["info"]
    q = {"key": o["key"], "steps_until_next_cmd": i[:, 3], "last_act": i[:, G["LAST_ACT"]:G["LAST_ACT"] + 12],
         "last_last_act": i[:, G["LAST_LAST_ACT"]:G["LAST_LAST_ACT"] + 12], "action_fifo": i[:, G["ACT_BUF"]:G["ACT_BUF"] + 48],
         "imu_fifo": i[:, G["GYRO_BUF"]:G["GRAV_BUF"] + 12], "last_contact": i[:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4],
         "kick_timers": i[:, G["STEPS_PERT"]:G["PERT_STEPS"] + 1], "kick_mag": i[:, G["PERT_MAG"]], "info_tail": i[:, 142:144],
         "obs/last_act_command": o["obs"][:, 33:48], "priv/last_act_command": o["priv"][:, 33:48], "priv/joint_vel": o["priv"][:, 75:87],
         "priv/last_contact": o["priv"][:, 99:103], "priv/kick_flag": o["priv"][:, 122], "done": o["done"], "steps": o["steps"]}
    if K["episode"]:
        q.update({"truncation": o["truncation"], "episode_done": o["episode_done"], "episode/length": o["episode_metrics"][:, 1]})
    return q


def needs_phys(name):
    """whether a quantity of the two tables above is computed from the physics results of the step"""
    return name.split("/")[0] in ("metrics", "reward", "obs", "priv", "ctrl", "air_time", "contact_time", "swing_peak", "episode",
                                  "imu_fifo", "last_contact")


def reward_from_metrics(K, metrics):
    """The reward a step must publish given the 21 scaled terms it published: their float32 sum in ORDER, times dt, clamped.  No libm
    call and no unpublished input is involved, so this is bit for bit what the kernel has to write."""
    m = np.asarray(metrics, f32)
    total = np.zeros(len(m), f32)
    for k in ORDER:
        total = total + m[:, k]
    return np.clip(total * K["F"][0], f32(0), f32(10000))


def episode_sums_from_outputs(K, pre, reward, metrics):
    """The Episode wrapper's sums given the reward and metrics the step published (float32, bit for bit)."""
    add = np.concatenate([np.asarray(reward, f32).reshape(-1, 1), np.ones((len(metrics), 1), f32), np.asarray(metrics, f32)], 1)
    prev = np.asarray(pre["episode_done"], f32).reshape(-1) != 0
    return np.where(prev[:, None], f32(0), np.asarray(pre["episode_metrics"], f32) + add)
