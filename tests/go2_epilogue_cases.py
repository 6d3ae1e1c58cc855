"""Branch classes of the Go2 joystick step's prologue / epilogue, the config variants they are run under, and one census predicate per
class.  A predicate looks at a record pair: `b` the record before the step (qpos, info_go2, info_steps, done, info_episode_done) and `a` what
the step left (info_go2, metrics, reward, done, qpos, and `restored`: AutoReset put the first state back, so qpos is not the step's).
Everything a predicate reads survives AutoReset (info and metrics are never restored), so the census can be taken from the device's
own record.  tests/golden/make_go2_epilogue_states.py builds states for the classes; the tests assert every class is reached."""
import numpy as np

from go2_epilogue_ref import G, RW_DOF_LIMITS, RW_FEET_OFF_STILL, RW_STAND_STILL, RW_TERM

f32 = np.float32
EPISODE_LENGTH = 1000
MIN_PER_CLASS = 8
NORM_MARGIN = 1e-4          # |cmd_norm - 0.01| of every state whose norm is not 0.01f exactly
HALF_MARGIN = 1e-4          # distance of t1 / dt from a half-integer for every timer draw a state can take
UP2_BAND = 1e-3             # |gravity[2]| below this: the sign of up[2] is not the reference's to call

_KICK = {"pert_config": {"enable": True, "kick_wait_times": [0.1, 0.4], "velocity_kick": [1.0, 4.0]}}
# the large tracking scale takes the total beyond the upper clamp; pose is 0 in the default config, where its term cannot be seen
_LARGE = {"reward_config": {"scales": {"tracking_lin_vel": 1.0e6, "pose": 0.5}}}


def _delay(a, i):
    return {"delay_config": {"action": {"enable": True, "steps": a}, "imu": {"enable": True, "steps": i}}}


def _m(*ds):
    out = {}
    for d in ds:
        for k, v in d.items():
            out[k] = {**out.get(k, {}), **v} if isinstance(v, dict) else v
    return out


# name -> (config overrides, episode_length, auto_reset).  Every delay pair, kicks on and off, the large scale and each wrapper
# stack (plain, Episode, Episode + AutoReset) occur; the states are the same in all of them.
VARIANTS = {
    "d33_autoreset": (_delay(3, 3), EPISODE_LENGTH, True),
    "d00_kicks_episode": (_m(_delay(0, 0), _KICK), EPISODE_LENGTH, False),
    "d12_kicks_autoreset": (_m(_delay(1, 2), _KICK), EPISODE_LENGTH, True),
    "d21_plain": (_delay(2, 1), 0, False),
    "d33_kicks_large_episode": (_m(_delay(3, 3), _KICK, _LARGE), EPISODE_LENGTH, False),
}

# soft limits are 0.95 x jnt_range; joints per leg: hip, thigh, calf
_JOINT = {"hip": 0, "thigh": 1, "calf": 2}


def _cmd_norm(b):
    c = b["info_go2"][:, :3].astype(f32)
    return np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])


def _env_done(a, K):
    return a["metrics"][:, RW_TERM] != 0 if K["SC"][RW_TERM] != 0 else a["done"] != 0


def _limit(a, K, kind, side):
    q = a["qpos"][:, 7:].astype(f32)
    j = np.arange(12) % 3 == _JOINT[kind]
    beyond = (q < K["soft"][:12]) if side == "low" else (q > K["soft"][12:])
    return (beyond & j).any(1) & ~a["restored"] & (a["metrics"][:, RW_DOF_LIMITS] != 0)


def _up2(b):
    """z of the trunk's up vector in the record before the step (a step turns it by a degree or two at the most)"""
    q = b["qpos"][:, 3:7].astype(np.float64)
    return 1.0 - 2.0 * (q[:, 1] ** 2 + q[:, 2] ** 2) / (q ** 2).sum(1)


def _kicking(b):
    return b["info_go2"][:, G["SINCE_PERT"]] >= b["info_go2"][:, G["STEPS_PERT"]]


def _nair(a):
    return 4 - (a["info_go2"][:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4] != 0).sum(1)


def _foot(f, kind):
    def pred(b, a, K):
        air0 = b["info_go2"][:, G["AIR"] + f] > 0
        lc0 = b["info_go2"][:, G["LAST_CONTACT"] + f] != 0
        c = a["info_go2"][:, G["LAST_CONTACT"] + f] != 0
        return {"first_touch": air0 & c, "filter": air0 & ~c & lc0, "ground": ~air0 & c}[kind]
    return pred


def _steps_cmd(k, done):
    return lambda b, a, K: (b["info_go2"][:, G["STEPS_CMD"]] == k) & (_env_done(a, K) == done)


def _if(cond, pred):
    pred.applies = cond
    return pred


_always = lambda K: True
_kicks = lambda K: bool(K["I"][2])
_episode = lambda K: K["episode"]
_large = lambda K: K["SC"][0] > 1e5

CLASSES = {
    "cmd_zero": lambda b, a, K: _cmd_norm(b) == 0,
    "cmd_just_still": lambda b, a, K: (_cmd_norm(b) > 0.0095) & (_cmd_norm(b) < f32(0.01)),
    "cmd_just_moving": lambda b, a, K: (_cmd_norm(b) > f32(0.01)) & (_cmd_norm(b) < 0.0105),
    "cmd_moving": lambda b, a, K: _cmd_norm(b) > 0.1,
    "cmd_exactly_threshold": lambda b, a, K: _cmd_norm(b) == f32(0.01),
    "stand_still_nonzero": lambda b, a, K: a["metrics"][:, RW_STAND_STILL] != 0,
    "feet_off_still_nonzero": lambda b, a, K: a["metrics"][:, RW_FEET_OFF_STILL] != 0,
    **{f"steps_cmd_{k}{'_done' if d else ''}": _steps_cmd(k, d) for k in (0, 1, 2) for d in (False, True)},
    **{f"foot{f}_{kind}": _foot(f, kind) for f in range(4) for kind in ("first_touch", "filter", "ground")},
    **{f"nair_{k}": (lambda k: lambda b, a, K: _nair(a) == k)(k) for k in (0, 2, 3, 4)},
    **{f"limit_{kind}_{side}": (lambda kind, side: lambda b, a, K: _limit(a, K, kind, side))(kind, side)
       for kind in _JOINT for side in ("low", "high")},
    "upside_down": lambda b, a, K: _env_done(a, K) & (_up2(b) < -0.5),
    "side_up": lambda b, a, K: ~_env_done(a, K) & (_up2(b) > 0) & (_up2(b) < 0.4),
    "side_down": lambda b, a, K: _env_done(a, K) & (_up2(b) < 0) & (_up2(b) > -0.4),
    "reward_positive": lambda b, a, K: (a["reward"] > 0) & (a["reward"] < 1e4),
    "reward_clamped_low": _if(lambda K: not _large(K), lambda b, a, K: a["reward"] == 0),
    "reward_clamped_high": _if(_large, lambda b, a, K: a["reward"] == 1e4),
    "kick_waiting": _if(_kicks, lambda b, a, K: b["info_go2"][:, G["SINCE_PERT"]] + 1 < b["info_go2"][:, G["STEPS_PERT"]]),
    "kick_start": _if(_kicks, lambda b, a, K: ~_kicking(b) & (b["info_go2"][:, G["SINCE_PERT"]] + 1 >= b["info_go2"][:, G["STEPS_PERT"]])),
    "kick_mid": _if(_kicks, lambda b, a, K: _kicking(b) & (b["info_go2"][:, G["PERT_STEPS"]] < b["info_go2"][:, G["PERT_DUR"]])),
    "kick_last": _if(_kicks, lambda b, a, K: _kicking(b) & (b["info_go2"][:, G["PERT_STEPS"]] >= b["info_go2"][:, G["PERT_DUR"]])),
    "kick_done": _if(_kicks, lambda b, a, K: _kicking(b) & _env_done(a, K)),
    "last_step": _if(_episode, lambda b, a, K: (b["info_steps"] == EPISODE_LENGTH - 1) & (b["done"] == 0) & ~_env_done(a, K)),
    "last_step_done": _if(_episode, lambda b, a, K: (b["info_steps"] == EPISODE_LENGTH - 1) & (b["done"] == 0) & _env_done(a, K)),
    "prev_episode_done": _if(_episode, lambda b, a, K: b["info_episode_done"] != 0),
    "prev_done": lambda b, a, K: b["done"] != 0,
}


def census(K, before, after):
    """{class: number of states in it}; classes that do not apply to this variant are left out."""
    flat = lambda d: {k: (np.asarray(v).reshape(len(v), -1)[:, 0] if k in ("info_steps", "done", "info_episode_done", "reward") else np.asarray(v))
                      for k, v in d.items()}
    b, a = flat(before), flat(after)
    return {name: int(np.count_nonzero(p(b, a, K))) for name, p in CLASSES.items() if getattr(p, "applies", _always)(K)}


# ---- plumbing shared by the generator and the tests ----
RECORD = ("qpos", "qvel", "ctrl", "qacc_warmstart", "time", "info_go2", "info_steps", "done", "info_episode_done", "info_episode_metrics")


def variant_fields(model, name, auto_reset=None):
    """(merged config, env fields) of a variant on a compiled Go2 model that carries the base.py overrides; auto_reset=False gives
    the variant's twin without AutoReset, whose done envs still publish what the step computed"""
    from rsr_mjx_amd.envs import config
    over, length, auto = VARIANTS[name]
    auto = auto if auto_reset is None else auto_reset
    c = config._merge(config.GO2_DEFAULT_CONFIG, over)
    return c, config.go2_env_fields(model, c, length, auto)


def variant_constants(model, name, auto_reset=None):
    import go2_epilogue_ref as R
    _, length, auto = VARIANTS[name]
    return R.constants(variant_fields(model, name)[1], length, auto if auto_reset is None else auto_reset)


def before_of(rec, action):
    """the part of a record a step reads, in the reference's terms"""
    return dict(qpos=rec["qpos"], info_go2=rec["info_go2"], steps=rec["info_steps"], info_steps=rec["info_steps"], done=rec["done"],
                episode_done=rec["info_episode_done"], info_episode_done=rec["info_episode_done"],
                episode_metrics=rec["info_episode_metrics"], action=action)


def phys_of(after, feet_sites):
    """what the reference takes from the record a step left: the published physics results and the step's contact flags"""
    sx = np.asarray(after["site_xpos"]).reshape(len(after["qpos"]), -1, 3)
    return dict(priv=after["priv_obs"], qpos=after["qpos"], qvel=after["qvel"], feet_z=sx[:, feet_sites, 2],
                contact=after["info_go2"][:, G["LAST_CONTACT"]:G["LAST_CONTACT"] + 4])


def after_of(after, restored):
    return dict(info_go2=after["info_go2"], metrics=after["metrics"], reward=after["reward"], done=after["done"], qpos=after["qpos"],
                restored=restored)


# ---- the comparison both test modules make ----
FACTOR = 4                  # x the recorded ref32-ref64 distance: the device's expf / sinf / cosf / log1pf differ from numpy's by a few ulp
ULPS = 2                    # + this many float32 ulp of the quantity's magnitude (the stored value is a float32)
# The reference derives up[0]^2 + up[1]^2 and glin[2] from the gravity sensor.  Both identities assume the third row of R has unit
# norm, which a float32 R built from a float32 quaternion has to a few ulp only: the quaternion's norm^2 is off by <= 2 ulp(1), the
# row's norm^2 by twice that, and each of the row's entries carries ~1 ulp from its own products.  8 ulp32(1) bounds the defect.
ROW_DEFECT = 8 * 2.0 ** -23
# Float quantities that pass through libm (expf, sinf, cosf) or the identities, or add such quantities up: the float32 reference
# need not give the kernel's (or the oracle's) bits there.  Everywhere else the env algebra is compiled with contraction off and the
# float32 reference restates it operation by operation, so it must be bit-identical.
NOT_BITWISE = ("metrics/tracking_lin_vel", "metrics/tracking_ang_vel", "metrics/pose", "metrics/lin_vel_z", "metrics/orientation", "reward",
               "episode/sum_reward", "episode/metrics", "kick_dir", "kick_force", "priv/xfrc")
CONTACT_BAND = 1e-7         # |foot z - radius| below this (3 ulp32 of a body position of 0.3 .. 0.6 m, from which the foot's is built)


def identity_allowance(K, phys, name, shape):
    """what the two identities may add to a quantity's distance (zero for quantities that do not go through them)"""
    import go2_epilogue_ref as R
    pv = np.asarray(phys["priv"], np.float64)
    g, lin = pv[:, 54:57], pv[:, 57:60]
    vnorm = np.sqrt((lin ** 2).sum(1))
    glin2 = np.abs((g * lin).sum(1))
    dz = (ROW_DEFECT + 3 * 2.0 ** -24) * vnorm                       # glin[2] itself, + the rounding of the three products
    a_or = abs(float(K["SC"][R.RW_ORIENT])) * ROW_DEFECT
    a_lz = abs(float(K["SC"][R.RW_LIN_VEL_Z])) * (2 * glin2 * dz + dz * dz)
    dt = float(K["F"][0])
    out = np.zeros(shape)
    if name == "metrics/orientation":
        out = out + a_or
    elif name == "metrics/lin_vel_z":
        out = out + a_lz
    elif name in ("reward", "episode/sum_reward"):
        out = out + (a_or + a_lz) * dt
    elif name == "episode/metrics":
        out[:, R.RW_ORIENT] += a_or
        out[:, R.RW_LIN_VEL_Z] += a_lz
    return out


def compare(K, tol, phys, ref, got, live):
    """(failures, report): every float quantity of `got` within FACTOR x tol + ULPS ulp32 (+ the identities' share) of the float64
    reference `ref`, every exact quantity equal.  `live`: envs whose record still holds what the step computed (not restored by
    AutoReset); the others are compared in what does not need the physics results."""
    import go2_epilogue_ref as R
    fails, report = [], {}
    rf, gf = R.float_quantities(ref, K), R.float_quantities(got, K)
    for nm in rf:
        sel = live if R.needs_phys(nm) else np.ones(len(live), bool)
        a, b = np.asarray(gf[nm], np.float64), np.asarray(rf[nm], np.float64)
        bound = FACTOR * tol[nm] + ULPS * np.spacing(np.abs(b).astype(f32)).astype(np.float64) + identity_allowance(K, phys, nm, b.shape)
        d = np.abs(a - b)
        ratio = np.where(d == 0, 0.0, d / bound)[sel]
        report[nm] = (float(d[sel].max()) if d[sel].size else 0.0, float(ratio.max()) if ratio.size else 0.0)
        if ratio.size and not (ratio <= 1).all():
            w = np.flatnonzero(sel)[np.argmax(ratio.reshape(ratio.shape[0], -1).max(1))]
            fails.append(f"{nm}: |device - ref64| = {report[nm][0]:.3e} is {report[nm][1]:.2f} x its bound (env {int(w)})")
    re_, ge = R.exact_quantities(ref, K), R.exact_quantities(got, K)
    for nm in re_:
        sel = live if R.needs_phys(nm) else np.ones(len(live), bool)
        ne = np.asarray(re_[nm])[sel] != np.asarray(ge[nm])[sel]
        if ne.any():
            rows = np.flatnonzero(sel)[np.flatnonzero(ne.reshape(ne.shape[0], -1).any(1))]
            fails.append(f"{nm}: not equal in {len(rows)} envs, first {rows[:5].tolist()}")
    return fails, report
