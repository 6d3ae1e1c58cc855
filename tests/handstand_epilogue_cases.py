"""Branch classes of the Go2 Handstand / Footstand step outside the physics, the config variants they are run under, and one census
predicate per class.  A predicate looks at `d`: the record before the step (`pre`), the reference's verdicts on the record the step
left (`r`: cause_up, cause_energy, unwanted, feet, done_env, reward, restored ...), the published joint angles and imu height, and --
on the variants with one substep, where the last forward pass runs at the fixture's own pose -- the fixture's per-pair contact data.
tests/golden/make_handstand_epilogue_states.py builds states for the classes; the tests assert every class is reached."""
import numpy as np

import handstand_epilogue_ref as R

f32 = np.float32
EPISODE_LENGTH = 500
MIN_PER_CLASS = 8
MAX_EXCLUDED = 0.02          # of the states, whatever the cause (none is excluded where n_frames = 1)
NCON_CAP = 12                # HandDims::NCON: the contact list the physics sees
TASKS = {"Go2Handstand": "handstand", "Go2Footstand": "footstand"}
# tests/test_planeprim_gpu.py holds the device's plane-capsule / -cylinder / -sphere dist to this of the float64 oracle's
PLANEPRIM_DIST_BOUND = 2e-5
# The generator keeps every penetration / clearance of a pair at least this far from 0 (metres): 200 x the contact band, and shallow
# enough that the contact forces of one substep stay moderate.
POSE_MARGIN = 4e-3
# No geom that starts this far above the floor touches it within one env-step: the fixture's joints turn at 9 rad/s at the most, a leg
# is 0.45 m long, free fall adds 0.2 m/s in 20 ms: 4.3 m/s x 0.02 s = 0.09 m.  The device's word on contact is not asked there.
REACH = 0.2
UP2_NEAR = 0.01              # "just on either side of -0.25": |up[2] + 0.25| below this

# Eleven distinct non-zero scales: no term hides behind a zero.  The magnitudes keep every term's share of a standing robot's total
# between 1e-3 and 1 (torques^2 ~ 1e2, dof_acc ~ 1e4 .. 1e9, energy ~ 1e1).
_ALL = {"height": 1.0, "orientation": 0.7, "contact": -0.1, "action_rate": -0.01, "termination": -2.0, "dof_pos_limits": -0.5,
        "torques": -2e-4, "pose": -0.15, "stay_still": -0.3, "energy": -1e-3, "dof_acc": -2.5e-7}
# below zero for every state that carries any torque: torques^2 of a standing robot is 50 .. 500
_NEGATIVE = {**_ALL, "torques": -1.0, "height": 0.3}
# above 1e4 / dt = 5e5 (2.5e6 at n_frames = 1 ... the height term is exp(-(z_des - h)) >= exp(-0.55) = 0.58, so 1e8 x 0.58 clears both)
_LARGE = {**_ALL, "height": 1.0e8}
_NOISE = {"level": 1.0, "scales": {"joint_pos": 0.03, "joint_vel": 1.1, "gyro": 0.25, "gravity": 0.07, "linvel": 0.13}}
ENERGY_THRESHOLD = 400.0     # W; the fixture's energetic states carry 12 x ~17 Nm x 8 rad/s ~ 1600, a standing robot below 100
_FWD = (0.36, 0.48, -0.8)    # a unit vector with x and y


def _v(scales=None, length=0, auto=False, nf1=False, energy=None, fwd=None, noise=None, clamp="none", term=None):
    over = {}
    if scales is not None:
        over["reward_config"] = {"scales": dict(scales)}
    if term is not None:
        over.setdefault("reward_config", {"scales": {}})["scales"]["termination"] = term
    if nf1:
        over["ctrl_dt"] = 0.004                                     # = sim_dt: n_frames = 1
    if energy is not None:
        over["energy_termination_threshold"] = energy
    if noise is not None:
        over["noise_config"] = noise
    return dict(over=over, length=length, auto=auto, fwd=fwd, clamp=clamp)


# Every wrapper stack (plain, Episode, Episode + AutoReset), the shipped forward vectors and a general one, the shipped noise (level 1,
# five distinct scales) and another set, n_frames = 5 and 1 (twice), a finite energy threshold, and both clamps occur.  Every variant has
# non-zero contact and termination scales: the device's flags can be read off its metrics where the reference cannot form them.
VARIANTS = {
    "shipped_autoreset": _v(term=-1.0, length=EPISODE_LENGTH, auto=True),
    "allscales_energy_plain": _v(_ALL, energy=ENERGY_THRESHOLD, noise=_NOISE),
    "nf1_allscales_energy_episode": _v(_ALL, length=EPISODE_LENGTH, nf1=True, energy=ENERGY_THRESHOLD, noise=_NOISE),
    "nf1_negative_autoreset": _v(_NEGATIVE, length=EPISODE_LENGTH, auto=True, nf1=True, clamp="low"),
    "fwd_large_episode": _v(_LARGE, length=EPISODE_LENGTH, fwd=_FWD, clamp="high"),
}

# Reset keys whose bernoulli draw uniform(split(key)[1]) is 0.0f (the first four) or 0.5f (the last four) exactly, found by a search over
# PRNGKey-like pairs (7, i): `ub < p` and `ub <= p` part on them at init_from_crouch = 0 and 0.5.
EDGE_KEYS = np.array([[7, 2751938], [7, 14965073], [7, 19348380], [7, 26114981], [7, 15271647], [7, 29993582], [7, 51722022], [7, 54719321]], np.uint32)


def reset_keys(n):
    from rsr_mjx_amd import prng
    return np.concatenate([EDGE_KEYS, prng.split(prng.PRNGKey(77), n - len(EDGE_KEYS))])


RECORD = ("qpos", "qvel", "ctrl", "qacc_warmstart", "time", "info_go2", "info_steps", "done", "info_episode_done", "info_episode_metrics")
FIRST = {"qpos": "first_qpos", "qvel": "first_qvel", "ctrl": "first_ctrl", "qacc_warmstart": "first_warmstart", "time": "first_time",
         "xpos": "first_xpos", "site_xpos": "first_site_xpos", "obs": "first_obs", "priv_obs": "first_priv_obs"}
READ = RECORD + ("xpos", "site_xpos", "obs", "priv_obs", "metrics", "reward", "info_truncation")
# the words a step with noise level 0 may write differently: the observation and its copies; the physics must not read the noise
NOISY_WORDS = ("obs", "priv_obs", "first_obs", "first_priv_obs")


def variant_config(name, quiet=False):
    from rsr_mjx_amd.envs import config
    c = config._merge(config.HANDSTAND_DEFAULT_CONFIG, VARIANTS[name]["over"])
    if quiet:
        c = config._merge(c, {"noise_config": {"level": 0.0}})
    return c


def patch_fields(name, fields):
    """the env fields no config entry reaches: the desired forward vector belongs to the task, not to the config"""
    fwd = VARIANTS[name]["fwd"]
    if fwd is not None:
        fields["env_go2f"] = fields["env_go2f"].copy()
        fields["env_go2f"][R.F_FWD:R.F_FWD + 3] = np.asarray(fwd, f32)
    return fields


def variant_fields(model, task, name, auto_reset=None, quiet=False):
    """(merged config, env fields) of a variant on a compiled Go2 model that carries the base.py overrides; auto_reset=False gives the
    variant's twin without AutoReset, whose done envs still publish what the step computed; quiet: noise level 0"""
    from rsr_mjx_amd.envs import config
    v = VARIANTS[name]
    c = variant_config(name, quiet)
    auto = v["auto"] if auto_reset is None else auto_reset
    return c, patch_fields(name, config.handstand_env_fields(model, c, v["length"], auto, variant=TASKS[task]))


def variant_constants(model, task, name, auto_reset=None):
    K = R.constants(variant_fields(model, task, name, auto_reset)[1], model)
    K["clamp"], K["general_fwd"], K["task"] = VARIANTS[name]["clamp"], VARIANTS[name]["fwd"] is not None, task
    return K


def device_env(task, name, n, auto_reset=None, quiet=False):
    """the batched HIP env of a variant (the forward vector patched into the fields its blob is packed from)"""
    from rsr_mjx_amd.envs import go2
    v = VARIANTS[name]
    over = dict(v["over"])
    if quiet:
        over["noise_config"] = {**over.get("noise_config", {}), "level": 0.0}
    jenv = go2.load(task, config_overrides=over)
    inner = jenv._fields_fn
    jenv._fields_fn = lambda sys, episode_length=0, auto_reset=False, **kw: patch_fields(name, inner(sys, episode_length, auto_reset, **kw))
    return jenv, jenv.batched(n, episode_length=v["length"], auto_reset=v["auto"] if auto_reset is None else auto_reset)


def before_of(rec, action):
    """the part of a record a step reads, in the reference's terms"""
    return dict(qpos=rec["qpos"], info_go2=rec["info_go2"], ctrl=rec["ctrl"], steps=rec["info_steps"], done=rec["done"],
                episode_done=rec["info_episode_done"], episode_metrics=rec["info_episode_metrics"], action=action)


def phys_of(K, model, after, quiet, fx, flags_from=None):
    """What the reference takes from the records a step left: the published physics results, the clean gravity of the quiet twin and the
    contact flags.  n_frames = 1: the flags of the fixture's float64 pair distances, all 30 pairs.  n_frames > 1: the pose of the last
    forward pass is the device's, and so are the flags, read off the metrics `flags_from` (the contact term; the termination term
    where neither the up vector nor the energy ends the episode, and then `unwanted` changes nothing the step writes) -- except for
    the states every pair of which starts more than REACH above the floor: they touch nothing, whatever the metrics say."""
    n = len(after["qpos"])
    imu = int(K["ids"][0])
    p = dict(priv=after["priv_obs"], qpos=after["qpos"], qvel=after["qvel"], qacc=after["qacc_warmstart"],
             height=np.asarray(after["site_xpos"]).reshape(n, -1, 3)[:, imu, 2], gravity=np.asarray(quiet["obs"])[:, 6:9],
             fwd_xy=R.imu_forward_xy(K, model, after["qpos"], after["qvel"]) if K["general_fwd"] else None)
    if K["n_frames"] == 1:
        p["unwanted"], p["feet"] = R.flags_from_pairs(K, fx["pair_dist"])
    else:
        m = np.asarray(flags_from, f32)
        assert K["SC"][R.HM_CONTACT] != 0 and K["SC"][R.HM_TERM] != 0
        clear = np.asarray(fx["pair_dist"]).min(1) > REACH
        p["unwanted"], p["done_env_given"], p["clear"], p["feet"] = None, m[:, R.HM_TERM] != 0, clear, (m[:, R.HM_CONTACT] != 0) & ~clear
    return p


# ---- classes ----
_JOINT = {"hip": 0, "thigh": 1, "calf": 2}
GROUPS = {"hip": 1, "thigh": 2, "calf": 3}                          # fixture pair_group: 0 trunk, 1 hip, 2 thigh, 3 calf, 4 foot


def _limit(d, kind, side):
    q = np.asarray(d["qpos"], f32)[:, 7:]
    j = np.arange(12) % 3 == _JOINT[kind]
    lo, hi = (q < d["K"]["soft"][:12]) & j, (q > d["K"]["soft"][12:]) & j
    return {"low": lo.any(1), "high": hi.any(1), "inside": ~(lo | hi).any(1)}[side]


def _alone(d):
    return d["r"]["unwanted"] & ~d["r"]["cause_up"] & ~d["r"]["cause_energy"]


def _group_alone(d, g):
    unw = d["touch"] & (d["K"]["pair_class"] == 1)
    return _alone(d) & (unw & (d["pair_group"] == GROUPS[g])).any(1) & ~(unw & (d["pair_group"] != GROUPS[g])).any(1)


def _foot_alone(d, k):
    feet = np.flatnonzero(d["K"]["pair_class"] == 2)
    return d["touch"][:, feet[k]] & ~d["touch"][:, feet[1 - k]]


def _cap(d, cls, late):
    """more penetrating points than the cap; exactly one pair of the class touches; none / all of its points among the first twelve"""
    mine = d["touch"] & (d["K"]["pair_class"] == cls)
    seen = (d["seen12"] & mine).any(1)
    cut = (d["cut12"] & mine).any(1)                                # some of its points beyond the twelfth
    return (d["npen"] > NCON_CAP) & (mine.sum(1) == 1) & ((~seen) if late else (seen & ~cut))


def _if(cond, pred):
    pred.applies = cond
    return pred


_always = lambda K: True
_nf1 = lambda K: K["n_frames"] == 1
_episode = lambda K: K["episode"]
_auto = lambda K: K["autoreset"]
_finite = lambda K: K["F"][R.F_ENERGY] < 1e30
_last = lambda d: (np.asarray(d["pre"]["steps"]).reshape(-1) == EPISODE_LENGTH - 1) & ((np.asarray(d["pre"]["done"]).reshape(-1) == 0) | (not d["K"]["autoreset"]))
# Handstand's unwanted geoms are the front legs', pairs 2..7 and 9..14.  The pairs before and between them that are not unwanted are
# the two trunk cylinders (3 points each) and the FR foot (1): at most 7 points can precede an unwanted pair, so the capped
# list of 12 never hides the only touching one.  Footstand's (the rear legs', pairs 16..21 and 23..28) come last.
_cap_unwanted_late = lambda K: K["n_frames"] == 1 and K["task"] == "Go2Footstand"

CLASSES = {
    "done_up_far": lambda d: d["r"]["cause_up"] & ~d["r"]["unwanted"] & ~d["r"]["cause_energy"] & (d["r"]["up2"] < -0.3),
    "done_up_just_below": lambda d: d["r"]["cause_up"] & (d["r"]["up2"] > -0.25 - UP2_NEAR),
    "up_just_above": lambda d: ~d["r"]["cause_up"] & (d["r"]["up2"] < -0.25 + UP2_NEAR),
    "done_unwanted_alone": _alone,
    **{f"done_unwanted_{g}": _if(_nf1, (lambda g: lambda d: _group_alone(d, g))(g)) for g in GROUPS},
    "done_energy_alone": _if(_finite, lambda d: d["r"]["cause_energy"] & ~d["r"]["cause_up"] & ~d["r"]["unwanted"]),
    "no_cause": lambda d: d["r"]["done_env"] == 0,
    **{f"cost_foot{k}_alone": _if(_nf1, (lambda k: lambda d: _foot_alone(d, k))(k)) for k in (0, 1)},
    "feet_touch": lambda d: d["r"]["feet"],
    "feet_clear": lambda d: ~d["r"]["feet"],
    "height_below": lambda d: np.asarray(d["height"], f32) < d["K"]["F"][R.F_ZDES],
    "height_at_or_above": lambda d: np.asarray(d["height"], f32) >= d["K"]["F"][R.F_ZDES],
    **{f"limit_{kind}_{side}": (lambda kind, side: lambda d: _limit(d, kind, side))(kind, side) for kind in _JOINT for side in ("low", "high", "inside")},
    "reward_clamped_low": _if(lambda K: K["clamp"] == "low", lambda d: (d["r"]["raw_total"] < 0) & (d["r"]["reward"] == 0)),
    "reward_clamped_high": _if(lambda K: K["clamp"] == "high", lambda d: d["r"]["reward"] == 1e4),
    "reward_unclamped": _if(lambda K: K["clamp"] == "none", lambda d: (d["r"]["reward"] > 0) & (d["r"]["reward"] < 1e4)),
    "last_step": _if(_episode, lambda d: _last(d) & (d["r"]["done_env"] == 0)),
    "last_step_done": _if(_episode, lambda d: _last(d) & (d["r"]["done_env"] != 0)),
    "prev_episode_done": _if(_episode, lambda d: np.asarray(d["pre"]["episode_done"]).reshape(-1) != 0),
    "prev_done": _if(_auto, lambda d: np.asarray(d["pre"]["done"]).reshape(-1) != 0),
    "restored": _if(_auto, lambda d: d["r"]["restored"]),
    "cap_unwanted_late": _if(_cap_unwanted_late, lambda d: _cap(d, 1, True)),
    "cap_unwanted_early": _if(_nf1, lambda d: _cap(d, 1, False)),
    "cap_foot_late": _if(_nf1, lambda d: _cap(d, 2, True)),
    "cap_foot_early": _if(_nf1, lambda d: _cap(d, 2, False)),
}


def census(K, pre, r, phys, fx):
    """{class: number of states in it}; classes that do not apply to this variant are left out.  `r`: the reference's result on the
    record under test, `phys` what it was fed."""
    d = dict(K=K, pre=pre, r=r, qpos=phys["qpos"], height=phys["height"], touch=np.asarray(fx["pair_dist"]) < 0, seen12=fx["seen12"] != 0,
             cut12=fx["cut12"] != 0, npen=fx["npen"], pair_group=np.asarray(fx["pair_group"]))
    return {name: int(np.count_nonzero(p(d))) for name, p in CLASSES.items() if getattr(p, "applies", _always)(K)}


# ---- the comparison both test modules make ----
FACTOR = 4                  # x the recorded ref32-ref64 distance: the device's expf differs from numpy's by an ulp or two
ULPS = 2                    # + this many float32 ulp of the quantity's magnitude (the stored value is a float32)
# Float quantities that pass through libm (expf of the height term) or add such a quantity up: the float32 reference need not give the
# kernel's (or the oracle's) bits there.  Everywhere else the env algebra is compiled with contraction off and the float32 reference
# restates it operation by operation, so it must be bit-identical.
NOT_BITWISE = ("metrics/height", "reward", "episode/sum_reward", "episode/metrics")
# with a general forward vector R[0], R[3] are reconstructed: the orientation term too (its share is recorded in the tolerances file)
NOT_BITWISE_GENERAL_FWD = NOT_BITWISE + ("metrics/orientation",)


def not_bitwise(K):
    return NOT_BITWISE_GENERAL_FWD if K["general_fwd"] else NOT_BITWISE


def share_allowance(K, share, name, shape):
    """what the reconstruction of R[0], R[3] may add to a quantity's distance: `share` (recorded, in units of the orientation metric)
    on the orientation, reward and sums of the variant with a general forward vector, zero everywhere else"""
    out = np.zeros(shape)
    if not K["general_fwd"]:
        return out
    dt = float(K["F"][R.F_DT])
    if name == "metrics/orientation":
        out = out + share
    elif name in ("reward", "episode/sum_reward"):
        out = out + share * dt
    elif name == "episode/metrics":
        out[:, R.HM_ORIENT] += share
    return out


def compare(K, tol, share, ref, got, live):
    """(failures, report): every float quantity of `got` within FACTOR x tol + ULPS ulp32 (+ the reconstruction's share) of the float64
    reference `ref`, every exact quantity equal.  `live`: envs whose record still holds what the step computed (not restored by
    AutoReset); the others are compared in what AutoReset does not restore."""
    fails, report = [], {}
    rf, gf = R.float_quantities(ref, K), R.float_quantities(got, K)
    for nm in rf:
        sel = live if R.needs_phys(nm) else np.ones(len(live), bool)
        a, b = np.asarray(gf[nm], np.float64), np.asarray(rf[nm], np.float64)
        bound = FACTOR * tol[nm] + ULPS * np.spacing(np.abs(b).astype(f32)).astype(np.float64) + share_allowance(K, share, nm, b.shape)
        dist = np.abs(a - b)
        ratio = np.where(dist == 0, 0.0, dist / bound)[sel]
        report[nm] = (float(dist[sel].max()) if dist[sel].size else 0.0, float(ratio.max()) if ratio.size else 0.0)
        if ratio.size and not (ratio <= 1).all():
            w = np.flatnonzero(sel)[np.argmax(ratio.reshape(ratio.shape[0], -1).max(1))]
            fails.append(f"{nm}: |got - ref64| = {report[nm][0]:.3e} is {report[nm][1]:.2f} x its bound (env {int(w)})")
    re_, ge = R.exact_quantities(ref, K), R.exact_quantities(got, K)
    for nm in re_:
        sel = live if R.needs_phys(nm) else np.ones(len(live), bool)
        ne = np.asarray(re_[nm])[sel] != np.asarray(ge[nm])[sel]
        if ne.any():
            rows = np.flatnonzero(sel)[np.flatnonzero(ne.reshape(ne.shape[0], -1).any(1))]
            fails.append(f"{nm}: not equal in {len(rows)} envs, first {rows[:5].tolist()}")
    return fails, report


def bitwise(K, r32, got, live):
    """{quantity: the float32 reference and the record agree bit for bit}"""
    g32, gq = R.float_quantities(r32, K), R.float_quantities(got, K)
    out = {}
    for nm in g32:
        sel = live if R.needs_phys(nm) else slice(None)
        out[nm] = bool((np.asarray(g32[nm], f32)[sel] == np.asarray(gq[nm], f32)[sel]).all())
    return out
