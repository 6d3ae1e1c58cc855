"""Branch classes of the Airbot step's prologue / epilogue (cube, sf, T-shape), the config variants they are run under, one census
predicate per class, and the comparison both test modules make.  A predicate looks at `b`, the record before the step (plus the
action), `a`, what the step left, and `r`, the float32 reference (tests/airbot_epilogue_ref.py) evaluated on that pair: its gate
quantities are the step's own float32 values.  Everything a predicate reads survives AutoReset (info words and metrics are never
restored), so the census can be taken from the device's own record.  tests/golden/make_airbot_epilogue_states.py builds states for
the classes; the tests assert every class is reached."""
import numpy as np

import airbot_epilogue_ref as R

f32 = np.float32
EPISODE_LENGTH = 7
MIN_PER_CLASS = 8
KINDS = R.KINDS

# name -> (env kwargs, episode_length, auto_reset).  The weights variant reaches both sides of the +-100 clamp: the push term is
# ~ +400 near the target (and siet = -400 inside the dead zone or 0 far from it), so totals run from below -100 to above +100.
VARIANTS = {
    "plain": ({}, 0, False),
    "episode": ({}, EPISODE_LENGTH, False),
    "autoreset": ({}, EPISODE_LENGTH, True),
    "weights_episode": ({"push_reward_weight": 400.0, "siet_to_box_reward_weight": -400.0}, EPISODE_LENGTH, False),
    "nframes1": ({"n_frames": 1}, 0, False),
}
NCON_CAP = {"cube": 24, "sf": 24, "tshape": 32}     # Dims::NCON of the kernels (dims.ncon_max on the device): the oracle drops contacts alike
GATE_Z = {"cube": 0.82, "sf": 0.82, "tshape": 0.83}        # the site-z gate of the reward
ASSET = {"cube": "airbot_cube.npz", "sf": "airbot_sf.npz", "tshape": "airbot_tshape.npz"}

COMMON = ("qpos", "qvel", "ctrl", "qacc_warmstart", "time", "xpos", "site_xpos", "done", "metrics", "info_steps", "info_truncation",
          "info_episode_done", "info_episode_metrics")
RECORD = {"cube": COMMON + ("info_target_pos", "info_new_cube_pos"),
          "sf": COMMON + ("info_target_pos", "info_new_cube_pos", "info_last_action"),
          "tshape": COMMON + ("info_target_base_pos", "info_target_vertical_pos", "info_new_T_pos")}
# every word a step may write or must leave alone, read back after it
READ = {k: tuple(dict.fromkeys(RECORD[k] + ("obs", "reward", "info_site_pos", R.BODY_POS[k]) + (("info_xita", "info_target_w") if k == "tshape" else ())))
        for k in KINDS}
FIRST = {"qpos": "first_qpos", "qvel": "first_qvel", "ctrl": "first_ctrl", "qacc_warmstart": "first_warmstart", "time": "first_time",
         "xpos": "first_xpos", "site_xpos": "first_site_xpos", "obs": "first_obs"}
# words no step writes: they must come back as they were
UNTOUCHED = {"cube": ("info_target_pos",), "sf": ("info_target_pos",), "tshape": ("info_target_base_pos", "info_target_vertical_pos", "info_target_w")}


def fields_fn(kind):
    from rsr_mjx_amd.envs import config
    return {"cube": config.cube_env_fields, "sf": config.sf_env_fields, "tshape": config.tshape_env_fields}[kind]


def variant_fields(model, kind, name, auto_reset=None):
    kw, length, auto = VARIANTS[name]
    return fields_fn(kind)(model, episode_length=length, auto_reset=auto if auto_reset is None else auto_reset, **kw)


def variant_constants(model, kind, name, auto_reset=None):
    return R.constants(kind, variant_fields(model, kind, name, auto_reset))


def before_of(rec, action):
    out = {k: np.asarray(v) for k, v in rec.items() if v is not None}
    out["action"] = np.asarray(action, f32)
    return out


def phys_of(kind, after):
    """what the reference takes from the record a step left: the published physics results (and, T-shape, the published geom
    differences and xita)"""
    p = dict(qpos=after["qpos"], xpos=after["xpos"], site_xpos=after["site_xpos"])
    if kind == "tshape":
        p.update(obs=after["obs"], xita=after["info_xita"])
    return p


# ---------------------------------------------------------------------------------------------------------------- census
def _aim(b, K):
    """float32 (dx, dy, dx + 1e-5f) of the wrist aim, from the record before the step"""
    n = len(b["ctrl"])
    ids = K["ids"]
    if K["kind"] == "tshape":
        sx = np.asarray(b["site_xpos"], f32).reshape(n, -1, 3)
        dx, dy = sx[:, ids[R.TID_TAIL], 0] - sx[:, ids[R.TID_SITE], 0], sx[:, ids[R.TID_TAIL], 1] - sx[:, ids[R.TID_SITE], 1]
    else:
        xp, tp = np.asarray(b["xpos"], f32).reshape(n, -1, 3), np.asarray(b["info_target_pos"], f32)
        dx, dy = tp[:, 0] - xp[:, ids[R.ID_CUBE], 0], tp[:, 1] - xp[:, ids[R.ID_CUBE], 1]
    return dx, dy, dx + f32(0.00001)


def _quadrant(y, x, k):
    return [(x > 0) & (y > 0), (x < 0) & (y > 0), (x < 0) & (y < 0), (x > 0) & (y < 0)][k]


def _q(r, g):
    return r["quant"][g][0]


def _sp(a):
    return np.asarray(a["info_site_pos"], f32)


def _col(d, k):
    return np.asarray(d[k]).reshape(len(d[k]), -1)[:, 0]


def _body_z(a, K):
    return np.asarray(a[R.BODY_POS[K["kind"]]], f32)[:, 2]


def _env_done(r):
    return r["done_env"] != 0


def _oob(a, K, which):
    sp, cz = _sp(a), np.asarray(a["info_cube_pos"], f32)[:, 2]
    v = [sp[:, 0] > 1, sp[:, 0] < f32(-0.6), sp[:, 1] > f32(0.3), sp[:, 1] < f32(-0.3), cz < f32(0.6)]
    alone = v[which] & ~np.any([v[i] for i in range(5) if i != which], 0)
    return alone & ~(sp[:, 2] < K["W"][3])                     # and the site is above endpoint_min_z: the bound alone flips health


def _if(cond, pred):
    pred.applies = cond
    return pred


_always = lambda K: True
_cs = lambda K: K["kind"] in ("cube", "sf")
_cube = lambda K: K["kind"] == "cube"
_sf = lambda K: K["kind"] == "sf"
_ts = lambda K: K["kind"] == "tshape"
_episode = lambda K: K["episode"]
_weights = lambda K: K["W"][0] > 100
_lane = lambda i, how: lambda b, a, K, r: {"low": r["ctrl"][:, i] == K["lo"][i], "high": r["ctrl"][:, i] == K["hi"][i],
                                            "inside": (r["ctrl"][:, i] > K["lo"][i]) & (r["ctrl"][:, i] < K["hi"][i])}[how]

CLASSES = {
    # ---- prologue ----
    **{f"ctrl{i}_{how}": _lane(i, how) for i in range(5) for how in ("low", "inside", "high")},
    "lanes34_ignore_action": lambda b, a, K, r: (np.abs(b["action"][:, 3]) > 0.5) & (np.abs(b["action"][:, 4]) > 0.5),
    **{f"aim_quadrant{k + 1}": (lambda k: lambda b, a, K, r: _quadrant(_aim(b, K)[1], _aim(b, K)[2], k))(k) for k in range(4)},
    "aim_epsilon_flips_sign": lambda b, a, K, r: (_aim(b, K)[0] < 0) & (_aim(b, K)[2] > 0),
    "aim_edge_dy0_dx_negative": lambda b, a, K, r: (_aim(b, K)[1] == 0) & (_aim(b, K)[2] < 0),
    "aim_edge_both_zero": lambda b, a, K, r: (_aim(b, K)[1] == 0) & (_aim(b, K)[2] == 0),
    "hold_taken": _if(_sf, lambda b, a, K, r: r["verdicts"]["hold"] & (_q(r, "hold") < 0.025)),
    "hold_near_inside": _if(_sf, lambda b, a, K, r: (_q(r, "hold") > 0.028) & (_q(r, "hold") < 0.03)),
    "hold_near_outside": _if(_sf, lambda b, a, K, r: (_q(r, "hold") > 0.03) & (_q(r, "hold") < 0.032)),
    "hold_not_taken": _if(_sf, lambda b, a, K, r: _q(r, "hold") > 0.05),
    "last_action_beyond_ctrl_range": _if(_sf, lambda b, a, K, r: np.abs(_col(a, "info_last_action")) > K["hi"][4]),
    # ---- cube / sf epilogue ----
    "btd_below": _if(_cs, lambda b, a, K, r: r["verdicts"]["btd_w4"]),
    "btd_above": _if(_cs, lambda b, a, K, r: _q(r, "btd_w4") > 0.006),
    "btd_just_above_005": _if(_cs, lambda b, a, K, r: (_q(r, "btd_w4") > 0.005) & (_q(r, "btd_w4") < 0.0075)),
    "btd_sf_band": _if(_sf, lambda b, a, K, r: (_q(r, "btd_w4") >= 0.0032) & (_q(r, "btd_w4") < 0.0048)),
    "site_z_below_082": _if(_cs, lambda b, a, K, r: _sp(a)[:, 2] < f32(0.82)),
    "site_z_above_082": _if(_cs, lambda b, a, K, r: ~(_sp(a)[:, 2] < f32(0.82))),
    "s2c_inside": lambda b, a, K, r: r["verdicts"]["s2c"],
    "s2c_just_outside": lambda b, a, K, r: ~r["verdicts"]["s2c"] & (_q(r, "s2c") < r["quant"]["s2c"][1] + 0.01),
    "s2c_far": lambda b, a, K, r: _q(r, "s2c") > 0.1,
    "health_site_below_min_z": lambda b, a, K, r: _sp(a)[:, 2] < K["W"][3],
    "health_site_above_min_z": lambda b, a, K, r: ~(_sp(a)[:, 2] < K["W"][3]),
    "site_z_just_below_gate": lambda b, a, K, r: (_sp(a)[:, 2] < f32(GATE_Z[K["kind"]])) & (_sp(a)[:, 2] > GATE_Z[K["kind"]] - 0.01),
    "site_z_just_above_gate": lambda b, a, K, r: ~(_sp(a)[:, 2] < f32(GATE_Z[K["kind"]])) & (_sp(a)[:, 2] < GATE_Z[K["kind"]] + 0.01),
    "min_z_just_below": lambda b, a, K, r: (_sp(a)[:, 2] < K["W"][3]) & (_sp(a)[:, 2] > K["W"][3] - 0.01),
    "min_z_just_above": lambda b, a, K, r: ~(_sp(a)[:, 2] < K["W"][3]) & (_sp(a)[:, 2] < K["W"][3] + 0.01),
    "body_z_just_below_06": lambda b, a, K, r: (_body_z(a, K) < f32(0.6)) & (_body_z(a, K) > 0.55),
    "body_z_just_above_06": lambda b, a, K, r: ~(_body_z(a, K) < f32(0.6)) & (_body_z(a, K) < 0.65),
    # (site x > 1.0 is beyond the arm's reach: that bound is exercised in the reference only, tests/test_airbot_epilogue.py)
    **{f"oob_{nm}_alone": _if(_sf, (lambda w: lambda b, a, K, r: _oob(a, K, w))(w)) for w, nm in ((1, "x_low"), (2, "y_high"), (3, "y_low"), (4, "cube_z"))},
    "done_cube_fell": _if(_cube, lambda b, a, K, r: np.asarray(a["info_cube_pos"], f32)[:, 2] < f32(0.6)),
    **{f"new_cube_pos_quadrant{k + 1}": _if(_cs, (lambda k: lambda b, a, K, r: r["new_pos_quadrant"] == k)(k)) for k in range(4)},
    # ---- T-shape epilogue ----
    "dis_base_snapped_only": _if(_ts, lambda b, a, K, r: r["verdicts"]["dis_base"] & ~r["verdicts"]["dis_vert"]),
    "dis_vert_snapped_only": _if(_ts, lambda b, a, K, r: ~r["verdicts"]["dis_base"] & r["verdicts"]["dis_vert"]),
    "dis_both_snapped": _if(_ts, lambda b, a, K, r: r["verdicts"]["dis_base"] & r["verdicts"]["dis_vert"]),
    "dis_none_snapped": _if(_ts, lambda b, a, K, r: ~r["verdicts"]["dis_base"] & ~r["verdicts"]["dis_vert"]),
    "dis_base_just_above_005": _if(_ts, lambda b, a, K, r: (_q(r, "dis_base") > 0.005) & (_q(r, "dis_base") < 0.0075)),
    "dis_vert_just_above_005": _if(_ts, lambda b, a, K, r: (_q(r, "dis_vert") > 0.005) & (_q(r, "dis_vert") < 0.0075)),
    "cosine_clamped_plus1": _if(_ts, lambda b, a, K, r: r["cosine"] > 1 - 1e-6),
    "cosine_clamped_minus1": _if(_ts, lambda b, a, K, r: r["cosine"] < -1 + 1e-6),
    "cosine_generic": _if(_ts, lambda b, a, K, r: np.abs(r["cosine"]) < 0.99),
    "site_z_below_083": _if(_ts, lambda b, a, K, r: _sp(a)[:, 2] < f32(0.83)),
    "site_z_above_083": _if(_ts, lambda b, a, K, r: ~(_sp(a)[:, 2] < f32(0.83))),
    "z_reward_just_below_0805": _if(_ts, lambda b, a, K, r: (_sp(a)[:, 2] < f32(0.805)) & (_sp(a)[:, 2] > 0.795)),
    "z_reward_just_above_0805": _if(_ts, lambda b, a, K, r: (_sp(a)[:, 2] > f32(0.805)) & (_sp(a)[:, 2] < 0.815)),
    "done_T_fell": _if(_ts, lambda b, a, K, r: np.asarray(a["info_T_pos"], f32)[:, 2] < f32(0.6)),
    **{f"new_T_pos_quadrant{k + 1}": _if(_ts, (lambda k: lambda b, a, K, r: r["new_pos_quadrant"] == k)(k)) for k in range(4)},
    # ---- total ----
    "reward_unclamped": _if(lambda K: not _weights(K), lambda b, a, K, r: np.abs(r["raw_total"]) < 100),
    "reward_clamped_high": _if(_weights, lambda b, a, K, r: r["raw_total"] > 100),
    "reward_clamped_low": _if(_weights, lambda b, a, K, r: r["raw_total"] < -100),
    # ---- wrappers ----
    "done_prev": lambda b, a, K, r: (_col(b, "done") != 0) & (_col(b, "info_steps") > 0),
    "prev_episode_done": _if(_episode, lambda b, a, K, r: _col(b, "info_episode_done") != 0),
    "nan_sum_prev_done": _if(_episode, lambda b, a, K, r: (_col(b, "info_episode_done") != 0) & np.isnan(b["info_episode_metrics"]).any(1)),
    "nan_sum_kept": _if(_episode, lambda b, a, K, r: (_col(b, "info_episode_done") == 0) & np.isnan(b["info_episode_metrics"]).any(1)),
    "last_step": _if(_episode, lambda b, a, K, r: (_col(b, "info_steps") == EPISODE_LENGTH - 1) & (_col(b, "done") == 0) & ~_env_done(r)),
    "last_step_done": _if(_episode, lambda b, a, K, r: (_col(b, "info_steps") == EPISODE_LENGTH - 1) & (_col(b, "done") == 0) & _env_done(r)),
}


def census(K, before, after, r32):
    """{class: number of states in it}; classes that do not apply to this kind and variant are left out."""
    with np.errstate(invalid="ignore"):
        return {name: int(np.count_nonzero(p(before, after, K, r32))) for name, p in CLASSES.items() if getattr(p, "applies", _always)(K)}


# ---------------------------------------------------------------------------------------------------------------- comparison
FACTOR = 4                  # x the recorded ref32-ref64 distance: the device's atan2f / sinf / cosf / tanhf / acosf differ from numpy's by a few ulp
ULPS = 2                    # + this many float32 ulp of the magnitude the quantity's roundings happen at (the stored value is a float32)
MAX_EXCLUDED = 0.02
# Float quantities that pass through libm (atan2f: the aim and what is held of it; sinf / cosf: the new push position; tanhf: siet;
# acosf: xita) or add such quantities up.  sqrtf and / are IEEE in this build (hipcc without fast-math keeps HIP's default of
# correctly rounded fp32 divide and sqrt), so btd, push and the dead-zone distances are not listed: everywhere else the env algebra is
# compiled with contraction off and the float32 reference restates it operation by operation, so it must be bit-identical.
NOT_BITWISE = ("ctrl/aim", "info_last_action", "new_pos", "obs/new_cube_pos", "obs/new_T_minus_site", "metrics/siet_to_box_reward",
               "metrics/siet2cube_reward", "xita", "reward", "episode/sum_reward", "episode/metrics")
XITA_CLASSES = ("aligned", "generic")


def xita_class(r64):
    """tolerance class of the angle: acosf next to +-1 is ill-conditioned (an ulp of the cosine is 3.5e-4 rad there)"""
    return np.where(np.abs(r64["cosine"]) > 1 - 1e-4, 0, 1)


def _tol_of(tol, nm, cls_names, cls, xcls):
    """per-state recorded distance of a quantity: its fixture class's, and for xita its angle class's on top"""
    t = np.array([tol[nm].get(c, 0.0) for c in cls_names])[cls]
    if nm == "xita":
        t = np.maximum(t, np.array([tol["xita@" + c] for c in XITA_CLASSES])[xcls])
    return t


def distances(K, r32, r64):
    """{quantity: |ref32 - ref64| per state (max over the quantity's components)}"""
    q32, q64 = R.float_quantities(r32, K), R.float_quantities(r64, K)
    out = {}
    for nm in q64:
        d = np.abs(np.asarray(q32[nm], np.float64) - q64[nm])
        d = np.where(np.isnan(q32[nm]) & np.isnan(q64[nm]), 0.0, d)
        out[nm] = d.reshape(len(d), -1).max(1)
    return out


def compare(K, tol, cls_names, cls, r64, got, live, excluded):
    """(failures, report): every float quantity of `got` within FACTOR x its class's recorded distance + ULPS ulp32 (+ xita's input
    allowance) of the float64 reference, every exact quantity equal.  `live`: envs whose record still holds obs and ctrl (not
    restored by AutoReset); `excluded`: states inside a threshold band, left to the step's verdict."""
    fails, report = [], {}
    rf, gf = R.float_quantities(r64, K), R.float_quantities(got, K)
    xcls = xita_class(r64) if K["kind"] == "tshape" else None
    for nm in rf:
        sel = (live if R.needs_phys(nm) else np.ones(len(live), bool)) & ~excluded
        a, b = np.asarray(gf[nm], np.float64), np.asarray(rf[nm], np.float64)
        sc = R.scale_of(nm, r64)
        mag = np.abs(b) if sc is None else np.maximum(np.abs(b), sc)
        t = _tol_of(tol, nm, cls_names, cls, xcls)
        bound = FACTOR * t.reshape((-1,) + (1,) * (b.ndim - 1)) + ULPS * np.spacing(np.nan_to_num(mag).astype(f32)).astype(np.float64)
        if nm == "xita":
            bound = bound + r64["xita_allowance"]
        d = np.where(np.isnan(a) & np.isnan(b), 0.0, np.abs(a - b))
        d = np.where(np.isnan(d), np.inf, d)
        ratio = np.where(d == 0, 0.0, d / bound)[sel]
        report[nm] = (float(d[sel].max()) if ratio.size else 0.0, float(ratio.max()) if ratio.size else 0.0)
        if ratio.size and not (ratio <= 1).all():
            w = np.flatnonzero(sel)[np.argmax(ratio.reshape(ratio.shape[0], -1).max(1))]
            fails.append(f"{nm}: |step - ref64| = {report[nm][0]:.3e} is {report[nm][1]:.2f} x its bound (state {int(w)}, class {cls_names[cls[w]]})")
    re_, ge = R.exact_quantities(r64, K), R.exact_quantities(got, K)
    for nm in re_:
        sel = (live if R.needs_phys(nm) else np.ones(len(live), bool)) & ~excluded
        x, y = np.asarray(re_[nm])[sel], np.asarray(ge[nm])[sel]
        ne = (x != y) & ~(np.isnan(x) & np.isnan(y))
        if ne.any():
            rows = np.flatnonzero(sel)[np.flatnonzero(ne.reshape(ne.shape[0], -1).any(1))]
            fails.append(f"{nm}: not equal in {len(rows)} states, first {rows[:5].tolist()}")
    return fails, report


def bitwise(K, r32, got, live, excluded):
    """{quantity: equal to the float32 reference bit for bit (over the states compared)}"""
    g32, gq = R.float_quantities(r32, K), R.float_quantities(got, K)
    out = {}
    for nm in g32:
        sel = (live if R.needs_phys(nm) else np.ones(len(live), bool)) & ~excluded
        x, y = np.asarray(g32[nm], f32)[sel], np.asarray(gq[nm], f32)[sel]
        out[nm] = bool(((x == y) | (np.isnan(x) & np.isnan(y))).all())
    return out


def excluded_states(K, r32):
    """states within BAND_ULPS ulp32 of a threshold in any gate (float32 quantities of the record at hand)"""
    b = R.bands(K, r32)
    out = np.zeros(len(r32["reward"]), bool)
    for v in b.values():
        out |= v
    return out
