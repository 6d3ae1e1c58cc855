"""Cost rollouts (rsr_physics_cost_rollouts, Physics.cost_rollouts) on every built family: the rollout is feedback_rollouts' or
param_rollouts' bit for bit; the cost, every step cost and every term sum are the weighted least-squares cost of the rows the same
call recorded, against fp64 numpy; the residuals are the tangent-space differences; on the reference everything is exactly zero;
a sample's numbers depend on nothing but its own inputs; rows go by slot; the refusals hold on the device; nothing but the
caller's buffers is written.  Batches, controls, gains and references are those of tests/test_feedback_gpu.py (N = 16, K = 3,
T = 3), built once per family and shared with that module."""
import ctypes as C
import functools

import numpy as np
import pytest

from physics_support import ALL, FAMILIES, assert_bitwise, assert_unchanged, handle_snapshot
from tangent_ref import differentiate_pos
from test_feedback_gpu import K, N, T, WITH_CTRL, _bare_handle, _base, _sampled

U = 2.0 ** -24
WEIGHTS = ("w_qpos", "w_qvel", "w_ctrl", "w_sensor")
EXTRA = dict(step_cost=True, terms=True, residual=True)


# ---- the shared inputs and the one call most tests read, computed once per family and left unchanged

@functools.lru_cache(maxsize=None)
def _cost(kind):
    """{name: [N, T, w]} on the device, rows by slot: weights uniform in (0.5, 2) per entry and per step; qpos_ref the record's
    qpos moved by N(0, 0.05) in the tangent space and qvel_ref the record's qvel + N(0, 0.1) (sample 0's rows of _base's
    references); ctrl_ref uniform inside the ctrl range; sensor_ref N(0, 0.1)."""
    import torch
    c = _base(kind)
    nq, nv, nu = c["dims"]
    nsd = c["pa"].nsensordata
    rng = np.random.default_rng(31)
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a.astype(np.float32)), device=c["A"].device)
    cost = dict(qpos_ref=c["qref"][:, 0].contiguous(), qvel_ref=c["vref"][:, 0].contiguous(),
                ctrl_ref=tt(c["lo"] + (c["hi"] - c["lo"]) * rng.uniform(size=(N, T, nu))), sensor_ref=tt(rng.normal(scale=0.1, size=(N, T, nsd))))
    for name, w in zip(WEIGHTS, (nv, nv, nu, nsd)):
        cost[name] = tt(rng.uniform(0.5, 2.0, size=(N, T, w)))
    return cost


def _feedback(c):
    return dict(gain=c["gain"], qpos_ref=c["qref"], qvel_ref=c["vref"])


@functools.lru_cache(maxsize=None)
def _costed(kind):
    """the closed-loop call with per-sample ctrl and gain rows, all four terms, every optional output and every field"""
    import torch
    c = _base(kind)
    c["A"].record.copy_(c["before"]["record"])
    out = c["pa"].cost_rollouts(c["ctrl"], _cost(kind), feedback=_feedback(c), fields=WITH_CTRL, **EXTRA)
    torch.cuda.synchronize()
    return out


def _f64(t):
    return t.cpu().numpy().astype(np.float64)


def _residuals64(c, cost, got):
    """(dq, dv, du, ds) [N, K, T, w] in fp64 from the fp32 rows `got` recorded and the fp32 references [N, T, w]"""
    nq, nv, nu = c["dims"]
    lead = got["qpos"].shape[:3]
    per = lambda name: np.broadcast_to(_f64(cost[name])[:, None], lead + (cost[name].shape[-1],))
    dq = differentiate_pos(c["arr"], nv, _f64(got["qpos"]).reshape(-1, nq), per("qpos_ref").reshape(-1, nq)).reshape(lead + (nv,))
    return dq, _f64(got["qvel"]) - per("qvel_ref"), _f64(got["ctrl"]) - per("ctrl_ref"), _f64(got["sensordata"]) - per("sensor_ref")


# ---- 1. the same rollout

@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_the_rollout_is_the_siblings_bit_for_bit(kind):
    """With sampled leaves, in closed loop (shared and per-sample gain rows, the clamp on) and open loop: all six fields and the
    applied ctrl are feedback_rollouts' / param_rollouts' on the same inputs.  Nothing but the caller's buffers is written, and a
    following env.step goes on as on a twin that never ran the call."""
    import torch
    c = _base(kind)
    A, twin, pa = c["A"], c["twin"], c["pa"]
    nq, nv, nu = c["dims"]
    A.record.copy_(c["before"]["record"])
    cost, params = _cost(kind), _sampled(c)
    given = {f: v.clone() for f, v in params.items()}
    kept = {f: v.clone() for f, v in cost.items()}
    own = {f: v.clone() for f, v in (A._dr or {}).items()}
    shared =[t[:, 0].contiguous() for t in (c["gain20"], c["qref"], c["vref"])]
    want = dict(closed=pa.feedback_rollouts(c["ctrl"], c["gain"], c["qref"], c["vref"], params=params, fields=WITH_CTRL),
                clamped=pa.feedback_rollouts(c["ctrl"], *shared, params=params, fields=WITH_CTRL, clamp=True),
                open=pa.param_rollouts(c["ctrl"], params, fields=ALL),
                logged=pa.param_rollouts(c["ctrl"][:, 0].contiguous(), params, fields=ALL))
    before = handle_snapshot(pa)
    got = dict(closed=pa.cost_rollouts(c["ctrl"], cost, feedback=_feedback(c), params=params, fields=WITH_CTRL, **EXTRA),
               clamped=pa.cost_rollouts(c["ctrl"], cost, feedback=dict(zip(("gain", "qpos_ref", "qvel_ref"), shared)), params=params,
                                        fields=WITH_CTRL, clamp=True),
               open=pa.cost_rollouts(c["ctrl"], cost, params=params, fields=WITH_CTRL, **EXTRA),
               logged=pa.cost_rollouts(c["ctrl"][:, 0].contiguous(), cost, params=params, fields=WITH_CTRL))
    after = handle_snapshot(pa)
    for name, res in got.items():
        for f in ALL:
            assert res[f].shape[:3] == (N, K, T) and torch.isfinite(res[f]).all(), (name, f)
            assert_bitwise(f"{kind} {name} {f}", res[f], want[name][f])
        assert torch.isfinite(res["cost"]).all() and res["cost"].shape == (N, K)
    for name in ("closed", "clamped"):
        assert_bitwise(f"{kind} {name} applied ctrl", got[name]["ctrl"], want[name]["ctrl"])
    assert_bitwise(f"{kind} open-loop applied ctrl", got["open"]["ctrl"], c["ctrl"])
    assert_bitwise(f"{kind} logged applied ctrl", got["logged"]["ctrl"], c["ctrl"][:, :1].expand(-1, K, -1, -1))
    assert bool((got["clamped"]["ctrl"] != got["closed"]["ctrl"]).any()) and (got["closed"]["ncon"] > 0).any()
    assert_unchanged(before, after)                                       # the whole record and every buffer of the handle
    assert_unchanged(c["before"], after)
    for f, v in given.items():
        assert_bitwise(f"{kind} the caller's {f}", params[f], v)
    for f, v in own.items():
        assert_bitwise(f"{kind} the batch's {f}", A._dr[f], v)
    for name, v in kept.items():
        assert_bitwise(f"{kind} the caller's {name}", cost[name], v)
    act =np.clip(np.random.default_rng(11).normal(size=(N, nu)) * c["scale"], -1, 1).astype(np.float32)
    A.step(None, act)
    twin.step(None, act)
    torch.cuda.synchronize()
    assert_bitwise(f"{kind} env.step after cost_rollouts", A.record, twin.record)
    A.record.copy_(c["before"]["record"]); twin.record.copy_(c["before"]["record"])
    torch.cuda.synchronize()


# ---- 2. the cost

@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_the_cost_against_fp64(kind):
    """J64 = sum_t 1/2 sum_i w_i d_i^2 in numpy fp64, from the fp32 rows this same call recorded (qpos, qvel, sensordata and the
    applied ctrl) and the fp32 references and weights, dq by tangent_ref.differentiate_pos.  With U = 2^-24, n = 2 nv + nu + nsd and
    delta_i = 1e-6 |dq_i| + 16 U (the bound tests/test_transition_gpu.py and tests/test_feedback_gpu.py hold differentiate_pos to):
        |cost - J64| <= (n + T + 8) U J64 + sum_t sum_i w_qpos,i (|dq_i| delta_i + delta_i^2 / 2).
    Where it comes from: an entry w d d carries at most 4 roundings (the difference, two products, and the halving is exact); a
    step adds at most n summands, every one >= 0, so each meets at most n additions (here 3 in its lane and 6 in wave_sum: 9 < n);
    the running cost adds T steps.  (1 + U)^(4 + n + T) - 1 stays below (n + T + 8) U at these sizes.  The second sum is what an
    error delta_i in dq_i moves 1/2 w (dq_i + e)^2 by.  The same bound without T holds every step cost, and with a term's own
    count in place of n (nv, nv, nu, nsd) every term sum.  terms.sum(-1) agrees with cost within 4 U cost and step_cost.sum(-1)
    within T U cost (sums of the fp32 numbers in fp64).  No env, sample or step is left out."""
    c, got, cost = _base(kind), _costed(kind), _cost(kind)
    nq, nv, nu = c["dims"]
    nsd = c["pa"].nsensordata
    n = 2 * nv + nu + nsd
    d = _residuals64(c, cost, got)
    w = [_f64(cost[name])[:, None] for name in WEIGHTS]
    per_step = [0.5 * (wk * dk * dk).sum(-1) for wk, dk in zip(w, d)]               # [N, K, T] each
    dq = np.abs(d[0])
    delta = 1e-6 * dq + 16 * U
    slack = (w[0] * (dq * delta + 0.5 * delta * delta)).sum(-1)                     # [N, K, T]
    step64 = sum(per_step)
    J64 = step64.sum(-1)
    term64 = np.stack([p.sum(-1) for p in per_step], -1)                            # [N, K, 4]
    cost32, step32, term32 = _f64(got["cost"]), _f64(got["step_cost"]), _f64(got["terms"])
    assert all(np.isfinite(a).all() for a in (cost32, step32, term32, J64, step64, term64))
    assert (term64 > 0).all() and (term32 > 0).all(), "every term sum is positive in every sample"
    assert (_f64(got["ncon"]) > 0).any()
    count = np.array([nv, nv, nu, nsd])
    term_slack = np.zeros_like(term64)
    term_slack[..., 0] = slack.sum(-1)
    checks = [("cost", cost32, J64, (n + T + 8) * U * J64 + slack.sum(-1)),
              ("step_cost", step32, step64, (n + 8) * U * step64 + slack),
              ("terms", term32, term64, (count + T + 8) * U * term64 + term_slack),
              ("terms.sum(-1) against cost", term32.sum(-1), cost32, 4 * U * cost32),
              ("step_cost.sum(-1) against cost", step32.sum(-1), cost32, T * U * cost32)]
    bad = []
    for name, a, b, bound in checks:
        err = np.abs(a - b)
        print(kind, name, "max err / bound %.3f" % float((err / bound).max()), "max rel err / U %.2f" % float((err / np.abs(b)).max() / U))
        if not (err <= bound).all():
            bad.append(f"{kind} {name}: {(err > bound).sum()} of {err.size} beyond the bound, worst ratio {(err / bound).max():.3f}")
    assert not bad, bad


# ---- 3. the residuals

@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_the_residuals(kind):
    """dx[..., nv:] is the one fp32 subtraction qvel - qvel_ref, bit for bit; dx[..., :nv] is the fp64 tangent difference within
    delta_i = 1e-6 |dq_i| + 16 * 2^-24."""
    c, got, cost = _base(kind), _costed(kind), _cost(kind)
    nq, nv, nu = c["dims"]
    dx = got["dx"].cpu().numpy()
    assert dx.shape == (N, K, T, 2 * nv) and dx.dtype == np.float32
    want = got["qvel"].cpu().numpy() - cost["qvel_ref"].cpu().numpy()[:, None]
    assert want.dtype == np.float32 and (dx[..., nv:].view(np.int32) == want.view(np.int32)).all()
    dq64 = _residuals64(c, cost, got)[0]
    err, bound = np.abs(dx[..., :nv].astype(np.float64) - dq64), 1e-6 * np.abs(dq64) + 16 * U
    print(kind, "dq max err / bound %.3f" % float((err / bound).max()))
    assert (err <= bound).all(), f"{kind}: {(err > bound).sum()} of {err.size} entries beyond the bound"
    assert (np.abs(dq64) > 0).all()


# ---- 4. exactly zero on the reference

@pytest.mark.gpu
@pytest.mark.parametrize("kind, steps", [("go2rough", T), ("cube", T), ("cube", 1)])
def test_exactly_zero_on_the_reference(kind, steps):
    """K = 1: the references are the rows a first call recorded (qpos, qvel, sensordata, the applied ctrl); the same call again
    then has every residual exactly zero, the free joint's rotation included, and so every cost.  steps = 1: K = T = 1."""
    import torch
    c = _base(kind)
    pa = c["pa"]
    c["A"].record.copy_(c["before"]["record"])
    one = lambda t: t[:, :1, :steps].contiguous()
    ctrl, fb = one(c["ctrl"]), {k: one(v) for k, v in _feedback(c).items()}
    cost = {k: v[:, :steps].contiguous() for k, v in _cost(kind).items()}
    first = pa.cost_rollouts(ctrl, cost, feedback=fb, fields=("qpos", "qvel", "sensordata", "ctrl"), **EXTRA)
    assert (first["terms"] > 0).all()
    on = dict(cost, qpos_ref=first["qpos"][:, 0].contiguous(), qvel_ref=first["qvel"][:, 0].contiguous(), ctrl_ref=first["ctrl"][:, 0].contiguous(),
              sensor_ref=first["sensordata"][:, 0].contiguous())
    second = pa.cost_rollouts(ctrl, on, feedback=fb, fields=("qpos", "qvel", "sensordata", "ctrl"), **EXTRA)
    torch.cuda.synchronize()
    for f in ("qpos", "qvel", "sensordata", "ctrl"):
        assert_bitwise(f"{kind} {f}", second[f], first[f])
    for f, shape in (("cost", (N, 1)), ("step_cost", (N, 1, steps)), ("terms", (N, 1, 4)), ("dx", (N, 1, steps, 2 * c["dims"][1]))):
        assert second[f].shape == shape and bool((second[f] == 0.0).all()), (kind, f, float(second[f].abs().max()))


# ---- 5. determinism and rows

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2rough"])
def test_a_sample_depends_on_its_own_inputs_alone(kind):
    import torch
    from rsr_mjx_amd import _lib
    c, full, cost = _base(kind), _costed(kind), _cost(kind)
    A, pa = c["A"], c["pa"]
    nq, nv, nu = c["dims"]
    A.record.copy_(c["before"]["record"])
    fb = _feedback(c)
    # with and without every optional output and every trajectory; and the run
    bare = pa.cost_rollouts(c["ctrl"], cost, feedback=fb)
    assert list(bare) == ["cost"]
    assert_bitwise(f"{kind} cost alone", bare["cost"], full["cost"])
    for kw, names in ((dict(step_cost=True), ("step_cost",)), (dict(terms=True), ("terms",)), (dict(residual=True), ("dx",)),
                      (dict(fields=("ctrl",)), ("ctrl",)), (dict(fields=("sensordata", "qpos"), terms=True), ("terms", "sensordata", "qpos"))):
        res = pa.cost_rollouts(c["ctrl"], cost, feedback=fb, **kw)
        assert list(res) == ["cost", *names]
        for f in res:
            assert_bitwise(f"{kind} {f} with {sorted(kw)}", res[f], full[f])
    # one term at a time: the others' references are not needed, and the term is the full call's
    for k, (wname, ref) in enumerate(zip(WEIGHTS, ("qpos_ref", "qvel_ref", "ctrl_ref", "sensor_ref"))):
        res = pa.cost_rollouts(c["ctrl"], {wname: cost[wname], ref: cost[ref]}, feedback=fb, terms=True)
        assert_bitwise(f"{kind} {wname} alone", res["terms"][..., k], full["terms"][..., k])
        assert bool((res["terms"][..., [j for j in range(4) if j != k]] == 0).all())
    # weights and references shared by a slot's K samples, different ctrl samples: different costs
    assert all(bool((full["cost"][:, j] != full["cost"][:, 0]).all()) for j in range(1, K))
    # rows by slot: a repeated env, another order, K = 1 of one sample
    ids = [3, 3, 0]
    sub = lambda t: t[ids].contiguous()
    res = pa.cost_rollouts(sub(c["ctrl"]), {k: sub(v) for k, v in cost.items()}, feedback={k: sub(v) for k, v in fb.items()}, env_ids=ids,
                           fields=WITH_CTRL, **EXTRA)
    for f in res:
        for s, e in enumerate(ids):
            assert_bitwise(f"{kind} slot {s} (env {e}) {f}", res[f][s], full[f][e])
    one = pa.cost_rollouts(c["ctrl"][:, 2:3].contiguous(), cost, feedback={k: v[:, 2:3].contiguous() for k, v in fb.items()}, fields=WITH_CTRL, **EXTRA)
    for f in one:
        assert_bitwise(f"{kind} K = 1 of sample 2 {f}", one[f][:, 0], full[f][:, 2])
    # the raw call: an id of num_envs runs nothing and leaves its slot's rows alone, in every output
    names = list(full)
    buf = {f: torch.full((4,) + tuple(full[f].shape[1:]), -7.25, device=A.device) for f in names}
    raw = torch.tensor([11, N, 7], dtype=torch.int32, device=A.device)
    rows = [11, 3, 7]
    held = [t[rows].contiguous() for t in (c["ctrl"], *fb.values())] + [cost[k][rows].contiguous() for k in _lib.COST_REFS + _lib.COST_WEIGHTS]
    o, co = _lib.RolloutOut(), _lib.CostOut()
    for f in ALL:
        setattr(o, f, buf[f].data_ptr())
    for f, member in (("cost", "cost"), ("step_cost", "step_cost"), ("terms", "terms"), ("dx", "dx"), ("ctrl", "ctrl")):
        setattr(co, member, buf[f].data_ptr())
    fbs, cs = _lib.Feedback(*[t.data_ptr() for t in held[1:4]]), _lib.Cost(*[t.data_ptr() for t in held[4:]])
    rc = _lib.lib().rsr_physics_cost_rollouts(pa._h, C.c_void_p(raw.data_ptr()), 3, C.c_void_p(held[0].data_ptr()), C.byref(fbs), None, C.byref(cs),
                                              K, T, pa.n_substeps, _lib.FB_CTRL_PER_SAMPLE | _lib.FB_PER_SAMPLE, C.byref(o), C.byref(co), pa._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rsr_last_error()
    for f in names:
        assert_bitwise(f"{kind} raw slot 0 {f}", buf[f][0], full[f][11])
        assert_bitwise(f"{kind} raw slot 2 {f}", buf[f][2], full[f][7])
        assert (buf[f][1] == -7.25).all() and (buf[f][3] == -7.25).all(), f
    assert_bitwise(f"{kind} record", A.record, c["before"]["record"])


# ---- 6. refusals

@pytest.mark.gpu
def test_refusals_on_the_device():
    import torch
    from rsr_mjx_amd import _lib
    c, cost = _base("cube"), _cost("cube")
    A, pa = c["A"], c["pa"]
    nq, nv, nu = c["dims"]
    A.record.copy_(c["before"]["record"])
    L = _lib.lib()
    fn = L.rsr_physics_cost_rollouts
    ctrl = C.c_void_p(c["ctrl"].data_ptr())
    sent = lambda *shape: torch.full(shape, -7.25, device=A.device)
    qpos, sd = sent(N, K, T, nq), sent(N, K, T, 64)
    outs = dict(cost=sent(N, K), step_cost=sent(N, K, T), terms=sent(N, K, 4), dx=sent(N, K, T, 2 * nv), ctrl=sent(N, K, T, nu))
    ids = torch.arange(2, dtype=torch.int32, device=A.device)
    o, o_sd = _lib.RolloutOut(), _lib.RolloutOut()
    o.qpos = qpos.data_ptr()
    o_sd.sensordata = sd.data_ptr()
    fb = _lib.Feedback(c["gain"].data_ptr(), c["qref"].data_ptr(), c["vref"].data_ptr())
    mass, ipos = torch.ones((N, K, A.dims.nbody), device=A.device), torch.zeros((N, K, A.dims.nbody, 3), device=A.device)
    ok, go2_only = _lib.ParamSamples(), _lib.ParamSamples()
    ok.leaf[_lib.DR_FIELDS.index("body_mass")] = mass.data_ptr()
    go2_only.leaf[_lib.DR_FIELDS.index("body_ipos")] = ipos.data_ptr()

    def cost_of(**kw):                           # the full cost with some members replaced (None: NULL)
        s = _lib.Cost(**{k: v.data_ptr() for k, v in cost.items()})
        for k, v in kw.items():
            setattr(s, k, v)
        return C.byref(s)

    def out_of(**kw):
        s = _lib.CostOut(**{k: v.data_ptr() for k, v in outs.items()})
        for k, v in kw.items():
            setattr(s, k, v)
        return C.byref(s)

    def partial(**kw):                           # an fb with one member NULL
        f = _lib.Feedback(c["gain"].data_ptr(), c["qref"].data_ptr(), c["vref"].data_ptr())
        for k, v in kw.items():
            setattr(f, k, v)
        return C.byref(f)

    nf, both = pa.n_substeps, _lib.FB_CTRL_PER_SAMPLE | _lib.FB_PER_SAMPLE
    h, fbp, ps, cs, tr, co = pa._h, C.byref(fb), C.byref(ok), cost_of(), C.byref(o), out_of()
    no_sensor = cost_of(w_sensor=None, sensor_ref=None)
    bare = _bare_handle(c)
    torch.cuda.synchronize()
    before = handle_snapshot(pa)
    E_ARG, E_UNSUPPORTED = -1, -2
    big = 2 ** 31 - 1
    calls = [("null ctrl", (h, None, 0, None, fbp, ps, cs, K, T, nf, both, tr, co), E_ARG),
             ("null gain", (h, None, 0, ctrl, partial(gain=None), ps, cs, K, T, nf, both, tr, co), E_ARG),
             ("null qpos_ref of fb", (h, None, 0, ctrl, partial(qpos_ref=None), ps, cs, K, T, nf, both, tr, co), E_ARG),
             ("null qvel_ref of fb", (h, None, 0, ctrl, partial(qvel_ref=None), ps, cs, K, T, nf, both, tr, co), E_ARG),
             ("RSR_FB_PER_SAMPLE with a null fb", (h, None, 0, ctrl, None, ps, cs, K, T, nf, both, tr, co), E_ARG),
             ("RSR_FB_CLAMP with a null fb", (h, None, 0, ctrl, None, ps, cs, K, T, nf, _lib.FB_CTRL_PER_SAMPLE | _lib.FB_CLAMP, tr, co), E_ARG),
             ("null cost", (h, None, 0, ctrl, fbp, ps, None, K, T, nf, both, tr, co), E_ARG),
             ("null out", (h, None, 0, ctrl, fbp, ps, cs, K, T, nf, both, tr, None), E_ARG),
             ("null out->cost", (h, None, 0, ctrl, fbp, ps, cs, K, T, nf, both, tr, out_of(cost=None)), E_ARG),
             ("all four weights null", (h, None, 0, ctrl, fbp, ps, cost_of(w_qpos=None, w_qvel=None, w_ctrl=None, w_sensor=None), K, T, nf, both, tr, co), E_ARG),
             ("w_qpos without qpos_ref", (h, None, 0, ctrl, fbp, ps, cost_of(qpos_ref=None), K, T, nf, both, tr, co), E_ARG),
             ("dx without qpos_ref", (h, None, 0, ctrl, fbp, ps, cost_of(qpos_ref=None, w_qpos=None), K, T, nf, both, tr, co), E_ARG),
             ("K = 0", (h, None, 0, ctrl, fbp, ps, cs, 0, T, nf, both, tr, co), E_ARG),
             ("T = 0", (h, None, 0, ctrl, fbp, ps, cs, K, 0, nf, both, tr, co), E_ARG),
             ("nsteps = 0", (h, None, 0, ctrl, fbp, ps, cs, K, T, 0, both, tr, co), E_ARG),
             ("flag bit 3", (h, None, 0, ctrl, fbp, ps, cs, K, T, nf, both | 8, tr, co), E_ARG),
             ("negative flags", (h, None, 0, ctrl, fbp, ps, cs, K, T, nf, -1, tr, co), E_ARG),
             ("env_ids with count 0", (h, C.c_void_p(ids.data_ptr()), 0, ctrl, fbp, ps, cs, K, T, nf, both, tr, co), E_ARG),
             ("M K at 2^31", (h, None, 0, ctrl, fbp, ps, cs, big, T, nf, both, tr, co), E_ARG),
             ("T nsteps at 2^31", (h, None, 0, ctrl, fbp, ps, cs, K, big, 2, both, tr, co), E_ARG),
             ("w_sensor with no table", (bare._h, None, 0, ctrl, fbp, ps, cost_of(sensor_ref=None), K, T, nf, both, tr, co), E_ARG),
             ("sensor_ref with no table", (bare._h, None, 0, ctrl, fbp, ps, cost_of(w_sensor=None), K, T, nf, both, tr, co), E_ARG),
             ("sensordata rows with no table", (bare._h, None, 0, ctrl, fbp, ps, no_sensor, K, T, nf, both, C.byref(o_sd), co), E_ARG),
             ("a Go2-only leaf", (h, None, 0, ctrl, fbp, C.byref(go2_only), cs, K, T, nf, both, tr, co), E_UNSUPPORTED)]
    for what, args, code in calls:
        assert fn(*args, pa._stream()) == code, what
        assert b"rsr_physics_cost_rollouts" in L.rsr_last_error(), what
    torch.cuda.synchronize()
    assert_unchanged(before, handle_snapshot(pa))
    assert (qpos == -7.25).all() and (sd == -7.25).all() and all(bool((t == -7.25).all()) for t in outs.values())
    # what is not refused: a null fb without its flags, a null traj, null params; the cost is the Python call's
    assert fn(h, None, 0, ctrl, None, None, cs, K, T, nf, _lib.FB_CTRL_PER_SAMPLE, None, out_of(step_cost=None, terms=None, dx=None, ctrl=None),
              pa._stream()) == 0, L.rsr_last_error()
    torch.cuda.synchronize()
    assert_bitwise("cube open loop, cost alone", outs["cost"], pa.cost_rollouts(c["ctrl"], cost)["cost"])
    assert (qpos == -7.25).all() and all(bool((outs[f] == -7.25).all()) for f in ("step_cost", "terms", "dx", "ctrl"))
    # ... and on a handle with no sensor table, the three terms that need none
    assert fn(bare._h, None, 0, ctrl, fbp, None, no_sensor, K, T, nf, both, None, out_of(step_cost=None, dx=None, ctrl=None), pa._stream()) == 0, L.rsr_last_error()
    torch.cuda.synchronize()
    assert_bitwise("cube no sensor table", outs["terms"][..., :3], _costed("cube")["terms"][..., :3])
    assert bool((outs["terms"][..., 3] == 0).all())
    assert_unchanged(before, handle_snapshot(pa))
