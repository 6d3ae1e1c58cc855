"""Closed-loop rollouts (rsr_physics_feedback_rollouts, Physics.feedback_rollouts) on every built family: with zero gains the call
is param_rollouts bit for bit; the controls it reports reproduce its trajectories through sample_rollouts bit for bit; every
control it applied is the affine law on the recorded state, against fp64 numpy, with and without the clamp; rows go by slot and by
sample; the refusals hold on the device; nothing but the caller's buffers is written.
The one tolerance (test_the_law_against_fp64) is the fma chain's standard bound plus the bound tests/test_transition_gpu.py holds
differentiate_pos to."""
import ctypes as C
import functools

import numpy as np
import pytest

from physics_support import ALL, FAMILIES, assert_bitwise, assert_unchanged, handle_snapshot, pair, sensor_spec
from tangent_ref import differentiate_pos, moved

N, K, T = 16, 3, 3
U = 2.0 ** -24
WITH_CTRL = ALL + ("ctrl",)
BASE_LEAVES = ("geom_friction", "body_mass", "dof_damping", "dof_frictionloss")
GO2_LEAVES = ("body_ipos", "qpos0", "dof_armature", "actuator_gainprm", "actuator_biasprm")
GO2 = ("go2flat", "go2rough", "footstand")


# ---- the shared inputs, computed once per family and left unchanged

@functools.lru_cache(maxsize=None)
def _base(kind):
    """Batch A (reset, 3 random env steps: cube on the table, feet on the ground) with its handle and its untouched twin; per
    (env, sample, step): a nominal ctrl uniform inside the ctrl range (no entry is +-0), qpos_ref = the record's qpos moved in the
    tangent space by N(0, 0.05) per dof, qvel_ref = the record's qvel + N(0, 0.1), and gains N(0, 1) g_j with g_j such that the
    median |sum_i gain_ji dx_i| of actuator j is a tenth of its ctrl range.  g is fixed ahead of every closed-loop call: dx is taken
    in fp64 along the open-loop trajectory of the nominal ctrl (sample_rollouts, an existing call)."""
    import torch
    from rsr_mjx_amd.physics import Physics
    envdef, A, twin, scale, rng = pair(kind, N)
    pa = Physics(A, sensors=sensor_spec(kind, envdef))
    arr, d = envdef.sys.arrays, A.dims
    nq, nv, nu = int(d.nq), int(d.nv), int(d.nu)
    dev = A.device
    lo, hi = arr["actuator_ctrlrange"][:, 0].astype(np.float64), arr["actuator_ctrlrange"][:, 1].astype(np.float64)
    limited = np.asarray(arr["actuator_ctrllimited"]).astype(bool)
    assert limited.all(), kind                   # every actuator of the shipped Airbot and Go2 models is ctrl-limited: the clamp acts on all
    ctrl = (lo + (hi - lo) * rng.uniform(size=(N, K, T, nu))).astype(np.float32)
    assert (ctrl != 0).all()
    torch.cuda.synchronize()
    q0, v0 = pa.qpos.cpu().numpy().copy(), pa.qvel.cpu().numpy().copy()
    rep = lambda a: np.repeat(a[:, None], K * T, 1).reshape(N * K * T, -1)
    qref = moved(arr, nv, rep(q0), rng.normal(scale=0.05, size=(N * K * T, nv))).astype(np.float32).reshape(N, K, T, nq)
    vref = (rep(v0) + rng.normal(scale=0.1, size=(N * K * T, nv))).astype(np.float32).reshape(N, K, T, nv)
    t_ctrl = torch.as_tensor(ctrl, device=dev)
    before = handle_snapshot(pa)
    open_loop = pa.sample_rollouts(t_ctrl, fields=("qpos", "qvel"))
    torch.cuda.synchronize()
    dx = _dx(arr, nv, q0, v0, open_loop["qpos"].cpu().numpy(), open_loop["qvel"].cpu().numpy(), qref, vref)
    raw = rng.normal(size=(N, K, T, nu, 2 * nv))
    med = np.median(np.abs(np.einsum("nktji,nkti->nktj", raw, dx)).reshape(-1, nu), 0)
    g = 0.1 * (hi - lo) / med
    gain = (raw * g[:, None]).astype(np.float32)
    print(kind, "gain scale per actuator", g)
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return dict(kind=kind, envdef=envdef, A=A, twin=twin, pa=pa, scale=scale, arr=arr, dims=(nq, nv, nu), lo=lo, hi=hi, q0=q0, v0=v0,
                ctrl=t_ctrl, gain=tt(gain), gain20=tt((20.0 * raw * g[:, None]).astype(np.float32)), qref=tt(qref), vref=tt(vref),
                before=before)


def _dx(arr, nv, q0, v0, qpos, qvel, qref, vref):
    """[N, K, T, 2 nv] in fp64: (qpos (-) qpos_ref, qvel - qvel_ref) at the start of every control step, from the record
    (q0, v0 [N, .]) for t = 0 and the recorded row t - 1 otherwise"""
    nq = q0.shape[1]
    qs = np.concatenate([np.repeat(q0[:, None, None], K, 1), qpos[:, :, :T - 1]], 2).astype(np.float64)
    vs = np.concatenate([np.repeat(v0[:, None, None], K, 1), qvel[:, :, :T - 1]], 2).astype(np.float64)
    dq = differentiate_pos(arr, nv, qs.reshape(-1, nq), qref.reshape(-1, nq)).reshape(N, K, T, nv)
    return np.concatenate([dq, vs - vref.astype(np.float64)], 3)


def _own_leaves(c):
    """each env's own leaves [N, ...]: its per-env values, or the model's"""
    names = BASE_LEAVES + (GO2_LEAVES if c["kind"] in GO2 else ())
    dr, arr = c["A"]._dr or {}, c["arr"]
    return {f: dr[f].cpu().numpy().astype(np.float32).reshape((N,) + arr[f].shape) if f in dr else
            np.tile(arr[f].astype(np.float32)[None], (N,) + (1,) * arr[f].ndim) for f in names}


def _sampled(c, seed=21):
    """{leaf: [N, K, ...]}: every leaf the family takes, within 5 % of the env's own (qpos0: the joints only)"""
    import torch
    rng = np.random.default_rng(seed)
    out = {}
    for f, own in _own_leaves(c).items():
        v = np.repeat(own[:, None], K, 1).astype(np.float64)
        if f == "qpos0":
            v[..., 7:] *= rng.uniform(0.95, 1.05, size=v[..., 7:].shape)
        else:
            v *= rng.uniform(0.95, 1.05, size=v.shape)
        out[f] = torch.as_tensor(v.astype(np.float32), device=c["A"].device).contiguous()
    return out


# ---- 1. zero gain is the open loop

@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_zero_gain_is_param_rollouts_bit_for_bit(kind):
    """gain = 0, refs arbitrary and finite: every fma(0, dx, u) is u, so all six fields are param_rollouts' on the same ctrl and
    leaves, and the applied ctrl is the nominal one.  Nothing but the caller's buffers is written."""
    import torch
    c = _base(kind)
    A, twin, pa = c["A"], c["twin"], c["pa"]
    nq, nv, nu = c["dims"]
    params = _sampled(c)
    given = {f: v.clone() for f, v in params.items()}
    own = {f: v.clone() for f, v in (A._dr or {}).items()}
    want = pa.param_rollouts(c["ctrl"], params, fields=ALL)
    zero = torch.zeros((N, T, nu, 2 * nv), device=A.device)
    before = handle_snapshot(pa)
    got = pa.feedback_rollouts(c["ctrl"], zero, c["qref"][:, 0].contiguous(), c["vref"][:, 0].contiguous(), params=params, fields=WITH_CTRL)
    each = pa.feedback_rollouts(c["ctrl"], torch.zeros((N, K, T, nu, 2 * nv), device=A.device), c["qref"], c["vref"], params=params,
                                fields=WITH_CTRL, clamp=True)              # (inside the range the clamp changes nothing)
    after = handle_snapshot(pa)
    for name, res in (("shared rows", got), ("per-sample rows, clamp", each)):
        for f in ALL:
            assert res[f].shape[:3] == (N, K, T) and torch.isfinite(res[f]).all(), f
            assert_bitwise(f"{kind} {name} {f}", res[f], want[f])
        assert_bitwise(f"{kind} {name} applied ctrl", res["ctrl"], c["ctrl"])
    assert (got["ncon"] > 0).any()
    assert_unchanged(before, after)                                       # the whole record and every buffer of the handle
    assert_unchanged(c["before"], after)
    for f, v in given.items():
        assert_bitwise(f"{kind} the caller's {f}", params[f], v)
    for f, v in own.items():
        assert_bitwise(f"{kind} the batch's {f}", A._dr[f], v)
    # env.step goes on as on a twin that never ran a closed-loop rollout
    act = np.clip(np.random.default_rng(11).normal(size=(N, nu)) * c["scale"], -1, 1).astype(np.float32)
    A.step(None, act)
    twin.step(None, act)
    torch.cuda.synchronize()
    assert_bitwise(f"{kind} env.step after feedback_rollouts", A.record, twin.record)
    A.record.copy_(c["before"]["record"]); twin.record.copy_(c["before"]["record"])
    torch.cuda.synchronize()


# ---- 2. the applied controls reproduce the trajectories

@functools.lru_cache(maxsize=None)
def _closed(kind, clamp=False):
    """the closed-loop call with per-sample ctrl, gains (x 20 with the clamp) and refs, no params: every field and the applied ctrl"""
    import torch
    c = _base(kind)
    c["A"].record.copy_(c["before"]["record"])
    out = c["pa"].feedback_rollouts(c["ctrl"], c["gain20"] if clamp else c["gain"], c["qref"], c["vref"], fields=WITH_CTRL, clamp=clamp)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2rough", "footstand"])
def test_the_applied_controls_reproduce_the_trajectories(kind):
    import torch
    c, got = _base(kind), _closed(kind)
    replay = c["pa"].sample_rollouts(got["ctrl"], fields=ALL)
    torch.cuda.synchronize()
    for f in ALL:
        assert torch.isfinite(got[f]).all(), f
        assert_bitwise(f"{kind} replay {f}", got[f], replay[f])
    assert bool((got["ctrl"] != c["ctrl"]).flatten(2).any(2).all())       # the feedback was felt in every sample
    assert (got["ncon"] > 0).any()
    assert_bitwise(f"{kind} record", c["A"].record, c["before"]["record"])


# ---- 3. the law

@pytest.mark.gpu
@pytest.mark.parametrize("clamp", [False, True], ids=["free", "clamp"])
@pytest.mark.parametrize("kind", FAMILIES)
def test_the_law_against_fp64(kind, clamp):
    """Every applied control, from the recorded fp32 states (the record for t = 0, row t - 1 otherwise) in fp64:
    u64_j = ctrl_j + sum_i g_ji dx_i, clamped in fp64 with the clamp on.  Per entry
        |u - u64| <= (2 nv + 2) 2^-24 (|ctrl_j| + sum_i |g_ji| |dx_i|) + sum_i |g_ji| (1e-6 |dx_i| + 16 * 2^-24):
    the fma chain's standard bound, and the bound tests/test_transition_gpu.py holds differentiate_pos to.  No env, sample, step or
    entry is left out.  With the clamp the gains are 20 times larger, so that both of its branches run: every actuator of the
    shipped models is ctrl-limited (_base asserts it), and more than 5 % and fewer than 95 % of the entries sit on a limit."""
    c, got = _base(kind), _closed(kind, clamp)
    nq, nv, nu = c["dims"]
    u = got["ctrl"].cpu().numpy().astype(np.float64)
    dx = _dx(c["arr"], nv, c["q0"], c["v0"], got["qpos"].cpu().numpy(), got["qvel"].cpu().numpy(), c["qref"].cpu().numpy(), c["vref"].cpu().numpy())
    g = (c["gain20"] if clamp else c["gain"]).cpu().numpy().astype(np.float64)
    nominal = c["ctrl"].cpu().numpy().astype(np.float64)
    fb = np.einsum("nktji,nkti->nktj", g, dx)
    mag = np.einsum("nktji,nkti->nktj", np.abs(g), np.abs(dx))
    u64 = nominal + fb
    if clamp:
        u64 = np.clip(u64, c["lo"], c["hi"])
    bound = (2 * nv + 2) * U * (np.abs(nominal) + mag) + 1e-6 * mag + 16 * U * np.abs(g).sum(-1)
    err = np.abs(u - u64)
    share = float(((u == c["lo"].astype(np.float32)) | (u == c["hi"].astype(np.float32))).mean())
    print(kind, "clamp" if clamp else "free", "median |gain dx| / range %.3f" % float(np.median(np.abs(fb) / (c["hi"] - c["lo"]))),
          "max err / bound %.3f" % float((err / bound).max()), "on a limit %.3f" % share)
    assert np.isfinite(u).all() and np.isfinite(u64).all()
    assert (err <= bound).all(), f"{kind}: {(err > bound).sum()} of {err.size} entries beyond the bound, worst ratio {(err / bound).max():.3f}"
    if clamp:
        assert 0.05 < share < 0.95, share
        assert (u >= c["lo"].astype(np.float32)).all() and (u <= c["hi"].astype(np.float32)).all()
    else:
        assert (np.abs(u - nominal) > 0).mean() > 0.99


# ---- 4. rows

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2rough"])
def test_rows_go_by_slot_and_by_sample(kind):
    import torch
    from rsr_mjx_amd import _lib
    c = _base(kind)
    A, pa = c["A"], c["pa"]
    nq, nv, nu = c["dims"]
    A.record.copy_(c["before"]["record"])
    shared_ctrl = c["ctrl"][:, 0].contiguous()                            # [N, T, nu]
    gain, qref, vref = c["gain"], c["qref"], c["vref"]
    # distinct per-sample rows under a shared 3-D ctrl: sample k uses row k, which is the slot-shared call made with that row
    per = pa.feedback_rollouts(shared_ctrl, gain, qref, vref, fields=WITH_CTRL)
    for k in range(K):
        one = pa.feedback_rollouts(shared_ctrl, gain[:, k].contiguous(), qref[:, k].contiguous(), vref[:, k].contiguous(), fields=WITH_CTRL, K=1)
        for f in WITH_CTRL:
            assert one[f].shape[:3] == (N, 1, T)
            assert_bitwise(f"{kind} row {k} {f}", per[f][:, k], one[f][:, 0])
    q = per["qpos"]
    assert all(not torch.equal(q[:, j], q[:, 0]) for j in range(1, K))    # the samples differ, by their gains alone
    # K identical rows give K identical samples, and are the slot-shared call with K = 3
    same = pa.feedback_rollouts(shared_ctrl, gain[:, :1].expand(-1, K, -1, -1, -1).contiguous(), qref[:, :1].expand(-1, K, -1, -1).contiguous(),
                                vref[:, :1].expand(-1, K, -1, -1).contiguous(), fields=WITH_CTRL)
    slot = pa.feedback_rollouts(shared_ctrl, gain[:, 0].contiguous(), qref[:, 0].contiguous(), vref[:, 0].contiguous(), fields=WITH_CTRL, K=K)
    for f in WITH_CTRL:
        for k in range(K):
            assert_bitwise(f"{kind} identical rows, sample {k} {f}", same[f][:, k], per[f][:, 0])
        assert_bitwise(f"{kind} slot-shared rows {f}", slot[f], same[f])
    # env_ids: caller-owned tensors for M = 3, each the head of a larger sentinel-filled buffer: written in full, nothing beyond
    full = _closed(kind)
    ids = [11, 3, 7]
    sub = [t[ids].contiguous() for t in (c["ctrl"], gain, qref, vref)]
    buf = {f: torch.full((len(ids) + 1,) + tuple(full[f].shape[1:]), -7.25, device=A.device) for f in WITH_CTRL}
    out = pa.feedback_rollouts(*sub, fields=WITH_CTRL, env_ids=ids, out={f: b[:len(ids)] for f, b in buf.items()})
    torch.cuda.synchronize()
    for f in WITH_CTRL:
        assert out[f].data_ptr() == buf[f].data_ptr()
        for s, e in enumerate(ids):
            assert_bitwise(f"{kind} slot {s} (env {e}) {f}", out[f][s], full[f][e])
        assert (buf[f][len(ids)] == -7.25).all(), f
    # an empty list launches nothing
    empty = pa.feedback_rollouts(*[t[:0] for t in sub], env_ids=[], fields=("qpos", "ctrl"))
    assert {f: tuple(t.shape) for f, t in empty.items()} == dict(qpos=(0, K, T, nq), ctrl=(0, K, T, nu))
    # the raw call: an id of num_envs runs nothing and leaves its slot's rows, ctrl_out's included, as they were
    for b in buf.values():
        b.fill_(-7.25)
    raw = torch.tensor([11, N, 7], dtype=torch.int32, device=A.device)
    o = _lib.RolloutOut()
    for f in ALL:
        setattr(o, f, buf[f].data_ptr())
    fb = _lib.Feedback(sub[1].data_ptr(), sub[2].data_ptr(), sub[3].data_ptr())
    rc = _lib.lib().rsr_physics_feedback_rollouts(pa._h, C.c_void_p(raw.data_ptr()), 3, C.c_void_p(sub[0].data_ptr()), C.byref(fb), None, K, T,
                                                  pa.n_substeps, _lib.FB_CTRL_PER_SAMPLE | _lib.FB_PER_SAMPLE, C.byref(o),
                                                  C.c_void_p(buf["ctrl"].data_ptr()), pa._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rsr_last_error()
    for f in WITH_CTRL:
        assert_bitwise(f"{kind} raw slot 0 {f}", buf[f][0], full[f][11])
        assert_bitwise(f"{kind} raw slot 2 {f}", buf[f][2], full[f][7])
        assert (buf[f][1] == -7.25).all() and (buf[f][3] == -7.25).all(), f
    assert_bitwise(f"{kind} record", A.record, c["before"]["record"])


# ---- 5. refusals

@pytest.mark.gpu
def test_refusals_on_the_device():
    import torch
    from rsr_mjx_amd import _lib
    c = _base("cube")
    A, pa = c["A"], c["pa"]
    nq, nv, nu = c["dims"]
    A.record.copy_(c["before"]["record"])
    L = _lib.lib()
    fn = L.rsr_physics_feedback_rollouts
    ctrl = C.c_void_p(c["ctrl"].data_ptr())
    qpos = torch.full((N, K, T, nq), -7.25, device=A.device)
    sd = torch.full((N, K, T, 64), -7.25, device=A.device)
    applied = torch.full((N, K, T, nu), -7.25, device=A.device)
    ids = torch.arange(2, dtype=torch.int32, device=A.device)
    o, none, o_sd = _lib.RolloutOut(), _lib.RolloutOut(), _lib.RolloutOut()
    o.qpos = qpos.data_ptr()
    o_sd.sensordata = sd.data_ptr()
    fb = _lib.Feedback(c["gain"].data_ptr(), c["qref"].data_ptr(), c["vref"].data_ptr())
    ipos = torch.zeros((N, K, A.dims.nbody, 3), device=A.device)
    mass = torch.ones((N, K, A.dims.nbody), device=A.device)
    ok, go2_only = _lib.ParamSamples(), _lib.ParamSamples()
    ok.leaf[_lib.DR_FIELDS.index("body_mass")] = mass.data_ptr()
    go2_only.leaf[_lib.DR_FIELDS.index("body_ipos")] = ipos.data_ptr()
    nf, both = pa.n_substeps, _lib.FB_CTRL_PER_SAMPLE | _lib.FB_PER_SAMPLE
    out_p, app_p, ps = C.byref(o), C.c_void_p(applied.data_ptr()), C.byref(ok)
    bare = _bare_handle(c)
    torch.cuda.synchronize()
    before = handle_snapshot(pa)

    def partial(**kw):                           # an fb with one member NULL
        f = _lib.Feedback(c["gain"].data_ptr(), c["qref"].data_ptr(), c["vref"].data_ptr())
        for k, v in kw.items():
            setattr(f, k, v)
        return C.byref(f)

    E_ARG, E_UNSUPPORTED = -1, -2
    big = 2 ** 31 - 1
    calls = [("null ctrl", (pa._h, None, 0, None, C.byref(fb), ps, K, T, nf, both, out_p, app_p), E_ARG),
             ("null fb", (pa._h, None, 0, ctrl, None, ps, K, T, nf, both, out_p, app_p), E_ARG),
             ("null gain", (pa._h, None, 0, ctrl, partial(gain=None), ps, K, T, nf, both, out_p, app_p), E_ARG),
             ("null qpos_ref", (pa._h, None, 0, ctrl, partial(qpos_ref=None), ps, K, T, nf, both, out_p, app_p), E_ARG),
             ("null qvel_ref", (pa._h, None, 0, ctrl, partial(qvel_ref=None), ps, K, T, nf, both, out_p, app_p), E_ARG),
             ("null out", (pa._h, None, 0, ctrl, C.byref(fb), ps, K, T, nf, both, None, app_p), E_ARG),
             ("nothing to record and null ctrl_out", (pa._h, None, 0, ctrl, C.byref(fb), ps, K, T, nf, both, C.byref(none), None), E_ARG),
             ("K = 0", (pa._h, None, 0, ctrl, C.byref(fb), ps, 0, T, nf, both, out_p, app_p), E_ARG),
             ("T = 0", (pa._h, None, 0, ctrl, C.byref(fb), ps, K, 0, nf, both, out_p, app_p), E_ARG),
             ("nsteps = 0", (pa._h, None, 0, ctrl, C.byref(fb), ps, K, T, 0, both, out_p, app_p), E_ARG),
             ("flag bit 3", (pa._h, None, 0, ctrl, C.byref(fb), ps, K, T, nf, both | 8, out_p, app_p), E_ARG),
             ("negative flags", (pa._h, None, 0, ctrl, C.byref(fb), ps, K, T, nf, -1, out_p, app_p), E_ARG),
             ("env_ids with count 0", (pa._h, C.c_void_p(ids.data_ptr()), 0, ctrl, C.byref(fb), ps, K, T, nf, both, out_p, app_p), E_ARG),
             ("M K at 2^31", (pa._h, None, 0, ctrl, C.byref(fb), ps, big, T, nf, both, out_p, app_p), E_ARG),
             ("T nsteps at 2^31", (pa._h, None, 0, ctrl, C.byref(fb), ps, K, big, 2, both, out_p, app_p), E_ARG),
             ("sensordata with no table", (bare._h, None, 0, ctrl, C.byref(fb), ps, K, T, nf, both, C.byref(o_sd), app_p), E_ARG),
             ("a Go2-only leaf", (pa._h, None, 0, ctrl, C.byref(fb), C.byref(go2_only), K, T, nf, both, out_p, app_p), E_UNSUPPORTED)]
    for what, args, code in calls:
        assert fn(*args, pa._stream()) == code, what
        assert b"rsr_physics_feedback_rollouts" in L.rsr_last_error(), what
    for leaf in range(_lib.DR_FIELDS.index("body_ipos"), len(_lib.DR_FIELDS)):      # each of the last five, one at a time
        one = _lib.ParamSamples()
        one.leaf[leaf] = ipos.data_ptr()
        assert fn(pa._h, None, 0, ctrl, C.byref(fb), C.byref(one), K, T, nf, both, out_p, app_p, pa._stream()) == E_UNSUPPORTED, _lib.DR_FIELDS[leaf]
        assert b"rsr_physics_feedback_rollouts" in L.rsr_last_error()
    torch.cuda.synchronize()
    assert_unchanged(before, handle_snapshot(pa))
    assert (qpos == -7.25).all() and (sd == -7.25).all() and (applied == -7.25).all()
    # an out with nothing to record is served when ctrl_out is given: the applied controls alone
    assert fn(pa._h, None, 0, ctrl, C.byref(fb), None, K, T, nf, both, C.byref(none), app_p, pa._stream()) == 0, L.rsr_last_error()
    torch.cuda.synchronize()
    assert_bitwise("cube ctrl_out alone", applied, _closed("cube")["ctrl"])
    assert (qpos == -7.25).all()
    assert_unchanged(before, handle_snapshot(pa))


def _bare_handle(c):
    """a second handle on the same batch with no sensor table set"""
    from rsr_mjx_amd.physics import Physics
    return Physics(c["A"])
