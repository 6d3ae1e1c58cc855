"""Applied forces (data.xfrc_applied / data.qfrc_applied: Physics.set_applied, rsr_physics_set_applied) on every built family:
zero forces change nothing, a rollout with held forces is its steps bit for bit, the body wrench is J^T w against fp64 kinematics,
qfrc goes through the full solver like an actuator force, a free body accelerates as Newton-Euler says, the Go2 kick written on
Physics lands on the env's own kick, and set_state / views / errors behave."""
import numpy as np
import pytest

from physics_support import FAMILIES, PIPE, assert_bitwise, handle_snapshot, make, pair, random_states, rel, rule
from rsr_mjx_amd import prng

AIRBOT_SPEC = [("pos", "framepos", "endpoint"), ("gyro", "gyro", "endpoint"), ("vel", "velocimeter", "endpoint")]


def _spec(kind, envdef):
    return AIRBOT_SPEC if kind in ("cube", "tshape") else envdef.sensors


def _outputs(E, phys):
    import torch
    torch.cuda.synchronize()
    out = {k: E.view(k).clone() for k in PIPE}
    out.update(handle_snapshot(phys, ("side",)))
    return out


def _assert_same(a, b, what):
    import torch
    for k in a:
        assert_bitwise(f"{what}: {k}", a[k], b[k])
        assert torch.equal(a[k], b[k]), f"{what}: {k} holds a NaN"


def _forces(envdef, n, rng, scale=1.0):
    """Random xfrc on every body (row 0 too: the world row must be ignored) of the order of the body's weight."""
    A = envdef.sys.arrays
    m = np.maximum(A["body_mass"], 0.05)[None, :, None]
    x = rng.normal(size=(n, len(A["body_mass"]), 6))
    x[:, :, :3] *= 9.81 * m * scale
    x[:, :, 3:] *= 0.1 * 9.81 * m * scale
    return x.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_zero_applied_forces_change_nothing(kind):
    """Applied forces on but zero: step (1 and n_frames), forward, forward_envs and rollout leave the record, side buffer and
    sensordata exactly as on a handle that never turned them on; the same after clear_applied()."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 256
    envdef, A, B, scale, rng = pair(kind, n)
    pa, pb = Physics(A, sensors=_spec(kind, envdef)), Physics(B, sensors=_spec(kind, envdef))
    pb.set_applied()
    assert pb.xfrc_applied is not None and not pb.xfrc_applied.any() and not pb.qfrc_applied.any()
    nf = pa.n_substeps
    ctrl = lambda: torch.as_tensor(np.clip(rng.normal(size=(n, A.dims.nu)) * scale, -1, 1).astype(np.float32), device=A.device)
    ids = [5, 9, 100, 200]
    qpos, qvel, c0 = (A.view(k)[ids].clone() for k in ("qpos", "qvel", "ctrl"))
    T = 3
    cr = torch.stack([ctrl() for _ in range(T)], 1)
    for label, run in (("step1", lambda p, c: p.step(c, 1)), ("stepN", lambda p, c: p.step(c, nf)),
                       ("forward", lambda p, c: p.forward()),
                       ("forward_envs", lambda p, c: p.set_state(qpos, qvel, c0, env_ids=ids)),
                       ("rollout", lambda p, c: p.rollout(cr, fields=("qpos", "qvel", "actuator_force", "sensordata")))):
        c = ctrl()
        ra, rb = run(pa, c), run(pb, c)
        _assert_same(_outputs(A, pa), _outputs(B, pb), f"{kind} {label}")
        if label == "rollout":
            _assert_same(ra, rb, f"{kind} rollout trajectories")
    pb.clear_applied()
    assert pb.xfrc_applied is None and pb.qfrc_applied is None
    c = ctrl()
    pa.step(c, nf); pb.step(c, nf)
    _assert_same(_outputs(A, pa), _outputs(B, pb), f"{kind} after clear_applied")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_rollout_with_applied_forces_equals_steps(kind):
    """A rollout with non-zero held forces is T step calls with the same forces, bit for bit."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n, T = 256, 4
    envdef, A, B, scale, rng = pair(kind, n)
    pa, pb = Physics(A, sensors=_spec(kind, envdef)), Physics(B, sensors=_spec(kind, envdef))
    x = _forces(envdef, n, rng, 0.3)
    q = (rng.normal(size=(n, A.dims.nv)) * 0.5).astype(np.float32)
    pa.set_applied(x, q); pb.set_applied(x, q)
    assert pa.xfrc_applied.any() and pa.qfrc_applied.any()
    c = torch.as_tensor(np.clip(rng.normal(size=(n, T, A.dims.nu)) * scale, -1, 1).astype(np.float32), device=A.device)
    res = pa.rollout(c, fields=("qpos", "qvel", "time", "actuator_force", "ncon", "sensordata"))
    for t in range(T):
        pb.step(c[:, t])
        torch.cuda.synchronize()
        for k, v in (("qpos", B.view("qpos")), ("qvel", B.view("qvel")), ("actuator_force", pb.actuator_force),
                     ("sensordata", pb.sensordata)):
            assert torch.equal(res[k][:, t], v), f"{kind} t={t} {k}"
    _assert_same(_outputs(A, pa), _outputs(B, pb), f"{kind} rollout vs steps")


def _jt(envdef, o, x):
    """qfrc = sum over bodies b >= 1 of J_b(xipos_b)^T [f; tau], fp64, from the oracle's cdof / xipos / subtree_com."""
    A = envdef.sys.arrays
    nb, nv = len(A["body_mass"]), len(A["dof_bodyid"])
    parent, root, dof_body = A["body_parentid"], A["body_rootid"], A["dof_bodyid"]
    cdof = o.get("cdof").reshape(nv, 6)
    xipos = o.get("xipos").reshape(nb, 3)
    com = o.get("subtree_com").reshape(nb, 3)
    q = np.zeros(nv)
    for b in range(1, nb):
        f, tau = x[b, :3].astype(np.float64), x[b, 3:].astype(np.float64)
        w = np.concatenate([tau + np.cross(xipos[b] - com[root[b]], f), f])
        chain, k = set(), b
        while k > 0:
            chain.add(k); k = parent[k]
        for i in range(nv):
            if dof_body[i] in chain:
                q[i] += cdof[i] @ w
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_xfrc_is_jacobian_transpose(oracle_mod, kind):
    """forward with xfrc only against forward with qfrc = sum J_b^T w_b (fp64 host, oracle kinematics), from random states."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 256
    envdef, E, _, _ = make(kind, n, False)
    E.reset(prng.split(prng.PRNGKey(1), n))
    qpos, qvel, ctrl = random_states(envdef, kind, n, 21)
    rng = np.random.default_rng(21)
    x = _forces(envdef, n, rng)
    o64 = oracle_mod.Oracle(E.blob, "f64"); o64.set_ncon_cap(E.dims.ncon_max)
    q = np.zeros((n, E.dims.nv))
    for e in range(n):
        o64.forward(qpos[e], qvel[e], ctrl[e], np.zeros(E.dims.nv), step=False)
        q[e] = _jt(envdef, o64, x[e])
    phys = Physics(E)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    warm = phys.qacc_warmstart.clone()            # both runs below start from the same warm start
    phys.set_applied(xfrc=x)
    phys.forward()
    torch.cuda.synchronize()
    acc_x, ncon_x = phys.qacc.cpu().numpy().copy(), phys.contacts()["ncon"].cpu().numpy()
    phys.qacc_warmstart.copy_(warm)
    phys.set_applied(xfrc=np.zeros_like(x), qfrc=q.astype(np.float32))
    phys.forward()
    torch.cuda.synchronize()
    acc_q, ncon_q = phys.qacc.cpu().numpy(), phys.contacts()["ncon"].cpu().numpy()
    flips = ncon_x != ncon_q
    assert flips.sum() <= max(2, n // 50), f"{kind}: contact sets differ in {flips.sum()} envs"
    err = rel(acc_x, acc_q)[~flips]
    p99 = float(np.quantile(err, 0.99))
    print(kind, "xfrc vs J^T qfrc: qacc p99 %.2e max %.2e, flips %d" % (p99, err.max(), flips.sum()))
    assert p99 <= 1e-5 and err.max() <= 1e-4, (kind, p99, err.max())
    assert np.abs(acc_x).max() > 0


def _clamp_free(A, af, sh):
    """Per actuator: no force clamp (actuator forcerange, joint actfrcrange) binds in a forward pass whose actuator forces are
    `af` under the shifted ctrl, nor would it under the unshifted one (af - gain * shift)."""
    gp = A["actuator_gainprm"]
    gain, gear = gp[:, 0], A["actuator_gear"]
    jnt = A["actuator_trnid"]
    ok = np.ones(len(gain), bool)
    for f in (af, af - gain * sh):
        lo, hi = A["actuator_forcerange"][:, 0], A["actuator_forcerange"][:, 1]
        ok &= ~A["actuator_forcelimited"].astype(bool) | ((f > lo + 1e-6 * np.abs(lo)) & (f < hi - 1e-6 * np.abs(hi)))
        t = gear * f
        lo, hi = A["jnt_actfrcrange"][jnt, 0], A["jnt_actfrcrange"][jnt, 1]
        ok &= ~A["jnt_actfrclimited"][jnt].astype(bool) | ((t > lo + 1e-6 * np.abs(lo)) & (t < hi - 1e-6 * np.abs(hi)))
    return ok


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_qfrc_through_the_solver_matches_the_oracle(oracle_mod, kind):
    """qfrc_applied = Q on actuated dofs with a joint transmission equals shifting ctrl by Q / (gear * gain) where no clamp binds:
    GPU forward / step with Q against the f32 / f64 oracle with the shifted ctrl.  Actuators whose force would clamp at the start
    get no shift; envs where a shifted actuator reaches a clamp during the substeps are left out (counted, bounded); contact-mode
    flips are counted and bounded as in test_physics_oracle_parity."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 128
    envdef, E, _, _ = make(kind, n, False)
    E.reset(prng.split(prng.PRNGKey(1), n))
    qpos, qvel, _ = random_states(envdef, kind, n, 31)
    A = envdef.sys.arrays
    gain, gear = A["actuator_gainprm"][:, 0], A["actuator_gear"]
    dof = A["jnt_dofadr"][A["actuator_trnid"]]
    lo, hi = A["actuator_ctrlrange"][:, 0], A["actuator_ctrlrange"][:, 1]
    rng = np.random.default_rng(31)
    # position servos near their joint's angle, so that the forces stay inside their ranges
    qadr = A["jnt_qposadr"][A["actuator_trnid"]]
    ctrl = np.clip(qpos[:, qadr] + (hi - lo) * rng.uniform(-0.02, 0.02, size=(n, len(lo))), lo, hi).astype(np.float32)
    shift = (np.clip(ctrl + (hi - lo) * rng.uniform(-0.02, 0.02, size=ctrl.shape), lo, hi) - ctrl).astype(np.float32)
    o32 = oracle_mod.Oracle(E.blob); o32.set_ncon_cap(E.dims.ncon_max)
    o64 = oracle_mod.Oracle(E.blob, "f64"); o64.set_ncon_cap(E.dims.ncon_max)
    for e in range(n):
        o64.forward(qpos[e], qvel[e], ctrl[e] + shift[e], np.zeros(E.dims.nv), step=False)
        shift[e, ~_clamp_free(A, o64.get("actuator_force"), shift[e])] = 0.0
    assert (shift != 0).mean() > 0.1, f"{kind}: clamps bind on almost every actuator"
    ctrl2 = (ctrl + shift).astype(np.float32)
    Q = np.zeros((n, E.dims.nv), np.float32)
    Q[:, dof] = (gear * gain)[None, :] * (ctrl2.astype(np.float64) - ctrl)
    phys = Physics(E)
    nf = phys.n_substeps
    fields = ("qacc", "qvel", "qpos")
    fails = []
    for mode, nsteps in (("forward", 0), ("stepN", nf)):
        phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)     # (zeroes the applied rows: set them again and redo mjx_env.init)
        phys.set_applied(qfrc=Q)
        phys.qacc_warmstart.zero_()
        phys.forward()
        if nsteps:
            phys.step(None, nsteps)
        torch.cuda.synchronize()
        hip = {"qacc": phys.qacc.cpu().numpy(), "qvel": phys.qvel.cpu().numpy(), "qpos": phys.qpos.cpu().numpy()}
        ref = {p: {f: np.zeros_like(hip[f], dtype=np.float64) for f in fields} for p in ("f32", "f64")}
        ncon = {p: np.zeros(n, int) for p in ("f32", "f64")}
        clamp = np.zeros(n, bool)
        for e in range(n):
            moved = shift[e] != 0
            for p, o in (("f32", o32), ("f64", o64)):
                q, v = qpos[e].astype(np.float64), qvel[e].astype(np.float64)
                o.forward(q, v, ctrl2[e], np.zeros(E.dims.nv), step=False)
                for s in range(nsteps + 1):
                    if p == "f64":
                        clamp[e] |= (~_clamp_free(A, o.get("actuator_force"), shift[e]) & moved).any()
                    if s == nsteps:
                        break
                    w = o.get("qacc")
                    o.forward(q, v, ctrl2[e], w, step=True)
                    q, v = o.get("qpos"), o.get("qvel")
                for f in fields:
                    ref[p][f][e] = o.get(f)
                ncon[p][e] = int(o.get("counts")[3])
        hip_ncon = phys.contacts()["ncon"].cpu().numpy()
        flips = (hip_ncon != ncon["f64"]) | (ncon["f32"] != ncon["f64"])
        if flips.mean() > 0.02:
            fails.append(f"{kind} {mode}: contact-mode flips in {flips.sum()} of {n} envs")
        if clamp.mean() > 0.25:                         # (those envs are left out of the comparison)
            fails.append(f"{kind} {mode}: a shifted actuator reaches a clamp in {clamp.sum()} of {n} envs")
        keep = ~flips & ~clamp
        for f in fields if nsteps else ("qacc",):
            err = rel(hip[f], ref["f64"][f])[keep]
            spread = rel(ref["f32"][f], ref["f64"][f])[keep]
            print(kind, mode, f, "flips %d, clamped %d" % (flips.sum(), clamp.sum()))
            rule(kind, f"{mode} {f}", err, spread, fails)
    assert not fails, fails


@pytest.mark.gpu
def test_free_body_newton_euler(oracle_mod):
    """The Airbot cube, DR off, away from every other geom at rest: a force m g up holds it (|qacc| <= 1e-4 g on its free
    joint), and a pure torque gives the angular acceleration of Euler's equations at rest, I^-1 tau in its own frame."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 64
    envdef, E, _, _ = make("cube", n, False)
    E.reset(prng.split(prng.PRNGKey(1), n))
    A = envdef.sys.arrays
    j = int(np.nonzero(A["jnt_type"] == 0)[0][0])                # the cube's free joint
    b, qa, da = int(A["jnt_bodyid"][j]), int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
    assert (A["dof_armature"][da:da + 6] == 0).all() and (A["dof_damping"][da:da + 6] == 0).all()
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    qpos = E.view("qpos").cpu().numpy().copy()
    qpos[:, qa:qa + 3] = [1.5, -1.5, 1.0]                          # far from the arm, the floor and the target
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    qpos[:, qa + 3:qa + 7] = quat
    qvel = np.zeros((n, E.dims.nv), np.float32)
    ctrl = E.view("ctrl").cpu().numpy()
    o = oracle_mod.Oracle(E.blob, "f64"); o.set_ncon_cap(E.dims.ncon_max)
    for e in range(0, n, 8):
        o.forward(qpos[e], qvel[e], ctrl[e], None)
        J = o.get("efc_J").reshape(-1, E.dims.nv)
        assert not J[:, da:da + 6].any(), f"env {e}: a constraint row touches the cube"
    g, m = 9.81, float(A["body_mass"][b])
    phys = Physics(E)
    phys.set_state(qpos=qpos.astype(np.float32), qvel=qvel, ctrl=ctrl)
    x = np.zeros((n, len(A["body_mass"]), 6), np.float32)
    x[:, b, 2] = m * g
    phys.set_applied(xfrc=x)
    phys.qacc_warmstart.zero_()      # (the solve starts from qacc_smooth: an unconverged warm start could stand for the answer)
    phys.forward()
    torch.cuda.synchronize()
    acc = phys.qacc.cpu().numpy()[:, da:da + 6]
    assert np.abs(acc).max() <= 1e-4 * g, np.abs(acc).max()
    # pure torque: angular qacc (body frame of the free joint) = R^T I_w^-1 tau, I_w = Ri diag(I) Ri^T
    tau = rng.normal(size=(n, 3)) * 1e-2
    x[:, b, 3:] = tau                                              # (and m g up: no linear acceleration)
    phys.set_applied(xfrc=x)
    phys.qacc_warmstart.zero_()
    phys.forward()
    torch.cuda.synchronize()
    acc = phys.qacc.cpu().numpy()[:, da:da + 6].astype(np.float64)
    I = A["body_inertia"][b].astype(np.float64)
    for e in range(n):
        o.forward(qpos[e], qvel[e], ctrl[e], None)
        R = o.get("xmat").reshape(-1, 3, 3)[b]
        Ri = o.get("ximat").reshape(-1, 3, 3)[b]
        want = R.T @ (Ri @ ((Ri.T @ tau[e].astype(np.float32).astype(np.float64)) / I))
        assert np.abs(acc[e, :3]).max() <= 1e-4 * g, (e, acc[e, :3])
        np.testing.assert_allclose(acc[e, 3:], want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["go2flat"])
def test_go2_kick_on_physics(kind):
    """The reference's perturbation kick (joystick.py's xfrc_applied on the torso) written on Physics: teacher-forced as in
    test_physics_step_is_bit_identical_to_env_step, with pert_config enabled and no wrappers.  physics.step with
    xfrc_applied[:, torso, :3] = that step's info_go2[139:142] lands on the env step: bitwise where no kick is active, within
    p99 1e-5 (every env 1e-4) where one is (the env adds J^T f to qfrc_smooth after the actuator forces, the applied path through
    the subtree force sums: different rounding)."""
    import torch
    from rsr_mjx_amd.envs import go2
    from rsr_mjx_amd.physics import Physics
    n = 1024
    over = {"pert_config": {"enable": True, "kick_wait_times": [0.1, 0.3], "velocity_kick": [1.0, 4.0]}}
    envs = []
    for _ in range(2):
        jenv = go2.load("Go2JoystickFlatTerrain", config_overrides=over)
        dr = go2.domain_randomize(jenv.sys, prng.split(prng.PRNGKey(12), n))
        envs.append((jenv, jenv.batched(n, randomization=dr)))
    (jenv, A), (_, B) = envs
    sa = jenv.sys.arrays
    torso = int(sa["jnt_bodyid"][int(np.nonzero(sa["jnt_type"] == 0)[0][0])])
    rng = np.random.default_rng(3)
    act = lambda: np.clip(rng.normal(size=(n, A.dims.nu)) * 0.5, -1, 1).astype(np.float32)
    A.reset(prng.split(prng.PRNGKey(7), n))
    B.reset(prng.split(prng.PRNGKey(8), n))
    phys = Physics(B)
    x = torch.zeros((n, B.dims.nbody, 6), dtype=torch.float32, device=B.device)
    kicked, errs = 0, []
    for _ in range(12):
        A.step(None, act())
    for rnd in range(8):
        for k in PIPE:
            B.view(k).copy_(A.view(k))
        A.step(None, act())
        torch.cuda.synchronize()
        f = A.view("info_go2")[:, 139:142].clone()
        on = (f != 0).any(1).cpu().numpy()
        x.zero_(); x[:, torso, :3] = f
        phys.set_applied(xfrc=x)
        phys.step(A.view("ctrl").clone(), phys.n_substeps)
        torch.cuda.synchronize()
        kicked += int(on.sum())
        for k in ("qpos", "qvel", "xpos"):
            a, b = A.view(k).cpu().numpy(), B.view(k).cpu().numpy()
            same = (a == b).all(1)
            assert same[~on].all(), f"round {rnd} {k}: {(~same[~on]).sum()} envs without a kick differ"
            if on.any():
                errs.append((k, rel(b[on], a[on])))
    assert kicked > 0, "no kick happened"
    for k in ("qpos", "qvel", "xpos"):
        e = np.concatenate([v for kk, v in errs if kk == k])
        p99 = float(np.quantile(e, 0.99))
        print(kind, k, "kicked env-steps %d, p99 %.2e max %.2e" % (len(e), p99, e.max()))
        assert p99 <= 1e-5 and e.max() <= 1e-4, (k, p99, e.max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_applied_state_views_and_errors(kind):
    import ctypes as C
    import torch
    from rsr_mjx_amd import _lib
    from rsr_mjx_amd.physics import Physics
    n = 64
    envdef, E, _, _ = make(kind, n, False)
    E.reset(prng.split(prng.PRNGKey(4), n))
    phys = Physics(E)
    d = E.dims
    assert phys.xfrc_applied is None and phys.qfrc_applied is None
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    L = _lib.lib()
    assert L.rsr_physics_applied_view(phys._h, 0, C.byref(ptr), shape, stride) == -1         # off
    assert L.rsr_physics_set_applied(phys._h, 2) == -1 and L.rsr_physics_set_applied(phys._h, -1) == -1
    rng = np.random.default_rng(0)
    x = rng.normal(size=(n, d.nbody, 6)).astype(np.float32)
    q = rng.normal(size=(n, d.nv)).astype(np.float32)
    phys.set_applied(x, q)
    assert tuple(phys.xfrc_applied.shape) == (n, d.nbody, 6) and tuple(phys.qfrc_applied.shape) == (n, d.nv)
    assert L.rsr_physics_applied_view(phys._h, 2, C.byref(ptr), shape, stride) == -1             # unknown id
    assert L.rsr_physics_applied_view(phys._h, 1, C.byref(ptr), shape, stride) == 0 and tuple(shape) == (n, d.nv)
    np.testing.assert_array_equal(phys.xfrc_applied.cpu().numpy(), x)
    # turning on again keeps the values; a subset write touches only its rows, in env_ids order
    phys.set_applied()
    np.testing.assert_array_equal(phys.qfrc_applied.cpu().numpy(), q)
    ids = [7, 3]
    phys.set_applied(qfrc=np.ones((2, d.nv), np.float32) * np.array([[1.0], [2.0]], np.float32), env_ids=ids)
    qq = phys.qfrc_applied.cpu().numpy()
    assert (qq[7] == 1).all() and (qq[3] == 2).all()
    others = np.setdiff1d(np.arange(n), ids)
    np.testing.assert_array_equal(qq[others], q[others])
    np.testing.assert_array_equal(phys.xfrc_applied.cpu().numpy(), x)
    # the views are writable and are what the kernels read
    phys.xfrc_applied[:, :, :] = 0.0
    phys.qfrc_applied[:, :] = 0.0
    assert not phys.xfrc_applied.any()
    phys.set_applied(x, q)
    # set_state(env_ids) zeroes exactly those rows (mjx_env.init: a fresh Data)
    torch.cuda.synchronize()
    sid = np.array([1, 30, 63])
    phys.set_state(qpos=E.view("qpos")[sid].clone(), env_ids=sid)
    xx, qq = phys.xfrc_applied.cpu().numpy(), phys.qfrc_applied.cpu().numpy()
    assert not xx[sid].any() and not qq[sid].any()
    rest = np.setdiff1d(np.arange(n), sid)
    np.testing.assert_array_equal(xx[rest], x[rest]); np.testing.assert_array_equal(qq[rest], q[rest])
    # errors
    with pytest.raises(ValueError):
        phys.set_applied(xfrc=x[:, :-1])
    with pytest.raises(ValueError):
        phys.set_applied(qfrc=q[:, :-1])
    with pytest.raises(ValueError):
        phys.set_applied(qfrc=q[:2], env_ids=[0])
    with pytest.raises(ValueError):
        phys.set_applied(qfrc=q[:1], env_ids=[n])
    with pytest.raises(ValueError):
        phys.set_applied(qfrc=q[:2], env_ids=[4, 4])
    np.testing.assert_array_equal(phys.qfrc_applied.cpu().numpy()[rest], q[rest])   # nothing written on error
    phys.clear_applied()
    assert phys.xfrc_applied is None and phys.qfrc_applied is None
    assert L.rsr_physics_applied_view(phys._h, 0, C.byref(ptr), shape, stride) == -1
    phys.set_applied()                                    # back on: zeroed by the clear
    assert not phys.xfrc_applied.any() and not phys.qfrc_applied.any()
