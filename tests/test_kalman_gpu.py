"""The Kalman filter and RTS smoother on the device (rsr_physics_kalman, Physics.kalman_smooth, csrc/physics/rsr_kalman.hpp) for the
three state widths the families give (cube nx = 40, Go2 36, T-shape 28): against the fp64 recursion of tests/kalman_ref.py under the
project's error rule, with the fp32 numpy recursion's own distance from fp64 as the spread; the slots' independence, the filter
alone, symmetry, missing entries and padding bit for bit; the failure protocol; nothing else written; and the hand-over from
trajectory_fd and sample_rollouts, with a known start deviation recovered.  The handle only supplies nv and nu: the inputs are
kalman_ref.inputs, whose conditioning tests/test_kalman_ref.py checks on the CPU."""
import functools

import numpy as np
import pytest

import kalman_ref
from physics_support import assert_bitwise, assert_unchanged, handle_snapshot, make, rel, rule
from rsr_mjx_amd import prng

pytestmark = pytest.mark.gpu

FAMILIES = list(kalman_ref.FAMILY_NX)
M = kalman_ref.M
SENTINEL = 12345.0
NAMES = ("xf", "Pf", "xs", "Ps", "nll", "status")


@functools.lru_cache(maxsize=None)
def _handle(kind):
    """(env, Physics, nx, nu) of a 4-env batch after a reset: the call takes of it nv, nu and the device"""
    import torch
    from rsr_mjx_amd.physics import Physics
    _, E, _, _ = make(kind, 4, False)
    E.reset(prng.split(prng.PRNGKey(1), 4))
    torch.cuda.synchronize()
    assert 2 * int(E.dims.nv) == kalman_ref.FAMILY_NX[kind]
    return E, Physics(E), 2 * int(E.dims.nv), int(E.dims.nu)


def _run(kind, inp, stride=None, fill=0.0, slots=None, x0=True, smooth=True, covariances=True, out=None):
    """Physics.kalman_smooth on the numpy inputs `inp` (the slots `slots` of them, packed at `stride`); the outputs on the device"""
    import torch
    E, phys, nx, nu = _handle(kind)
    sl = slice(None) if slots is None else list(slots)
    dev = lambda a: torch.as_tensor(np.array(a[sl]), device=E.device)            # (a copy: the shared inputs are read-only)
    col = dev(kalman_ref.pack(inp["A"], inp["C"], nu, stride, fill))
    res = phys.kalman_smooth(col, dev(inp["dy"]), dev(inp["r"]), dev(inp["q"]), dev(inp["P0"]), x0=dev(inp["x0"]) if x0 else None,
                             smooth=smooth, covariances=covariances and smooth, out=out)
    torch.cuda.synchronize()
    return res


def _run_c(kind, inp, stride, fill):
    """rsr_physics_kalman itself, with a row_stride beyond nx + ny (Physics.kalman_smooth takes ny from the width): smoothing, every
    output asked for"""
    import ctypes as C
    import torch
    from rsr_mjx_amd import _lib
    E, phys, nx, nu = _handle(kind)
    Mc, T, ny, _ = inp["C"].shape
    dev = lambda a: torch.as_tensor(np.array(a), device=E.device)
    col = dev(kalman_ref.pack(inp["A"], inp["C"], nu, stride, fill))
    ins = {k: dev(inp[k]) for k in ("dy", "r", "q", "x0", "P0")}
    shapes = dict(xf=(Mc, T + 1, nx), pf=(Mc, T + 1, nx, nx), xs=(Mc, T + 1, nx), ps=(Mc, T + 1, nx, nx), nll=(Mc,), status=(Mc, 2))
    out = {k: torch.empty(s, dtype=torch.float32, device=E.device) for k, s in shapes.items()}
    rc = _lib.lib().rsr_physics_kalman(phys._h, Mc, T, C.c_void_p(col.data_ptr()), stride, ny,
                                       C.byref(_lib.KalmanIn(**{k: t.data_ptr() for k, t in ins.items()})), 0,
                                       C.byref(_lib.KalmanOut(**{k: t.data_ptr() for k, t in out.items()})), phys._stream())
    assert rc == 0, _lib.lib().rsr_last_error()
    torch.cuda.synchronize()
    return dict(xf=out["xf"], Pf=out["pf"], xs=out["xs"], Ps=out["ps"], nll=out["nll"], status=out["status"])


def _prefilled(kind, T):
    import torch
    E, _, nx, _ = _handle(kind)
    shapes = dict(xf=(M, T + 1, nx), Pf=(M, T + 1, nx, nx), xs=(M, T + 1, nx), Ps=(M, T + 1, nx, nx), nll=(M,), status=(M, 2))
    return {k: torch.full(s, SENTINEL, device=E.device) for k, s in shapes.items()}


@pytest.mark.parametrize("kind", FAMILIES)
def test_against_fp64(kind):
    fails = []
    for T, ny in kalman_ref.shapes(kind):
        inp, r64, r32 = kalman_ref.family_case(kind, T, ny)
        got = _run(kind, inp)
        assert (got["status"].cpu().numpy() == -1).all(), (T, ny, got["status"])
        for k in kalman_ref.OUTPUTS:
            rule(kind, f"T={T} ny={ny} {k}", rel(got[k].cpu().numpy(), r64[k]), rel(r32[k], r64[k]), fails)
    assert not fails, fails


@pytest.mark.parametrize("kind", FAMILIES)
def test_bitwise_properties(kind):
    import torch
    _, _, nx, nu = _handle(kind)
    T, ny = 6, 55
    inp, _, _ = kalman_ref.family_case(kind, T, ny)
    base = _run(kind, inp)
    for k in NAMES:
        assert bool(torch.isfinite(base[k]).all()), k
    # the unread entries of a row and the B / D rows change nothing
    wide = _run_c(kind, inp, stride=nx + ny + 5, fill=SENTINEL)
    for k in NAMES:
        assert_bitwise(f"{kind} padding {k}", wide[k], base[k])
    # a slot's result depends on that slot's inputs alone, whatever M is and wherever the slot stands
    pick = [5, 0, 17]
    few = _run(kind, inp, slots=pick)
    for k in NAMES:
        assert_bitwise(f"{kind} slots {k}", few[k], base[k][pick])
    perm = list(np.random.default_rng(2).permutation(M))
    shuffled = _run(kind, inp, slots=perm)
    for k in NAMES:
        assert_bitwise(f"{kind} permutation {k}", shuffled[k], base[k][perm])
    # from run to run
    again = _run(kind, inp)
    for k in NAMES:
        assert_bitwise(f"{kind} rerun {k}", again[k], base[k])
    # the filter alone gives the smoothing call's filter outputs
    lean = _run(kind, inp, smooth=False)
    assert sorted(lean) == ["Pf", "nll", "status", "xf"]
    for k in lean:
        assert_bitwise(f"{kind} smooth=False {k}", lean[k], base[k])
    # ... and without the covariances the same means
    means = _run(kind, inp, covariances=False)
    assert sorted(means) == ["Pf", "nll", "status", "xf", "xs"]
    for k in means:
        assert_bitwise(f"{kind} covariances=False {k}", means[k], base[k])
    # Pf and Ps are symmetric bit for bit; the last smoothed row is the last filtered one
    assert_bitwise(f"{kind} Pf symmetric", base["Pf"], base["Pf"].transpose(2, 3))
    assert_bitwise(f"{kind} Ps symmetric", base["Ps"], base["Ps"].transpose(2, 3))
    assert_bitwise(f"{kind} xs[T]", base["xs"][:, T], base["xf"][:, T])
    assert_bitwise(f"{kind} Ps[T]", base["Ps"][:, T], base["Pf"][:, T])
    # no x0 is a zero x0
    zero = dict(inp, x0=np.zeros_like(inp["x0"]))
    with_zero, without = _run(kind, zero), _run(kind, zero, x0=False)
    assert not torch.equal(with_zero["xs"], base["xs"])
    for k in NAMES:
        assert_bitwise(f"{kind} x0 {k}", without[k], with_zero[k])
    # entries with r = +inf are the same problem with those sensor columns removed and ny smaller
    gone = [0, 7, 8, 30, 54]
    keep = [j for j in range(ny) if j not in gone]
    r = inp["r"].copy()
    r[:, :, gone] = np.inf
    a, b = _run(kind, dict(inp, r=r)), _run(kind, kalman_ref.drop_columns(inp, keep))
    assert not torch.equal(a["xs"], base["xs"])
    for k in NAMES:
        assert_bitwise(f"{kind} missing {k}", a[k], b[k])


@pytest.mark.parametrize("kind", FAMILIES)
def test_failure_stops_the_slot_alone(kind):
    import torch
    T, ny = 6, 55
    inp, _, _ = kalman_ref.family_case(kind, T, ny)
    base = _run(kind, inp)
    bad_r, t0, bad_s, bad_pm = 3, 2, 9, 20
    failing = kalman_ref.failing
    mod = failing(failing(failing(inp, "r", bad_r, t0), "s", bad_s), "pm", bad_pm)
    ref, ref32 = kalman_ref.smooth(**mod), kalman_ref.smooth(**mod, dtype=np.float32)
    want = -np.ones((M, 2))
    want[bad_r, 0], want[bad_s, 0], want[bad_pm, 1] = t0, 0, T - 1
    assert np.array_equal(ref["status"], want)                     # (the fp64 recursion fails there too)
    got = _run(kind, mod, out=_prefilled(kind, T))
    assert np.array_equal(got["status"].cpu().numpy(), want), got["status"]
    ok = [s for s in range(M) if s not in (bad_r, bad_s, bad_pm)]
    for k in NAMES:
        assert_bitwise(f"{kind} {k} other slots", got[k][ok], base[k][ok])
    # a filter failure at t: rows < t as they were written, rows >= t left alone, nll 0, no smoother
    for s, t in ((bad_r, t0), (bad_s, 0)):
        assert float(got["nll"][s]) == 0.0
        for k in ("xf", "Pf"):
            assert_bitwise(f"{kind} {k} rows < t", got[k][s, :t], base[k][s, :t])
            assert (got[k][s, t:] == SENTINEL).all(), (k, s)
        assert (got["xs"][s] == SENTINEL).all() and (got["Ps"][s] == SENTINEL).all()
    # a smoother failure at T - 1: the filter's outputs stand (fp64 rule), xs / Ps rows <= T - 1 left alone, row T written
    s = bad_pm
    fails = []
    for k in ("xf", "Pf", "nll"):
        rule(kind, f"singular Pm {k}", rel(got[k][s:s + 1].cpu().numpy(), ref[k][s:s + 1]), rel(ref32[k][s:s + 1], ref[k][s:s + 1]), fails)
    assert not fails, fails
    assert float(got["nll"][s]) != 0.0
    for k, f in (("xs", "xf"), ("Ps", "Pf")):
        assert (got[k][s, :T] == SENTINEL).all(), k
        assert_bitwise(f"{kind} {k}[T]", got[k][s, T], got[f][s, T])
    # a NaN variance in one slot: that slot fails at its step, the call returns, the others are untouched
    nan = {k: v.copy() for k, v in inp.items()}
    nan["r"][12, 4, 30] = np.nan
    got = _run(kind, nan, out=_prefilled(kind, T))
    status = got["status"].cpu().numpy()
    rest = [s for s in range(M) if s != 12]
    assert tuple(status[12]) == (4, -1) and (status[rest] == -1).all(), status
    assert (got["xf"][12, 4:] == SENTINEL).all() and (got["xs"][12] == SENTINEL).all()
    for k in NAMES:
        assert_bitwise(f"{kind} {k} slots without the NaN", got[k][rest], base[k][rest])


@pytest.mark.parametrize("kind", FAMILIES)
def test_nothing_else_is_written(kind):
    _, phys, _, _ = _handle(kind)
    inp, _, _ = kalman_ref.family_case(kind, 6, 55)
    before = handle_snapshot(phys)
    _run(kind, inp)
    assert_unchanged(before, handle_snapshot(phys))


# ---- the hand-over: trajectory_fd -> sample_rollouts (K = 1) -> kalman_smooth -> integrate_state

ENDPOINT_SPEC = [("pos", "framepos", "endpoint"), ("linvel", "framelinvel", "endpoint")]
SIGMA_Q, SIGMA_V = 1e-3, 1e-2          # the start deviation: of the size of trajectory_fd's eps, where its secants were taken


@functools.lru_cache(maxsize=None)
def _plumbing(kind):
    """8 envs at physics_support.free_states, at rest and without dry joint friction: clear of every contact (the Go2 a metre up, the
    Airbot's arm raised and its free bodies in the air), where the step is smooth and trajectory_fd's secants are the Jacobians.
    (At states in contact they are not a model of a run 1e-3 away: measured on such batches, the products of the A_t had spectral
    radii up to 240 and C_t A_{t-1} .. A_0 dx_0 missed the logged deviation by orders of magnitude from the fourth step on.)  The
    sensor table is the env's (Go2) or the endpoint's framepos / framelinvel (cube).  The log: each env's start moved by a known
    dx_0 ~ N(0, P0) with integrate_state, and sample_rollouts (K = 1) from there.  The nominal run, its sensordata and `columns` are
    taken at the unmoved start.  r is the measured mean square of what the linear model leaves out, per sensor entry; q a process
    noise of 1 % of the prior variance per step.  Computed once."""
    import torch
    from model_variants import envdef_of
    from physics_support import free_states, setup
    n, T = 8, 6
    envdef, E, phys, _, _, _ = setup(kind, n=n, seed=11, sensors=envdef_of(kind).sensors if kind == "go2flat" else ENDPOINT_SPEC,
                                     zero_floss=True)      # (dry joint friction is a kink at zero velocity, as in the FD tests)
    qf, vf, cf = free_states(envdef, kind, n, 11, zero_vel=True)      # (at rest: at 0.2 m/s the Airbot's fingers reach their stops within T)
    rng = np.random.default_rng(3)
    nv, nu = int(E.dims.nv), int(E.dims.nu)
    nx, ny = 2 * nv, phys.nsensordata
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=E.device)
    # the position servos' targets stay within 0.03 rad of where their joints are: a target drawn from the whole control range (as
    # random_states draws it) runs the servos into their force limits, a kink that no Jacobian models
    Am = envdef.sys.arrays
    at = qf[:, [int(Am["jnt_qposadr"][int(j)]) for j in np.asarray(Am["actuator_trnid"]).reshape(nu, -1)[:, 0]]]
    phys.set_state(dev(qf), dev(vf), dev(at))
    if kind == "cube":
        # the Airbot's link4 and fingers have no servo and a narrow range: from mid-range they drop onto their stops within the
        # window, a kink again.  20 control steps let them come to rest there (the free bodies are still in the air after T more)
        for _ in range(20):
            phys.step(dev(at))
    q0, v0 = phys.qpos.clone(), phys.qvel.clone()
    ctrl = (dev(at)[:, None, :] + dev(rng.normal(scale=0.01, size=(n, T, nu)))).contiguous()
    tf = phys.trajectory_fd(ctrl, nominal=True)
    y_nom = phys.sample_rollouts(ctrl[:, None].contiguous(), fields=("sensordata",))["sensordata"][:, 0]
    sig = np.concatenate([np.full(nv, SIGMA_Q), np.full(nv, SIGMA_V)])
    dx0 = dev(rng.normal(size=(n, nx)) * sig)
    q1, v1 = phys.integrate_state(q0, v0, dx0)
    phys.set_state(q1, v1)
    y_log = phys.sample_rollouts(ctrl[:, None].contiguous(), fields=("sensordata",))["sensordata"][:, 0]
    phys.set_state(q0, v0)
    dy = (y_log - y_nom).contiguous()
    host = lambda t: t.cpu().numpy()
    A, C = kalman_ref.unpack(host(tf["columns"]), nx, ny)
    # r: the log has no noise, so what the "measurement noise" stands for is what the linear model leaves out, and with dx_0 known
    # that is measured, not guessed: the mean square of dy_t - C_t A_{t-1} .. A_0 dx_0 per sensor entry (fp64, on the host)
    x, left_out = host(dx0).astype(np.float64), np.zeros((n, T, ny))
    for t in range(T):
        left_out[:, t] = host(dy)[:, t] - np.einsum("mrj,mj->mr", C[:, t].astype(np.float64), x)
        x = np.einsum("mij,mj->mi", A[:, t].astype(np.float64), x)
    r = dev(np.broadcast_to((left_out ** 2).mean((0, 1)) + 1e-12, (n, ny))).contiguous()
    qn = dev(0.01 * sig * sig).expand(n, nx).contiguous()
    P0 = torch.diag(dev(sig * sig)).expand(n, nx, nx).contiguous()
    res = phys.kalman_smooth(tf["columns"], dy, r, qn, P0, covariances=True)
    torch.cuda.synchronize()
    inp = dict(A=A, C=C, dy=host(dy), r=host(r)[:, None].repeat(T, 1), q=host(qn)[:, None].repeat(T, 1), P0=host(P0))
    refs = [kalman_ref.smooth(**inp, dtype=dt) for dt in (np.float64, np.float32)]
    return dict(kind=kind, phys=phys, n=n, T=T, nx=nx, ny=ny, nu=nu, tf=tf, dy=dy, r=r, qn=qn, P0=P0, dx0=host(dx0).astype(np.float64),
                sig=sig, res=res, refs=refs, q0=q0, v0=v0)


@pytest.mark.parametrize("kind", ["go2flat", "cube"])
def test_plumbing_columns_pass_as_they_are(kind):
    """trajectory_fd's columns, B and D rows and all, go in as they came; the device result is the fp64 recursion's on those same
    columns under the project's rule."""
    c = _plumbing(kind)
    n, T, nx, ny, nu = c["n"], c["T"], c["nx"], c["ny"], c["nu"]
    assert ny > 0 and tuple(c["tf"]["columns"].shape) == (n, T, nx + nu, nx + ny) and (ny == 6 if kind == "cube" else ny > 30)
    r64, r32 = c["refs"]
    assert (r64["status"] == -1).all() and (c["res"]["status"].cpu().numpy() == -1).all(), c["res"]["status"]
    fails = []
    for k in kalman_ref.OUTPUTS:
        rule(kind, f"plumbing {k}", rel(c["res"][k].cpu().numpy(), r64[k]), rel(r32[k], r64[k]), fails)
    # (the deviations are of the order of 1e-3: the same figures in units of the prior's standard deviations, printed only)
    sig = c["sig"]
    for k, unit in (("xf", sig), ("xs", sig), ("Pf", np.outer(sig, sig)), ("Ps", np.outer(sig, sig))):
        print(kind, f"plumbing {k} in prior sigmas: device-f64 %.2e, f32-f64 %.2e"
              % (rel(c["res"][k].cpu().numpy() / unit, r64[k] / unit).max(), rel(r32[k] / unit, r64[k] / unit).max()))
    assert not fails, fails


@pytest.mark.parametrize("kind", ["go2flat", "cube"])
def test_plumbing_the_smoothed_start_is_closer_than_the_prior(kind):
    """xs[:, 0] is closer to the true dx_0 than the prior mean (zero) is, in the P0^-1 norm, for every env: first for the fp64
    recursion on the device-made columns (else the chosen dx_0 / sensors are at fault), then for the device.  No margin.  Measured:
    DESIGN 4r."""
    import torch
    c = _plumbing(kind)
    sig, dx0 = c["sig"], c["dx0"]
    norm = lambda e: np.sqrt(((e / sig) ** 2).sum(1))
    prior = norm(dx0)
    ref = norm(c["refs"][0]["xs"][:, 0] - dx0)
    dev = norm(c["res"]["xs"][:, 0].cpu().numpy().astype(np.float64) - dx0)
    print(kind, "P0^-1 distance to the true dx_0: prior", np.round(prior, 2), "fp64 smoother", np.round(ref, 2), "device", np.round(dev, 2))
    print(kind, "ratio smoothed / prior: fp64 max %.3f mean %.3f, device max %.3f mean %.3f"
          % ((ref / prior).max(), (ref / prior).mean(), (dev / prior).max(), (dev / prior).mean()))
    assert (ref < prior).all(), ref / prior
    assert (dev < prior).all(), dev / prior
    # the smoothed start is a state set_state takes
    phys = c["phys"]
    q1, v1 = phys.integrate_state(c["q0"], c["v0"], c["res"]["xs"][:, 0])
    assert tuple(q1.shape) == tuple(c["q0"].shape) and bool(torch.isfinite(q1).all()) and bool(torch.isfinite(v1).all())
    before = phys.qpos.clone()
    phys.set_state(q1, v1)
    phys.set_state(c["q0"], c["v0"])
    torch.cuda.synchronize()
    assert torch.equal(phys.qpos, before)
