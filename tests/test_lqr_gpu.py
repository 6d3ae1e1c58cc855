"""The LQR backward pass on the device (rsr_physics_lqr_backward, Physics.lqr_backward, csrc/physics/rsr_lqr.hpp) for the three
operand shapes the families give (cube nx = 40, nu = 5; Go2 36, 12; T-shape 28, 5): against the fp64 recursion of tests/lqr_ref.py
under the project's error rule, with the fp32 numpy recursion's own distance from fp64 as the spread; the layout and the slots'
independence bit for bit; the failure protocol; nothing else written; and the hand-over from trajectory_fd and to feedback_rollouts.
The handle only supplies nv and nu: the inputs are lqr_ref.inputs, whose conditioning tests/test_lqr_ref.py checks on the CPU."""
import functools

import numpy as np
import pytest

import lqr_ref
from physics_support import assert_bitwise, assert_unchanged, handle_snapshot, make, rel, rule
from rsr_mjx_amd import prng

pytestmark = pytest.mark.gpu

FAMILIES = ["cube", "go2flat", "tshape"]
M, MU = 32, 1e-3
SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _handle(kind):
    """(env, Physics, nx, nu) of a 4-env batch after a reset: the call takes of it nv, nu and the device"""
    import torch
    from rsr_mjx_amd.physics import Physics
    _, E, _, _ = make(kind, 4, False)
    E.reset(prng.split(prng.PRNGKey(1), 4))
    torch.cuda.synchronize()
    return E, Physics(E), 2 * int(E.dims.nv), int(E.dims.nu)


def _case(kind, T, state_reg=False):
    _, _, nx, nu = _handle(kind)
    return lqr_ref.case(M, T, nx, nu, seed=100 + T, mu=MU, state_reg=state_reg)


def _run(kind, inp, mu=MU, state_reg=False, stride=None, fill=0.0, slots=None, lux=True, values=True, out=None):
    """Physics.lqr_backward on the numpy inputs `inp` (the slots `slots` of them, packed at `stride`); the outputs on the device"""
    import torch
    E, phys, nx, nu = _handle(kind)
    sl = slice(None) if slots is None else list(slots)
    dev = lambda a: torch.as_tensor(np.array(a[sl]), device=E.device)            # (a copy: the shared inputs are read-only)
    col = dev(lqr_ref.pack(inp["A"], inp["B"], stride, fill))
    mu_in = mu if np.isscalar(mu) else dev(np.asarray(mu, np.float32))
    res = phys.lqr_backward(col, dev(inp["lx"]), dev(inp["lu"]), dev(inp["lxx"]), dev(inp["luu"]),
                            lux=dev(inp["lux"]) if lux else None, mu=mu_in, state_reg=state_reg, values=values, out=out)
    torch.cuda.synchronize()
    return res


def _rule_all(kind, tag, got, r64, r32, fails):
    for k in lqr_ref.OUTPUTS:
        rule(kind, f"{tag} {k}", rel(got[k].cpu().numpy(), r64[k]), rel(r32[k], r64[k]), fails)


@pytest.mark.parametrize("state_reg", [False, True])
@pytest.mark.parametrize("kind", FAMILIES)
def test_against_fp64(kind, state_reg):
    fails = []
    for T in (1, 6) + ((64,) if kind == "cube" else ()):
        inp, r64, r32 = _case(kind, T, state_reg)
        got = _run(kind, inp, state_reg=state_reg)
        assert (got["status"].cpu().numpy() == -1).all(), (T, got["status"])
        _rule_all(kind, f"T={T} state_reg={state_reg}", got, r64, r32, fails)
    assert not fails, fails


@pytest.mark.parametrize("kind", FAMILIES)
def test_layout_and_independence_bitwise(kind):
    import torch
    _, _, nx, nu = _handle(kind)
    inp, _, _ = _case(kind, 6)
    base = _run(kind, inp)
    names = ("gain", "k", "dV", "status", "Vx", "Vxx")
    # the entries of a row past nx are never read
    wide = _run(kind, inp, stride=nx + 7, fill=np.nan)
    for k in names:
        assert_bitwise(f"{kind} stride {k}", wide[k], base[k])
        assert bool(torch.isfinite(base[k]).all()), k
    # a slot's result depends on that slot's inputs alone, whatever M is
    pick = [5, 0, 17]
    few = _run(kind, inp, slots=pick)
    for k in names:
        assert_bitwise(f"{kind} slots {k}", few[k], base[k][pick])
    # from run to run
    again = _run(kind, inp)
    for k in names:
        assert_bitwise(f"{kind} rerun {k}", again[k], base[k])
    # no lux is an all-zero lux
    zero = dict(inp, lux=np.zeros_like(inp["lux"]))
    with_zero, without = _run(kind, zero), _run(kind, zero, lux=False)
    assert not torch.equal(with_zero["gain"], base["gain"])
    for k in names:
        assert_bitwise(f"{kind} lux {k}", without[k], with_zero[k])
    # the optional outputs change nothing
    lean = _run(kind, inp, values=False)
    assert sorted(lean) == ["dV", "gain", "k", "status"]
    for k in lean:
        assert_bitwise(f"{kind} values {k}", lean[k], base[k])
    # Vxx is symmetric bit for bit, and its terminal row is the terminal cost
    assert_bitwise(f"{kind} Vxx symmetric", base["Vxx"], base["Vxx"].transpose(2, 3))
    assert_bitwise(f"{kind} Vxx[T]", base["Vxx"][:, 6], torch.as_tensor(np.array(inp["lxx"][:, 6]), device=base["Vxx"].device))
    assert_bitwise(f"{kind} Vx[T]", base["Vx"][:, 6], torch.as_tensor(np.array(inp["lx"][:, 6]), device=base["Vx"].device))


@pytest.mark.parametrize("kind", FAMILIES)
def test_failure_stops_the_slot_alone(kind):
    import torch
    E, _, nx, nu = _handle(kind)
    T, t0, bad = 6, 2, [3, 9]
    inp, r64, _ = _case(kind, T)
    base = _run(kind, inp)
    mod = {k: v.copy() for k, v in inp.items()}
    for s in bad:
        mod["luu"][s, t0] = -1e4 * np.eye(nu, dtype=np.float32)
        # in fp64: Quu + mu I at (s, t0) is indefinite (the steps t > t0 do not see the change)
        B = inp["B"][s, t0].astype(np.float64)
        quu = mod["luu"][s, t0].astype(np.float64) + B.T @ r64["Vxx"][s, t0 + 1] @ B + MU * np.eye(nu)
        assert np.linalg.eigvalsh(quu).min() < 0
    shapes = dict(gain=(M, T, nu, nx), k=(M, T, nu), dV=(M, 2), status=(M,), Vx=(M, T + 1, nx), Vxx=(M, T + 1, nx, nx))
    out = {k: torch.full(s, SENTINEL, device=E.device) for k, s in shapes.items()}
    got = _run(kind, mod, out=out)
    ok = [s for s in range(M) if s not in bad]
    status = got["status"].cpu().numpy()
    assert (status[bad] == t0).all() and (status[ok] == -1).all(), status
    assert (got["dV"][bad] == 0).all()
    for k in ("gain", "k", "Vx", "Vxx"):
        assert_bitwise(f"{kind} {k} rows > t0", got[k][bad][:, t0 + 1:], base[k][bad][:, t0 + 1:])
        assert (got[k][bad][:, :t0 + 1] == SENTINEL).all(), k
    for k in shapes:
        assert_bitwise(f"{kind} {k} other slots", got[k][ok], base[k][ok])
    # a larger mu on those slots alone, read on the device: they succeed, and every slot passes the fp64 rule
    mu = np.full(M, MU, np.float32)
    mu[bad] = 2e4
    refs = [lqr_ref.backward(**mod, mu=mu.astype(dt), dtype=dt) for dt in (np.float64, np.float32)]
    assert (refs[0]["status"] == -1).all()
    raised = _run(kind, mod, mu=mu)
    assert (raised["status"].cpu().numpy() == -1).all()
    fails = []
    _rule_all(kind, "mu raised", raised, refs[0], refs[1], fails)
    assert not fails, fails
    for k in shapes:
        assert_bitwise(f"{kind} {k} other slots, mu raised", raised[k][ok], base[k][ok])
    # a NaN in the terminal cost of one slot: that slot fails at its first step, the call returns, the others are untouched
    nan = {k: v.copy() for k, v in inp.items()}
    nan["lxx"][12, T, 1, 2] = np.nan
    out = {k: torch.full(s, SENTINEL, device=E.device) for k, s in shapes.items()}
    got = _run(kind, nan, out=out)
    status = got["status"].cpu().numpy()
    rest = [s for s in range(M) if s != 12]
    assert status[12] == T - 1 and (status[rest] == -1).all(), status
    assert (got["dV"][12] == 0).all() and (got["gain"][12] == SENTINEL).all() and (got["k"][12] == SENTINEL).all()
    for k in shapes:
        assert_bitwise(f"{kind} {k} slots without the NaN", got[k][rest], base[k][rest])


@pytest.mark.parametrize("kind", FAMILIES)
def test_nothing_else_is_written(kind):
    _, phys, _, _ = _handle(kind)
    inp, _, _ = _case(kind, 6)
    before = handle_snapshot(phys)
    _run(kind, inp, state_reg=True)
    assert_unchanged(before, handle_snapshot(phys))


@functools.lru_cache(maxsize=None)
def _plumbing():
    """The Go2 on flat ground, 4 envs after a reset and 3 env steps, its sensor table set (nsd > 0): trajectory_fd about a noisy
    control sequence of T = 3, lqr_backward on its columns as they are, and feedback_rollouts with ctrl + alpha k for alpha in
    {0, 0.5} as the two samples, the gain shared and the nominal rows as the reference.  Computed once and left unchanged."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n, T = 4, 3
    envdef, E, _, scale = make("go2flat", n, False)
    rng = np.random.default_rng(3)
    E.reset(prng.split(prng.PRNGKey(7), n))
    for _ in range(3):
        E.step(None, np.clip(rng.normal(size=(n, E.dims.nu)) * scale, -1, 1).astype(np.float32))
    phys = Physics(E, sensors=envdef.sensors)
    nv, nu = int(E.dims.nv), int(E.dims.nu)
    nx = 2 * nv
    ctrl = (phys.ctrl.clone()[:, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(n, T, nu)).astype(np.float32), device=E.device)).contiguous()
    tf = phys.trajectory_fd(ctrl, nominal=True)
    inp = lqr_ref.inputs(n, T, nx, nu, seed=21)
    cost = {k: torch.as_tensor(inp[k], device=E.device) for k in ("lx", "lu", "lxx", "luu", "lux")}
    as_is = phys.lqr_backward(tf["columns"], **cost, mu=MU)
    alpha = torch.tensor([0.0, 0.5], device=E.device)
    cand = (ctrl[:, None] + alpha[None, :, None, None] * as_is["k"][:, None]).contiguous()
    qref, vref = tf["qpos"][:, :T].contiguous(), tf["qvel"][:, :T].contiguous()
    fb = phys.feedback_rollouts(cand, as_is["gain"], qref, vref, fields=("qpos", "qvel", "ctrl"))
    torch.cuda.synchronize()
    return dict(E=E, phys=phys, n=n, T=T, nx=nx, nu=nu, ctrl=ctrl, tf=tf, cost=cost, as_is=as_is, cand=cand, qref=qref, vref=vref, fb=fb)


def test_plumbing_columns_pass_as_they_are():
    """trajectory_fd's columns, sensor entries and all, give bit for bit what contiguous copies of its A and B packed tight give, and
    the gain goes into feedback_rollouts unchanged.  No assertion on a cost decrease: contact makes the step piecewise smooth."""
    import torch
    c = _plumbing()
    n, T, nx, nu, tf, phys = c["n"], c["T"], c["nx"], c["nu"], c["tf"], c["phys"]
    nsd = phys.nsensordata
    assert nsd > 0 and tuple(tf["columns"].shape) == (n, T, nx + nu, nx + nsd)
    a, b = tf["A"].contiguous(), tf["B"].contiguous()
    tight = torch.cat([a.transpose(2, 3), b.transpose(2, 3)], dim=2).contiguous()
    assert tuple(tight.shape) == (n, T, nx + nu, nx)
    packed = phys.lqr_backward(tight, **c["cost"], mu=MU)
    torch.cuda.synchronize()
    assert (c["as_is"]["status"] == -1).all()
    for k in c["as_is"]:
        assert_bitwise(f"plumbing {k}", c["as_is"][k], packed[k])
    assert tuple(c["as_is"]["gain"].shape) == (n, T, nu, nx)
    assert tuple(c["fb"]["qpos"].shape) == (n, 2, T, int(c["E"].dims.nq)) and bool(torch.isfinite(c["fb"]["qpos"]).all())
    # the two candidates differ
    assert not torch.equal(c["fb"]["ctrl"][:, 0], c["fb"]["ctrl"][:, 1])


def test_plumbing_alpha_zero_reproduces_the_nominal_trajectory():
    """The alpha = 0 sample against the nominal rows, bit for bit, under the gain the backward pass returned (up to 140 here): at the
    nominal state every feedback term is a zero, the free joint's rotation included (its difference at equal quaternions is 0, not
    the rounding residue of conj(q) q: feedback_ctrl asks differentiate_pos for that), so the sample applies the nominal ctrl and
    stays on the nominal trajectory.  The alpha = 0.5 sample leaves it."""
    import torch
    c = _plumbing()
    assert float(c["as_is"]["gain"][..., 3:6].abs().max()) > 1.0                # (the rotation columns are not idle)
    assert_bitwise("alpha = 0 ctrl", c["fb"]["ctrl"][:, 0], c["ctrl"])
    assert_bitwise("alpha = 0 qpos", c["fb"]["qpos"][:, 0], c["tf"]["qpos"][:, 1:])
    assert_bitwise("alpha = 0 qvel", c["fb"]["qvel"][:, 0], c["tf"]["qvel"][:, 1:])
    assert not torch.equal(c["fb"]["qpos"][:, 1], c["tf"]["qpos"][:, 1:])
