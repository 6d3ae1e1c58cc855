"""The control-limited backward pass on the device (rsr_physics_lqr_box, Physics.lqr_backward_box, box_backward_kernel of
csrc/physics/rsr_lqr.hpp) for the three operand shapes the families give: against the fp64 reference of tests/lqr_box_ref.py (the
clamped sets and codes exactly, the outputs under the project's error rule with the fp32 numpy reference's distance as the
spread); bit for bit the plain pass where no bound is reached; the layout and the slots' independence bit for bit; the failure
protocol; max_iter = 1; nothing else written; and the chain trajectory_fd -> ctrl_bounds -> lqr_backward_box -> feedback_rollouts.
The inputs are lqr_ref.inputs with lqr_box_ref.bounds, whose conditioning tests/test_lqr_box_ref.py checks on the CPU."""
import functools

import numpy as np
import pytest

import lqr_box_ref as box
import lqr_ref
from physics_support import assert_bitwise, assert_unchanged, handle_snapshot, make, rel, rule
from rsr_mjx_amd import prng
from test_lqr_gpu import FAMILIES, M, MU, SENTINEL, _handle
from test_lqr_gpu import _run as _run_plain

pytestmark = pytest.mark.gpu

NAMES = ("gain", "k", "dV", "status", "Vx", "Vxx", "clamped", "qp")


def _case(kind, T, state_reg=False, max_iter=32):
    _, _, nx, nu = _handle(kind)
    return box.case(M, T, nx, nu, 100 + T, 700 + T, mu=MU, state_reg=state_reg, max_iter=max_iter)


def _directed(kind):
    _, _, nx, nu = _handle(kind)
    b = box.BACKTRACK
    return box.case(M, b["T"], nx, nu, b["seed"], b["bseed"], mu=MU, directed=True)


def _run(kind, inp, mu=MU, state_reg=False, stride=None, fill=0.0, slots=None, values=True, report=True, max_iter=32, out=None, lo=None, hi=None):
    """Physics.lqr_backward_box on the numpy inputs `inp` (the slots `slots` of them, packed at `stride`); the outputs on the device"""
    import torch
    E, phys, nx, nu = _handle(kind)
    sl = slice(None) if slots is None else list(slots)
    dev = lambda a: torch.as_tensor(np.array(a[sl]), device=E.device)            # (a copy: the shared inputs are read-only)
    col = dev(lqr_ref.pack(inp["A"], inp["B"], stride, fill))
    mu_in = mu if np.isscalar(mu) else dev(np.asarray(mu, np.float32))
    res = phys.lqr_backward_box(col, dev(inp["lx"]), dev(inp["lu"]), dev(inp["lxx"]), dev(inp["luu"]), dev(inp["lo"] if lo is None else lo),
                                dev(inp["hi"] if hi is None else hi), lux=dev(inp["lux"]), mu=mu_in, state_reg=state_reg, values=values,
                                max_iter=max_iter, report=report, out=out)
    torch.cuda.synchronize()
    return res


def _against(kind, tag, inp, got, r64, r32, fails):
    assert (got["status"].cpu().numpy() == -1).all(), (tag, got["status"])
    cl, qp, k = got["clamped"].cpu().numpy(), got["qp"].cpu().numpy(), got["k"].cpu().numpy()
    assert (cl == r64["clamped"]).all(), (tag, np.argwhere(cl != r64["clamped"])[:5])
    assert (qp[..., 1] == r64["qp"][..., 1]).all(), (tag, np.argwhere(qp[..., 1] != r64["qp"][..., 1])[:5])
    for n in lqr_ref.OUTPUTS:
        rule(kind, f"{tag} {n}", rel(got[n].cpu().numpy(), r64[n]), rel(r32[n], r64[n]), fails)
    assert (inp["lo"] <= k).all() and (k <= inp["hi"]).all(), tag
    assert (k[cl == -1].view(np.int32) == inp["lo"][cl == -1].view(np.int32)).all(), tag
    assert (k[cl == 1].view(np.int32) == inp["hi"][cl == 1].view(np.int32)).all(), tag
    assert (got["gain"].cpu().numpy()[cl != 0] == 0).all(), tag


@pytest.mark.parametrize("state_reg", [False, True])
@pytest.mark.parametrize("kind", FAMILIES)
def test_against_fp64(kind, state_reg):
    fails = []
    for T in (1, 6) + ((64,) if kind == "cube" else ()):
        inp, r64, r32 = _case(kind, T, state_reg)
        _against(kind, f"T={T} state_reg={state_reg}", inp, _run(kind, inp, state_reg=state_reg), r64, r32, fails)
    assert not fails, fails


@pytest.mark.parametrize("kind", FAMILIES)
def test_backtracking_inputs_against_fp64(kind):
    fails = []
    inp, r64, r32 = _directed(kind)
    assert r64["census"][..., 2].sum() > 0
    _against(kind, "directed", inp, _run(kind, inp), r64, r32, fails)
    assert not fails, fails


@pytest.mark.parametrize("kind", FAMILIES)
def test_unreached_bounds_give_the_plain_pass_bitwise(kind):
    _, _, nx, nu = _handle(kind)
    for T in (1, 6):
        inp, _, _ = _case(kind, T)
        for state_reg in (False, True):
            plain = _run_plain(kind, inp, state_reg=state_reg)
            for bound in (np.inf, 1e6):
                b = np.full((M, T, nu), bound, np.float32)
                got = _run(kind, inp, state_reg=state_reg, lo=-b, hi=b)
                for n in plain:
                    assert_bitwise(f"{kind} T={T} state_reg={state_reg} bound={bound} {n}", got[n], plain[n])
                assert (got["clamped"] == 0).all() and (got["qp"][..., 0] == 1).all() and (got["qp"][..., 1] == 0).all()


@pytest.mark.parametrize("kind", FAMILIES)
def test_layout_and_independence_bitwise(kind):
    import torch
    _, _, nx, nu = _handle(kind)
    inp, _, _ = _case(kind, 6)
    base = _run(kind, inp)
    for n in NAMES:
        assert bool(torch.isfinite(base[n]).all()), n
    wide = _run(kind, inp, stride=nx + 7, fill=np.nan)                           # the entries of a row past nx are never read
    pick = [5, 0, 17]
    few = _run(kind, inp, slots=pick)                                            # a slot's result depends on that slot's inputs alone
    again = _run(kind, inp)                                                      # from run to run
    for n in NAMES:
        assert_bitwise(f"{kind} stride {n}", wide[n], base[n])
        assert_bitwise(f"{kind} slots {n}", few[n], base[n][pick])
        assert_bitwise(f"{kind} rerun {n}", again[n], base[n])
    lean = _run(kind, inp, values=False, report=False)                           # the optional outputs change nothing
    assert sorted(lean) == ["dV", "gain", "k", "status"]
    for n in lean:
        assert_bitwise(f"{kind} lean {n}", lean[n], base[n])
    assert_bitwise(f"{kind} Vxx symmetric", base["Vxx"], base["Vxx"].transpose(2, 3))


def _shapes(nx, nu, T):
    return dict(gain=(M, T, nu, nx), k=(M, T, nu), dV=(M, 2), status=(M,), Vx=(M, T + 1, nx), Vxx=(M, T + 1, nx, nx), clamped=(M, T, nu), qp=(M, T, 2))


@pytest.mark.parametrize("kind", FAMILIES)
def test_failure_stops_the_slot_alone(kind):
    """Each case takes the kernel's own early return (a refused pivot or refused bounds): none of them is a device fault."""
    import torch
    E, _, nx, nu = _handle(kind)
    T, t0, bad = 6, 2, [3, 9]
    inp, _, _ = _case(kind, T)
    rows = ("gain", "k", "Vx", "Vxx", "clamped", "qp")
    mod = {k: v.copy() for k, v in inp.items()}
    for s in bad:
        mod["luu"][s, t0] = -1e4 * np.eye(nu, dtype=np.float32)
        mod["lo"][s, t0], mod["hi"][s, t0] = -np.inf, np.inf
    # (the base run has those steps' bounds infinite too, so that the other rows compare bit for bit)
    base_in = dict(inp, lo=mod["lo"], hi=mod["hi"])
    base = _run(kind, base_in)
    shapes = _shapes(nx, nu, T)
    fresh = lambda: {k: torch.full(s, SENTINEL, device=E.device) for k, s in shapes.items()}
    got = _run(kind, mod, out=fresh())
    ok = [s for s in range(M) if s not in bad]
    status = got["status"].cpu().numpy()
    assert (status[bad] == t0).all() and (status[ok] == -1).all(), status
    assert (got["dV"][bad] == 0).all()
    for k in rows:
        assert_bitwise(f"{kind} {k} rows > t0", got[k][bad][:, t0 + 1:], base[k][bad][:, t0 + 1:])
        assert (got[k][bad][:, :t0 + 1] == SENTINEL).all(), k
    for k in shapes:
        assert_bitwise(f"{kind} {k} other slots", got[k][ok], base[k][ok])
    # a larger mu on those slots alone cures it, and every slot passes the fp64 rule
    mu = np.full(M, MU, np.float32)
    mu[bad] = 2e4
    refs = [box.backward_box(**mod, mu=mu.astype(dt), dtype=dt) for dt in (np.float64, np.float32)]
    assert (refs[0]["status"] == -1).all() and (refs[0]["clamped"] == refs[1]["clamped"]).all()
    raised = _run(kind, mod, mu=mu)
    assert (raised["status"].cpu().numpy() == -1).all()
    assert (raised["clamped"].cpu().numpy() == refs[0]["clamped"]).all()
    fails = []
    for n in lqr_ref.OUTPUTS:
        rule(kind, f"mu raised {n}", rel(raised[n].cpu().numpy(), refs[0][n]), rel(refs[1][n], refs[0][n]), fails)
    assert not fails, fails
    for k in shapes:
        assert_bitwise(f"{kind} {k} other slots, mu raised", raised[k][ok], base[k][ok])
    # a NaN in the terminal cost of one slot: that slot fails at its first step
    nan = {k: v.copy() for k, v in base_in.items()}
    nan["lxx"][12, T, 1, 2] = np.nan
    got = _run(kind, nan, out=fresh())
    status = got["status"].cpu().numpy()
    rest = [s for s in range(M) if s != 12]
    assert status[12] == T - 1 and (status[rest] == -1).all(), status
    assert (got["dV"][12] == 0).all() and all((got[k][12] == SENTINEL).all() for k in ("gain", "k", "clamped", "qp"))
    for k in shapes:
        assert_bitwise(f"{kind} {k} slots without the NaN", got[k][rest], base[k][rest])
    # bounds that are not ordered, and a NaN bound: the slot fails at that step
    for s, t, (l, h) in ((7, 4, (0.5, 0.25)), (20, 1, (np.nan, 1.0)), (21, 0, (-1.0, np.nan))):
        unordered = {k: v.copy() for k, v in base_in.items()}
        unordered["lo"][s, t, nu - 1], unordered["hi"][s, t, nu - 1] = l, h
        got = _run(kind, unordered, out=fresh())
        status = got["status"].cpu().numpy()
        rest = [r for r in range(M) if r != s]
        assert status[s] == t and (status[rest] == -1).all(), (s, t, status)
        assert (got["dV"][s] == 0).all()
        for k in rows:
            assert (got[k][s][:t + 1] == SENTINEL).all(), k
            assert_bitwise(f"{kind} {k} rows above", got[k][s][t + 1:], base[k][s][t + 1:])
        for k in shapes:
            assert_bitwise(f"{kind} {k} slots with ordered bounds", got[k][rest], base[k][rest])


@pytest.mark.parametrize("kind", FAMILIES)
def test_max_iter_one(kind):
    from test_lqr_box_ref import agreed_slots
    _, _, nx, nu = _handle(kind)
    for T in (1, 6):
        inp, r64, ok = agreed_slots(nx, nu, T)
        got = _run(kind, inp, max_iter=1)
        assert (got["status"].cpu().numpy() == -1).all()
        k, qp, cl = got["k"].cpu().numpy(), got["qp"].cpu().numpy(), got["clamped"].cpu().numpy()
        assert (inp["lo"] <= k).all() and (k <= inp["hi"]).all() and (qp[..., 0] <= 1).all()
        assert (qp[ok] == r64["qp"][ok]).all() and (cl[ok] == r64["clamped"][ok]).all()
        assert (qp[..., 1] == 2).any()


@pytest.mark.parametrize("kind", FAMILIES)
def test_nothing_else_is_written(kind):
    _, phys, _, _ = _handle(kind)
    inp, _, _ = _case(kind, 6)
    before = handle_snapshot(phys)
    _run(kind, inp, state_reg=True)
    assert_unchanged(before, handle_snapshot(phys))


@functools.lru_cache(maxsize=None)
def _plumbing():
    """The cube, 4 envs after a reset and 3 env steps: trajectory_fd about a control sequence of T = 3 that sits 1e-3 inside the
    upper limit of every limited actuator, ctrl_bounds about it, lqr_backward_box on the columns as they are, and feedback_rollouts
    with clamp=True and ctrl + alpha k for alpha in {0, 1} as the two samples.  Computed once and left unchanged."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n, T = 4, 3
    envdef, E, _, scale = make("cube", n, False)
    rng = np.random.default_rng(3)
    E.reset(prng.split(prng.PRNGKey(7), n))
    for _ in range(3):
        E.step(None, np.clip(rng.normal(size=(n, E.dims.nu)) * scale, -1, 1).astype(np.float32))
    phys = Physics(E)
    nv, nu = int(E.dims.nv), int(E.dims.nu)
    nx = 2 * nv
    A = E.sys.arrays
    lim = np.asarray(A["actuator_ctrllimited"]).reshape(nu) != 0
    rng_hi = np.asarray(A["actuator_ctrlrange"], np.float32).reshape(nu, 2)[:, 1]
    ctrl = phys.ctrl.clone()[:, None, :].repeat(1, T, 1)
    ctrl[..., torch.as_tensor(lim, device=E.device)] = torch.as_tensor(rng_hi[lim] - 1e-3, device=E.device)
    ctrl = ctrl.contiguous()
    tf = phys.trajectory_fd(ctrl, nominal=True)
    inp = lqr_ref.inputs(n, T, nx, nu, seed=21)
    cost = {k: torch.as_tensor(inp[k], device=E.device) for k in ("lx", "lu", "lxx", "luu", "lux")}
    lo, hi = phys.ctrl_bounds(ctrl)
    bw = phys.lqr_backward_box(tf["columns"], **cost, lo=lo, hi=hi, mu=MU, report=True)
    alpha = torch.tensor([0.0, 1.0], device=E.device)
    cand = (ctrl[:, None] + alpha[None, :, None, None] * bw["k"][:, None]).contiguous()
    qref, vref = tf["qpos"][:, :T].contiguous(), tf["qvel"][:, :T].contiguous()
    fb = phys.feedback_rollouts(cand, bw["gain"], qref, vref, fields=("qpos", "qvel", "ctrl"), clamp=True)
    torch.cuda.synchronize()
    return dict(E=E, lim=lim, ctrl=ctrl, tf=tf, lo=lo, hi=hi, bw=bw, cand=cand, fb=fb)


def test_plumbing_chain():
    import torch
    c = _plumbing()
    E, bw, fb, ctrl = c["E"], c["bw"], c["fb"], c["ctrl"]
    A = E.sys.arrays
    nu = int(E.dims.nu)
    assert c["lim"].any() and (bw["status"] == -1).all()
    assert c["lo"].dtype == torch.float32 and c["lo"].is_contiguous() and tuple(c["lo"].shape) == tuple(ctrl.shape)
    r = torch.as_tensor(np.asarray(A["actuator_ctrlrange"], np.float32).reshape(nu, 2), device=E.device)
    lim = torch.as_tensor(c["lim"], device=E.device)
    assert_bitwise("lo", c["lo"][..., lim], (r[:, 0] - ctrl)[..., lim])
    assert_bitwise("hi", c["hi"][..., lim], (r[:, 1] - ctrl)[..., lim])
    assert bool(torch.isinf(c["lo"][..., ~lim]).all()) and bool(torch.isinf(c["hi"][..., ~lim]).all())
    # the nominal controls sit near a limit: some control is clamped, and k stays inside the bounds
    assert bool((bw["clamped"] != 0).any()) and bool((c["lo"] <= bw["k"]).all()) and bool((bw["k"] <= c["hi"]).all())
    # alpha = 0 reproduces the nominal rows bit for bit
    assert_bitwise("alpha = 0 ctrl", fb["ctrl"][:, 0], ctrl)
    assert_bitwise("alpha = 0 qpos", fb["qpos"][:, 0], c["tf"]["qpos"][:, 1:])
    assert_bitwise("alpha = 0 qvel", fb["qvel"][:, 0], c["tf"]["qvel"][:, 1:])
    # alpha = 1, first step (the state is the nominal one: no feedback term): the applied control is u_nom + k wherever that
    # lies inside the range
    want, applied = c["cand"][:, 1, 0], fb["ctrl"][:, 1, 0]
    inside = ~lim[None, :] | ((want >= r[:, 0]) & (want <= r[:, 1]))
    assert bool(inside.any()) and bool((applied[inside] == want[inside]).all())
    assert not torch.equal(fb["ctrl"][:, 1], fb["ctrl"][:, 0])
