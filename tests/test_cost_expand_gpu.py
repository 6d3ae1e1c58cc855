"""The cost expansion on the device (rsr_physics_cost_expand, Physics.cost_expand, csrc/physics/rsr_expand.hpp) for the three
operand shapes the families give (cube nx = 40, nu = 5; Go2 36, 12; T-shape 28, 5): against the float64 expansion of
tests/cost_expand_ref.py under the project's error rule, with the float32 numpy expansion's own distance from float64 as the spread;
the header's two exactness guarantees, the layout and the problems' independence bit for bit; nothing else written; the refusals;
and the chain cost_rollouts -> trajectory_fd -> cost_expand -> lqr_backward on a batch.  The handle only supplies nv and nu: the
inputs are cost_expand_ref.inputs, whose expansion tests/test_cost_expand_ref.py checks against the cost on the CPU.

Shapes: M = 8 problems; T in {1, 5} (T = 1: index 0 and index T are the only rows); ny in {1, 7, 64} (one lane, a partial wave,
RSR_MAX_SENSORDATA); the column rows tight and 5 floats wider.

The chain's measured gap.  The first-order change of the cost along a seeded du, predicted from the float64 reference expansion on
the device's columns, is compared with the central difference of cost_rollouts' cost between u_nom +- H du.  The gap between the two
is a finite-difference and piecewise-smoothness error (the columns' own step, the difference's step H, the cost's fp32 rounding
over 2 H), not the expansion's rounding; it was measured per family on the device's trajectories at the states, seed and H below
(the largest of the envs counted: 4.5e-2 on the cube, 8.9e-3 on the Go2) and is recorded in tests/golden/cost_expand_tolerances.json;
the test allows 3 x the recorded value.  An env in which a contact or a joint-limit row is active in one of the nominal run and the
two samples and not in another is skipped and counted, at most one of the four.  At the recorded seed none is on the Go2; on the
cube the arm, driven towards controls drawn from the whole range, meets joint limits within the four steps, with the same rows
active in all three runs of three envs and not in the fourth, which is skipped."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import cost_expand_ref as R
from physics_support import assert_bitwise, assert_unchanged, bits, free_states, handle_snapshot, make, rel, rule, sensor_spec
from rsr_mjx_amd import prng

pytestmark = pytest.mark.gpu

FAMILIES = ["cube", "go2flat", "tshape"]
M = 8
SENTINEL = 12345.0
GRID = [(T, ny, wide) for T in (1, 5) for ny in (1, 7, 64) for wide in (False, True)]
REFS = ("ctrl_ref", "sensor_ref")
CHAIN_T, CHAIN_H, CHAIN_SEED = 4, 1e-3, 31
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cost_expand_tolerances.json")


@functools.lru_cache(maxsize=None)
def _handle(kind):
    """(env, Physics, nv, nu) of a 4-env batch after a reset: the call takes of it nv, nu and the device"""
    import torch
    from rsr_mjx_amd.physics import Physics
    _, E, _, _ = make(kind, 4, False)
    E.reset(prng.split(prng.PRNGKey(1), 4))
    torch.cuda.synchronize()
    return E, Physics(E), int(E.dims.nv), int(E.dims.nu)


@functools.lru_cache(maxsize=None)
def _case(kind, T, ny, wide=False):
    """(inputs, float64 and float32 reference of every term on), computed once and read-only"""
    _, _, nv, nu = _handle(kind)
    inp = R.inputs(M, T, nv, nu, ny, seed=1000 + 10 * T + ny, stride=2 * nv + ny + (5 if wide else 0))
    return inp, R.expand(inp, np.float64), R.expand(inp, np.float32)


def _run(kind, inp, terms=R.TERMS, refs=REFS, slots=None, out=None):
    """Physics.cost_expand on the numpy inputs `inp` (the slots `slots` of them), with the weights `terms` and the references
    `refs` given and only the inputs those terms need; the outputs on the device"""
    import torch
    E, phys, _, _ = _handle(kind)
    sl = slice(None) if slots is None else list(slots)
    dev = lambda k: torch.as_tensor(np.array(inp[k][sl]), device=E.device)          # (a copy: the shared inputs are read-only)
    cost = {k: dev(k) for k in terms + tuple(refs)}
    kw = {}
    if {"w_qpos", "w_qvel"} & set(terms):
        kw["dx"] = dev("dx")
    if "w_ctrl" in terms:
        kw["ctrl"] = dev("ctrl")
    if "w_sensor" in terms:
        kw.update(sensordata=dev("sensordata"), columns=dev("columns"))
    res = phys.cost_expand(cost, out=out, **kw)
    torch.cuda.synchronize()
    return res


def _rule_all(kind, tag, got, r64, r32, fails):
    for k in R.OUTPUTS:
        rule(kind, f"{tag} {k}", rel(got[k].cpu().numpy(), r64[k]), rel(r32[k], r64[k]), fails)


@pytest.mark.parametrize("kind", FAMILIES)
def test_against_fp64(kind):
    fails = []
    for T, ny, wide in GRID:                                          # every term on, over the whole grid of shapes
        inp, r64, r32 = _case(kind, T, ny, wide)
        _rule_all(kind, f"T={T} ny={ny} wide={wide} all", _run(kind, inp), r64, r32, fails)
    for T in (1, 5):                                                   # each term alone, and the references absent
        inp, _, _ = _case(kind, T, 7, True)
        for terms, refs in [((w,), REFS) for w in R.TERMS] + [(R.TERMS, ()), (R.TERMS, ("ctrl_ref",)), (R.TERMS, ("sensor_ref",))]:
            r64, r32 = R.expand(inp, np.float64, terms, refs), R.expand(inp, np.float32, terms, refs)
            _rule_all(kind, f"T={T} {'+'.join(terms)} refs={refs}", _run(kind, inp, terms, refs), r64, r32, fails)
    assert not fails, fails


@pytest.mark.parametrize("kind", FAMILIES)
def test_exact_with_the_sensor_term_off(kind):
    """Guarantee 1 of the header, against fp32 torch products formed on the device."""
    import torch
    E, _, nv, nu = _handle(kind)
    for T in (1, 5):
        inp, _, _ = _case(kind, T, 7)
        dev = lambda k: torch.as_tensor(np.array(inp[k]), device=E.device)
        w = torch.cat([dev("w_qpos"), dev("w_qvel")], dim=2)
        for refs in (REFS, ()):
            got = _run(kind, inp, ("w_qpos", "w_qvel", "w_ctrl"), refs)
            assert_bitwise(f"{kind} lx[t+1]", got["lx"][:, 1:], w * dev("dx"))
            du = dev("ctrl") - dev("ctrl_ref") if refs else dev("ctrl")
            assert_bitwise(f"{kind} lu", got["lu"], dev("w_ctrl") * du)
            assert_bitwise(f"{kind} lxx[t+1]", got["lxx"][:, 1:], torch.diag_embed(w))
            assert_bitwise(f"{kind} luu", got["luu"], torch.diag_embed(dev("w_ctrl")))
            for k, t in (("lux", got["lux"]), ("lx[0]", got["lx"][:, 0]), ("lxx[0]", got["lxx"][:, 0])):
                assert not bool(bits(t).any()), (kind, k)              # exactly +0
        # one state weight alone: the other half is exactly +0 and its diagonal too
        got = _run(kind, inp, ("w_qvel",), ())
        assert not bool(bits(got["lx"][:, :, :nv]).any()) and not bool(bits(got["lxx"][:, :, :nv]).any()) and not bool(bits(got["lu"]).any())
        assert_bitwise(f"{kind} w_qvel alone", got["lx"][:, 1:, nv:], dev("w_qvel") * dev("dx")[..., nv:])


@pytest.mark.parametrize("kind", FAMILIES)
def test_symmetric_bit_for_bit(kind):
    """Guarantee 2 of the header, with the sensor term on."""
    import torch
    for T, ny in ((5, 64), (5, 7), (1, 1)):
        got = _run(kind, _case(kind, T, ny)[0])
        for k in ("lxx", "luu"):
            assert_bitwise(f"{kind} {k} symmetric", got[k], got[k].transpose(2, 3))
            assert bool(torch.isfinite(got[k]).all()), k


@pytest.mark.parametrize("kind", FAMILIES)
def test_layout_and_independence_bitwise(kind):
    import torch
    E, _, nv, nu = _handle(kind)
    T, ny = 5, 7
    nx = 2 * nv
    inp, _, _ = _case(kind, T, ny)
    base = _run(kind, inp)
    for k in R.OUTPUTS:
        assert bool(torch.isfinite(base[k]).all()), k                 # (the NaN around the sensor slice was never read)
    # a wider row with NaN padding; other values below nx
    for other in (R.repack(inp, nx + ny + 5), R.repack(inp, nx + ny, below=0.0), R.repack(inp, nx + ny + 1, fill=7.0, below=-3.0)):
        got = _run(kind, other)
        for k in R.OUTPUTS:
            assert_bitwise(f"{kind} layout {k}", got[k], base[k])
    # a problem's result depends on its own inputs alone, whatever M is and wherever it stands
    pick = [5, 0, 3]
    few = _run(kind, inp, slots=pick)
    for k in R.OUTPUTS:
        assert_bitwise(f"{kind} slots {k}", few[k], base[k][pick])
    # from run to run
    again = _run(kind, inp)
    for k in R.OUTPUTS:
        assert_bitwise(f"{kind} rerun {k}", again[k], base[k])
    # out= is filled in place, and in full: no sentinel is left, with every term on and with one alone
    shapes = dict(lx=(M, T + 1, nx), lu=(M, T, nu), lxx=(M, T + 1, nx, nx), luu=(M, T, nu, nu), lux=(M, T, nu, nx))
    for terms in (R.TERMS, ("w_qvel",), ("w_sensor",)):
        out = {k: torch.full(s, SENTINEL, device=E.device) for k, s in shapes.items()}
        got = _run(kind, inp, terms, out=out)
        for k in R.OUTPUTS:
            assert got[k] is out[k] and not bool((out[k] == SENTINEL).any()), (terms, k)
        if terms == R.TERMS:
            for k in R.OUTPUTS:
                assert_bitwise(f"{kind} out= {k}", out[k], base[k])


@pytest.mark.parametrize("kind", FAMILIES)
def test_nothing_else_is_written(kind):
    _, phys, _, _ = _handle(kind)
    inp, _, _ = _case(kind, 5, 64, True)
    before = handle_snapshot(phys)
    _run(kind, inp)
    assert_unchanged(before, handle_snapshot(phys))


@pytest.mark.parametrize("kind", FAMILIES)
def test_refusals(kind):
    """Every RSR_ERR_ARG case of the header: the wrapper raises ValueError ahead of the C call, and the C entry itself, on the
    real handle, returns RSR_ERR_ARG; neither the handle's buffers nor the outputs are touched."""
    import torch
    from rsr_mjx_amd import _lib
    E, phys, nv, nu = _handle(kind)
    T, ny = 5, 7
    nx, ncol = 2 * nv, 2 * nv + nu
    inp, _, _ = _case(kind, T, ny)
    dev = lambda k: torch.as_tensor(np.array(inp[k]), device=E.device)
    t = {k: dev(k) for k in inp}
    cost = {k: t[k] for k in R.TERMS + REFS}
    good = dict(cost=cost, dx=t["dx"], ctrl=t["ctrl"], sensordata=t["sensordata"], columns=t["columns"])
    shapes = dict(lx=(M, T + 1, nx), lu=(M, T, nu), lxx=(M, T + 1, nx, nx), luu=(M, T, nu, nu), lux=(M, T, nu, nx))
    out = {k: torch.full(s, SENTINEL, device=E.device) for k, s in shapes.items()}
    before = handle_snapshot(phys)
    z = lambda *s: torch.zeros(s, device=E.device)
    huge = z(1, 1, nv).expand(2 ** 30, 1, nv)                          # M (T + 1) = 2^31, no memory behind it
    cases = [(dict(good, cost={k: v for k, v in cost.items() if k in REFS}), "cost gives no weight"),
             (dict(good, cost=None), "cost must be a dict"),
             (dict(good, cost=dict(cost, w_time=t["w_qvel"])), r"cost has \['w_time'\]"),
             (dict(good, dx=None), "expects dx"),
             (dict(good, ctrl=None), "expects ctrl"),
             (dict(good, sensordata=None), "expects sensordata"),
             (dict(good, columns=None), "expects columns"),
             (dict(good, cost=dict(cost, w_sensor=z(M, T, 0))), r"cost\['w_sensor'\]"),              # ny == 0 with w_sensor
             (dict(good, cost=dict(cost, w_sensor=z(M, T, 65))), r"cost\['w_sensor'\]"),             # ny above the cap
             (dict(good, columns=t["columns"][..., :nx + ny - 1].contiguous()), "expects columns"),   # row_stride < nx + ny
             (dict(good, cost=dict(w_qvel=z(0, T, nv))), r"cost\['w_qvel'\]"),                        # M < 1
             (dict(good, cost=dict(w_qvel=z(M, 0, nv))), r"cost\['w_qvel'\]"),                        # T < 1
             (dict(good, cost=dict(w_qvel=huge)), "below 2\\^31"),
             (dict(good, out=dict(out, lxx=None, Vxx=out["lxx"])), r"out has \['Vxx'\]"),
             (dict(good, out=dict(out, lux=z(M, T, nx, nu))), r"out\['lux'\]")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            phys.cost_expand(**{"out": out, **kw})
    # the C entry on the real handle
    fn = _lib.lib().rsr_physics_cost_expand
    p = lambda x: None if x is None else x.data_ptr()

    def call(M_=M, T_=T, columns=t["columns"], stride=nx + ny, ny_=ny, cs="good", nom="good", o="good"):
        c = _lib.Cost(**{k: p(v) for k, v in (cost if cs == "good" else cs).items()}) if cs is not None else None
        n = _lib.CostNominal(**{k: p(v) for k, v in (dict(dx=t["dx"], ctrl=t["ctrl"], sensordata=t["sensordata"]) if nom == "good" else nom).items()}) \
            if nom is not None else None
        e = _lib.CostExpansion(**{k: p(v) for k, v in (out if o == "good" else o).items()}) if o is not None else None
        ref = lambda s: None if s is None else C.byref(s)
        return fn(phys._h, M_, T_, None if columns is None else C.c_void_p(columns.data_ptr()), stride, ny_, ref(c), ref(n), ref(e), phys._stream())
    nom_all = dict(dx=t["dx"], ctrl=t["ctrl"], sensordata=t["sensordata"])
    bad = [dict(cs=None), dict(nom=None), dict(o=None)] + [dict(o=dict(out, **{k: None})) for k in R.OUTPUTS] + \
        [dict(M_=0), dict(T_=0), dict(ny_=-1), dict(ny_=65, stride=nx + 65), dict(cs={k: cost[k] for k in REFS}),
         dict(nom=dict(nom_all, dx=None)), dict(cs=dict(w_qvel=cost["w_qvel"]), nom=dict(nom_all, dx=None)), dict(nom=dict(nom_all, ctrl=None)),
         dict(ny_=0), dict(nom=dict(nom_all, sensordata=None)), dict(columns=None), dict(stride=nx + ny - 1), dict(M_=2 ** 30, T_=1)]
    for kw in bad:
        assert call(**kw) == -1 and b"rsr_physics_cost_expand: " in _lib.lib().rsr_last_error(), kw
    assert fn(None, M, T, None, 0, 0, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert_unchanged(before, handle_snapshot(phys))
    for k in R.OUTPUTS:
        assert bool((out[k] == SENTINEL).all()), k
    # and the good call goes through, by both ways
    assert call() == 0
    torch.cuda.synchronize()
    base = _run(kind, inp)
    for k in R.OUTPUTS:
        assert_bitwise(f"{kind} C call {k}", out[k], base[k])


# ---- the chain

@functools.lru_cache(maxsize=None)
def _chain(kind):
    """_chain_build at the recorded step and seed, computed once and left unchanged"""
    return _chain_build(kind, CHAIN_H, CHAIN_SEED)


def _chain_build(kind, h, seed):
    """4 envs that start clear of every contact and joint limit (free_states) with the joints' friction loss zeroed through the
    per-env leaf, the family's sensor table set, T = 4: the nominal run's residuals from cost_rollouts, the columns from
    trajectory_fd, the expansion, the backward pass, and the cost of u_nom +- h du as two samples, with the ncon and qpos rows by
    which test_chain sees a contact or a limit row change activity.  (With the friction loss on, the stick / slip switch of its
    rows made the measured difference jump by its own size from one h to the next; with it off, h = 1e-3 and h = 3e-4 measured the
    same change to 1e-3 of it in every env at this seed.)"""
    import torch
    from rsr_mjx_amd.physics import Physics
    n, T = 4, CHAIN_T
    envdef, E, _, _ = make(kind, n, False)
    E.set_randomization({"dof_frictionloss": np.zeros((n, E.dims.nv), np.float32)})
    E.reset(prng.split(prng.PRNGKey(1), n))
    phys = Physics(E, sensors=sensor_spec(kind, envdef))
    qpos, qvel, ctrl = free_states(envdef, kind, n, seed)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=E.device)
    phys.set_state(dev(qpos), dev(qvel), dev(ctrl))
    nv, nu, nq, nsd = int(E.dims.nv), int(E.dims.nu), int(E.dims.nq), phys.nsensordata
    rng = np.random.default_rng(seed)
    u_nom = dev(ctrl[:, None, :] + rng.normal(scale=0.02, size=(n, T, nu)))
    cost = dict(w_qpos=dev(rng.uniform(0.0, 2.0, size=(n, T, nv))), w_qvel=dev(rng.uniform(0.0, 0.2, size=(n, T, nv))),
                w_ctrl=dev(rng.uniform(0.5, 2.0, size=(n, T, nu))), w_sensor=dev(rng.uniform(0.0, 0.5, size=(n, T, nsd))),
                qpos_ref=dev(np.repeat(qpos[:, None], T, 1)), ctrl_ref=dev(ctrl[:, None, :] + rng.normal(scale=0.1, size=(n, T, nu))))
    du = rng.normal(size=(n, T, nu))
    nom = phys.cost_rollouts(u_nom[:, None].contiguous(), cost, residual=True, fields=("ctrl", "sensordata", "ncon", "qpos"))
    fd = phys.trajectory_fd(u_nom)
    src = dict(dx=nom["dx"][:, 0].contiguous(), ctrl=nom["ctrl"][:, 0].contiguous(), sensordata=nom["sensordata"][:, 0].contiguous())
    ex = phys.cost_expand(cost, columns=fd["columns"], **src)
    lq = phys.lqr_backward(fd["columns"], **ex, mu=1e-3)
    pm = torch.stack([u_nom + h * dev(du), u_nom - h * dev(du)], dim=1).contiguous()
    two = phys.cost_rollouts(pm, cost, fields=("ncon", "qpos"))
    torch.cuda.synchronize()
    return dict(h=h, A=envdef.sys.arrays, E=E, phys=phys, n=n, T=T, nv=nv, nu=nu, nsd=nsd, cost=cost, src=src, nom=nom, fd=fd, ex=ex, lq=lq, two=two, du=du)


def _prediction(c, e):
    """sum_t lu_t . du_t + lx_t . dx_t per env in float64, dx_0 = 0 and dx_{t+1} = A_t dx_t + B_t du_t on the device's columns"""
    A, B = c["fd"]["A"].cpu().numpy().astype(np.float64), c["fd"]["B"].cpu().numpy().astype(np.float64)
    lx, lu = np.asarray(e["lx"], np.float64), np.asarray(e["lu"], np.float64)
    x = np.zeros((c["n"], 2 * c["nv"]))
    pred = np.zeros(c["n"])
    for t in range(c["T"]):
        pred += (lu[:, t] * c["du"][:, t]).sum(1) + (lx[:, t] * x).sum(1)
        x = np.einsum("eij,ej->ei", A[:, t], x) + np.einsum("eij,ej->ei", B[:, t], c["du"][:, t])
    return pred + (lx[:, c["T"]] * x).sum(1)


@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_chain(kind):
    c = _chain(kind)
    n, T, nv, nu, nsd = c["n"], c["T"], c["nv"], c["nu"], c["nsd"]
    assert nsd > 0 and tuple(c["fd"]["columns"].shape) == (n, T, 2 * nv + nu, 2 * nv + nsd)
    assert (c["lq"]["status"].cpu().numpy() == -1).all(), c["lq"]["status"]
    assert (c["lq"]["dV"][:, 0].cpu().numpy() <= 0).all(), c["lq"]["dV"]
    # the expansion on the batch's own inputs, against the references on the same inputs
    inp = {k: v.cpu().numpy() for k, v in {**c["cost"], **c["src"]}.items() if k != "qpos_ref"}
    inp["columns"] = c["fd"]["columns"].cpu().numpy()
    r64, r32 = R.expand(inp, np.float64, refs=("ctrl_ref",)), R.expand(inp, np.float32, refs=("ctrl_ref",))
    fails = []
    _rule_all(kind, "chain", c["ex"], r64, r32, fails)
    # the predicted first-order cost change along du: the device's expansion against the float64 reference's
    got = _prediction(c, {k: v.cpu().numpy() for k, v in c["ex"].items()})
    p64, p32 = _prediction(c, r64), _prediction(c, r32)
    rule(kind, "prediction", rel(got[:, None], p64[:, None]), rel(p32[:, None], p64[:, None]), fails)
    assert not fails, fails
    # ... and against the measured change of cost_rollouts' cost between u_nom +- H du
    cost = c["two"]["cost"].cpu().numpy().astype(np.float64)
    measured = (cost[:, 0] - cost[:, 1]) / (2 * c["h"])
    # a sample in which a contact or a joint-limit row is active in one of the three runs (the nominal, +H, -H) and not in
    # another is skipped and counted.  Contacts: the ncon rows.  Limits: a limited joint at or beyond an end of its range in a
    # recorded state (the end of every control step; the substeps between are not recorded)
    ncon, ncon0 = c["two"]["ncon"].cpu().numpy(), c["nom"]["ncon"].cpu().numpy()[:, 0]
    flipped = (ncon[:, 0] != ncon[:, 1]).any((1, 2)) | (ncon[:, 0] != ncon0).any((1, 2))
    A = c["A"]
    lim = [j for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) in (2, 3) and A["jnt_limited"][j]]
    qa, lo, hi = A["jnt_qposadr"][lim], A["jnt_range"][lim, 0].astype(np.float32), A["jnt_range"][lim, 1].astype(np.float32)
    q = np.concatenate([c["nom"]["qpos"].cpu().numpy(), c["two"]["qpos"].cpu().numpy()], 1)[..., qa]       # [n, 3, T, limited joints]
    active = np.stack([q <= lo, q >= hi], -1)
    assert len(lim) > 0
    flipped |= (active != active[:, :1]).any((1, 2, 3, 4))
    nearest = np.minimum(q - lo, hi - q).min((1, 2, 3))
    print(kind, "limit rows active", int(active.sum()), "nearest approach to a limit per env", nearest)
    assert flipped.sum() <= 1, flipped
    gap = np.abs(measured - p64)[~flipped] / np.abs(p64)[~flipped]
    recorded = json.load(open(GOLDEN))[kind]
    print(kind, "predicted", p64, "measured", measured, "relative gap", gap, "skipped", int(flipped.sum()), "recorded", recorded["gap"])
    assert (recorded["T"], recorded["h"], recorded["seed"]) == (CHAIN_T, CHAIN_H, CHAIN_SEED)
    assert gap.max() <= 3.0 * recorded["gap"], (gap, recorded)
