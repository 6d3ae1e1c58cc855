"""Physics.transition_fd (rsr_physics_transition_fd, csrc/physics/rsr_transition.hpp): finite differences of Physics.step in the
tangent space of (qpos, qvel), MuJoCo's mjd_transitionFD.  The call is specified as "the differences of the step at the given eps",
so the tests take it apart: every perturbed run is the stepper's bit for bit, the perturbations are mj_integratePos's, the columns
are mj_differentiatePos of the runs' end states, and at the same eps the columns agree with the CPU oracle's own finite differences
as closely as the project's rule for a dynamic field asks (tests/physics_support.py)."""
import numpy as np
import pytest

from physics_support import FAMILIES, PIPE, all_but, assert_unchanged, bits, free_states, handle_snapshot, handle_views, make, rel, rule
from rsr_mjx_amd import prng
from tangent_ref import columns, differentiate_pos, integrate_pos

N = 64
EPS = 1e-3
U = 2.0 ** -24
# (family, DR on, applied forces on, centred, nsteps or None = n_substeps)
CONFIGS = [(k, False, False, True, None) for k in FAMILIES] + [
    ("cube", True, False, True, None), ("go2flat", True, False, True, None), ("go2flat", False, True, True, None),
    ("cube", False, False, False, None), ("go2flat", False, False, True, 1)]
_ID = lambda c: "%s%s%s%s%s" % (c[0], "-dr" if c[1] else "", "-applied" if c[2] else "", "" if c[3] else "-forward",
                                "" if c[4] is None else "-nsteps%d" % c[4])
_RUNS = {}


def _stepped(kind, n, dr_on, seed=7):
    """(envdef, env batch) after a reset and 3 env steps: Go2 feet and Airbot fingers in contact"""
    envdef, E, _, scale = make(kind, n, dr_on)
    rng = np.random.default_rng(3)
    E.reset(prng.split(prng.PRNGKey(seed), n))
    for _ in range(3):
        E.step(None, np.clip(rng.normal(size=(n, E.dims.nu)) * scale, -1, 1).astype(np.float32))
    return envdef, E


def _run(cfg):
    """transition_fd with keep_states on one config, then the replay of every run through Physics.step (computed once per config):
    the record, fd_x, fd_y, the column buffer, each run's sensordata, and the count of runs whose replay differs bitwise."""
    if cfg in _RUNS:
        return _RUNS[cfg]
    import torch
    from rsr_mjx_amd.physics import Physics
    kind, dr_on, applied, centered, nsteps = cfg
    envdef, E = _stepped(kind, N, dr_on)
    phys = Physics(E, sensors=envdef.sensors if kind.startswith("go2") else None)
    d = E.dims
    nq, nv, nu, ncol = d.nq, d.nv, d.nu, 2 * d.nv + d.nu
    if applied:
        rng = np.random.default_rng(5)
        phys.set_applied(xfrc=rng.normal(scale=2.0, size=(N, d.nbody, 6)).astype(np.float32),
                         qfrc=rng.normal(scale=0.5, size=(N, nv)).astype(np.float32))
    nsd = phys.nsensordata
    ns = phys.n_substeps if nsteps is None else nsteps
    phys.transition_fd(nsteps=nsteps, eps=EPS, centered=centered, keep_states=True)
    torch.cuda.synchronize()
    saved = {k: E.view(k).clone() for k in PIPE}
    x, y = phys.fd_x.clone(), phys.fd_y.clone()
    assert x.shape == (N, ncol, 2, nq + nv + nu) and y.shape == (N, ncol, 2, nq + nv)
    for k in PIPE:                                                 # the call left the record alone
        assert torch.equal(bits(E.view(k)), bits(saved[k])), k
    bad = torch.zeros((), dtype=torch.int64, device=x.device)
    sd = torch.zeros((N, ncol, 2, nsd), device=x.device)
    for c in range(ncol):
        for sg in range(2):
            for k in PIPE:                                          # restore the record, the warm start as saved
                E.view(k).copy_(saved[k])
            phys.qpos.copy_(x[:, c, sg, :nq])
            phys.qvel.copy_(x[:, c, sg, nq:nq + nv])
            phys.step(x[:, c, sg, nq + nv:].contiguous(), ns)
            bad += (bits(phys.qpos) != bits(y[:, c, sg, :nq])).any().long() + (bits(phys.qvel) != bits(y[:, c, sg, nq:])).any().long()
            if nsd:
                sd[:, c, sg] = phys.sensordata
    ncon = phys.contacts()["ncon"].cpu().numpy()                    # of the last replayed run's last pass
    for k in PIPE:
        E.view(k).copy_(saved[k])
    torch.cuda.synchronize()
    raw = phys._fetch("rsr_physics_transition_view", 0)
    out = dict(cfg=cfg, ncon=ncon, dims=(nq, nv, nu, ncol, nsd), A=envdef.sys.arrays, bad=int(bad), x=x.cpu().numpy(), y=y.cpu().numpy(),
               sd=sd.cpu().numpy().astype(np.float64), cols=raw.cpu().numpy().reshape(N, ncol, -1),
               rec=np.concatenate([saved[k].cpu().numpy() for k in ("qpos", "qvel", "ctrl")], 1),
               blocks={b: getattr(phys, "fd_" + b).cpu().numpy() for b in "ABCD"})
    _RUNS[cfg] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_the_runs_are_the_steppers_bit_for_bit(cfg):
    """Every column's two runs, replayed: record restored, fd_x's qpos / qvel written into it (the warm start as saved),
    Physics.step(fd_x's ctrl, nsteps) must land on fd_y bit for bit.  All five families, with DR, with applied forces, not
    centred (the second run is the unperturbed state) and with nsteps = 1."""
    r = _run(cfg)
    assert r["bad"] == 0, f"{_ID(cfg)}: {r['bad']} of {2 * r['dims'][3]} replayed runs differ from fd_y"
    assert np.isfinite(r["y"]).all() and np.abs(r["y"]).max() > 0
    assert (r["ncon"] > 0).mean() > 0.5, f"{_ID(cfg)}: the runs do not exercise the contact path ({(r['ncon'] > 0).sum()} of {N} envs in contact)"
    if not cfg[3]:                                                 # not centred: run 1 starts from the record itself
        nq, nv, nu, ncol, _ = r["dims"]
        assert (r["x"][:, :, 1].view(np.int32) == r["rec"][:, None].view(np.int32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[2], CONFIGS[4]], ids=_ID)
def test_the_perturbations_are_the_tangent_space_ones(cfg):
    """fd_x against a numpy restatement of mj_integratePos: the moved coordinate is the fp32 sum bit for bit (hinge / slide,
    free-joint translation, qvel, ctrl); a rotated quaternion is within 4 * 2^-24 of the fp64 formula per component and unit to
    4 * 2^-24; every other entry is the record's, bitwise."""
    r = _run(cfg)
    nq, nv, nu, ncol, _ = r["dims"]
    rec, x = r["rec"], r["x"]
    cols = columns(r["A"], nv)
    nrot = 0
    for c in range(ncol):
        for sg, dlt in ((0, np.float32(EPS)), (1, np.float32(-EPS))):
            exp = rec.copy()
            own = np.zeros(rec.shape[1], bool)
            if c < nv and cols[c][0] == "rot":
                qa = cols[c][1]
                own[qa:qa + 4] = True
                ref = integrate_pos(r["A"], nv, rec[:, :nq], c, float(dlt))[:, qa:qa + 4]
                got = x[:, c, sg, qa:qa + 4].astype(np.float64)
                assert np.abs(got - ref).max() <= 4 * U, (c, sg, np.abs(got - ref).max())
                assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 4 * U
                assert np.abs(got - rec[:, qa:qa + 4]).max() > 1e-4          # it did move
                nrot += 1
            else:
                at = cols[c][1] if c < nv else (nq + c - nv if c < 2 * nv else nq + nv + c - 2 * nv)
                own[at] = True
                exp[:, at] = rec[:, at] + dlt                                 # one fp32 add
                assert (x[:, c, sg, at].view(np.int32) == exp[:, at].view(np.int32)).all(), (c, sg)
            assert (x[:, c, sg][:, ~own].view(np.int32) == rec[:, ~own].view(np.int32)).all(), (c, sg)
    assert nrot == 6 * sum(1 for k in cols if k[0] == "rot" and k[2] == 0)


def _fd_ref(r):
    """[A B; C D] columns from fd_y and the replayed sensordata in fp64: [N, ncol, 2nv + nsd], and h"""
    nq, nv, nu, ncol, nsd = r["dims"]
    h = float(np.float32(2.0) * np.float32(EPS)) if r["cfg"][3] else float(np.float32(EPS))
    y = r["y"].astype(np.float64)
    ref = np.zeros((N, ncol, 2 * nv + nsd))
    for c in range(ncol):
        ref[:, c, :nv] = differentiate_pos(r["A"], nv, y[:, c, 0, :nq], y[:, c, 1, :nq]) / h
        ref[:, c, nv:2 * nv] = (y[:, c, 0, nq:] - y[:, c, 1, nq:]) / h
        ref[:, c, 2 * nv:] = (r["sd"][:, c, 0] - r["sd"][:, c, 1]) / h
    return ref, h


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_the_differencing_is_right(cfg):
    """A, B, C, D against fp64 numpy on fd_y (mj_differentiatePos, the same h) and, for C and D, on the sensordata of the replayed
    runs: |out - ref| <= 1e-6 |ref| + 16 * 2^-24 / h -- the one rounding of the division, and the cancellation in the fp32
    quaternion log and subtraction.  The blocks are the transposed column buffer."""
    r = _run(cfg)
    nq, nv, nu, ncol, nsd = r["dims"]
    ref, h = _fd_ref(r)
    out = r["cols"][:, :, :2 * nv + nsd].astype(np.float64)
    err, bound = np.abs(out - ref), 1e-6 * np.abs(ref) + 16 * U / h
    print(_ID(cfg), "max |out - ref| %.3e, max err / bound %.3f, max |ref| %.3e" % (err.max(), (err / bound).max(), np.abs(ref).max()))
    assert (err <= bound).all(), f"{_ID(cfg)}: {(err > bound).sum()} entries beyond the bound, worst ratio {(err / bound).max():.2f}"
    assert (r["cols"][:, :, 2 * nv + nsd:] == 0.0).all()            # the rest of each row stays zero
    b, cols = r["blocks"], r["cols"]
    assert b["A"].shape == (N, 2 * nv, 2 * nv) and b["B"].shape == (N, 2 * nv, nu)
    assert b["C"].shape == (N, nsd, 2 * nv) and b["D"].shape == (N, nsd, nu)
    np.testing.assert_array_equal(b["A"], cols[:, :2 * nv, :2 * nv].transpose(0, 2, 1))
    np.testing.assert_array_equal(b["B"], cols[:, 2 * nv:, :2 * nv].transpose(0, 2, 1))
    np.testing.assert_array_equal(b["C"], cols[:, :2 * nv, 2 * nv:2 * nv + nsd].transpose(0, 2, 1))
    np.testing.assert_array_equal(b["D"], cols[:, 2 * nv:, 2 * nv:2 * nv + nsd].transpose(0, 2, 1))
    assert np.abs(b["A"]).max() > 0.5 and np.abs(b["B"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat", "footstand"])
def test_against_the_oracle_at_the_same_eps(oracle_mod, kind):
    """DR off, 16 contact-free states, nsteps = 1, eps 1e-3 centred, against central differences through the fp64 oracle's step
    from the record's warm start with the same perturbation formula; the yardstick is the fp32 oracle's same-eps distance from
    that.  Relative errors per env as _rel, bounded by the project's rule (_rule); no env is excluded."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 16
    envdef, E, _, _ = make(kind, n, False)
    E.reset(prng.split(prng.PRNGKey(1), n))
    qpos, qvel, ctrl = free_states(envdef, kind, n, 31)
    phys = Physics(E)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.transition_fd(nsteps=1, eps=EPS)
    torch.cuda.synchronize()
    assert int(phys.contacts()["ncon"].max()) == 0
    d = E.dims
    nq, nv, nu, ncol = d.nq, d.nv, d.nu, 2 * d.nv + d.nu
    hip = np.concatenate([phys.fd_A.cpu().numpy(), phys.fd_B.cpu().numpy()], 2)          # [n, 2nv, ncol]
    q0, v0, u0 = (getattr(phys, k).cpu().numpy().astype(np.float64) for k in ("qpos", "qvel", "ctrl"))
    warm = phys.qacc_warmstart.cpu().numpy().astype(np.float64)
    A = envdef.sys.arrays
    ref = {}
    for prec in ("f64", "f32"):
        o = oracle_mod.Oracle(E.blob, prec)
        o.set_ncon_cap(d.ncon_max)
        J = np.zeros((n, 2 * nv, ncol))
        for c in range(ncol):
            ends = []
            for dlt in (EPS, -EPS):
                q, v, u = q0.copy(), v0.copy(), u0.copy()
                if c < nv:
                    q = integrate_pos(A, nv, q, c, dlt)
                elif c < 2 * nv:
                    v[:, c - nv] += dlt
                else:
                    u[:, c - 2 * nv] += dlt
                yq, yv = np.zeros((n, nq)), np.zeros((n, nv))
                for e in range(n):
                    o.forward(q[e], v[e], u[e], warm[e], step=True)
                    yq[e], yv[e] = o.get("qpos"), o.get("qvel")
                ends.append((yq, yv))
            J[:, :nv, c] = differentiate_pos(A, nv, ends[0][0], ends[1][0]) / (2 * EPS)
            J[:, nv:, c] = (ends[0][1] - ends[1][1]) / (2 * EPS)
        ref[prec] = J
    print(kind, "fd [A B]: max |entry| %.3e, hip to the f32 oracle: max rel %.2e" % (np.abs(ref["f64"]).max(), rel(hip, ref["f32"]).max()))
    fails = []
    rule(kind, "fd [A B]", rel(hip, ref["f64"]), rel(ref["f32"], ref["f64"]), fails)
    assert not fails, fails


@pytest.mark.gpu
def test_env_ids_and_no_side_effects():
    """N = 65, a shuffled 7-env subset with envs 0 and 64: the other envs' rows stay bitwise zero, the selected rows equal an
    all-env call's, the record and every other buffer of the handle are bitwise unchanged, and a following env.step
    equals that of a batch that never made the call."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n, kind = 65, "go2flat"
    envdef, E = _stepped(kind, n, True)
    _, F = _stepped(kind, n, True)
    ids = [64, 3, 17, 0, 40, 9, 33]
    others = [e for e in range(n) if e not in ids]
    phys, twin = Physics(E, sensors=envdef.sensors), Physics(F, sensors=envdef.sensors)
    for p in (phys, twin):
        p.step(None, 1)
        p.dynamics()
        p.constraint_forces()
    assert float(phys.fd_A.abs().max()) == 0.0 and float(phys.fd_C.abs().max()) == 0.0      # zeros until the first call
    before = handle_snapshot(phys, all_but("transition"))
    phys.transition_fd(env_ids=ids, keep_states=True)
    assert_unchanged(before, handle_snapshot(phys, all_but("transition")))
    cols = handle_views(phys, "transition")["columns"].clone()
    assert (bits(cols[others]) == 0).all() and (bits(phys.fd_x[others]) == 0).all() and (bits(phys.fd_y[others]) == 0).all()
    assert float(cols[ids].abs().amax(dim=(1, 2)).min()) > 0
    phys.transition_fd()
    torch.cuda.synchronize()
    full = handle_views(phys, "transition")["columns"]
    assert torch.equal(bits(full[ids]), bits(cols[ids]))
    assert float(full[others].abs().amax(dim=(1, 2)).min()) > 0
    for bad in ([0, 0], [n], [-1]):
        with pytest.raises(ValueError):
            phys.transition_fd(env_ids=bad)
    for kw in (dict(nsteps=0), dict(eps=0.0), dict(eps=float("nan")), dict(eps=-1e-3)):
        with pytest.raises(ValueError):
            phys.transition_fd(**kw)
    act = np.clip(np.random.default_rng(9).normal(size=(n, E.dims.nu)) * 0.5, -1, 1).astype(np.float32)
    E.step(None, act)
    F.step(None, act)
    torch.cuda.synchronize()
    for k in PIPE + ("obs", "reward"):
        assert torch.equal(bits(E.view(k)), bits(F.view(k))), k


@pytest.mark.gpu
def test_sensor_rows():
    """go2flat with the env's sensor table: fd_C / fd_D have nsensordata rows, and the gyro rows of fd_C in the base
    angular-velocity columns are within the differencing bound of the replayed runs' values; with no table the shapes are
    [N, 0, .], and the blocks follow set_sensors."""
    import torch
    from rsr_mjx_amd.physics import Physics
    r = _run(CONFIGS[2])
    nq, nv, nu, ncol, nsd = r["dims"]
    assert nsd > 0 and r["blocks"]["C"].shape == (N, nsd, 2 * nv) and r["blocks"]["D"].shape == (N, nsd, nu)
    ref, h = _fd_ref(r)
    gyro = slice(2 * nv, 2 * nv + 3)                                # the table's first sensor
    got = r["blocks"]["C"][:, 0:3, nv + 3:nv + 6].astype(np.float64)          # d gyro / d base angular velocity
    want = ref[:, nv + 3:nv + 6, gyro].transpose(0, 2, 1)
    assert (np.abs(got - want) <= 1e-6 * np.abs(want) + 16 * U / h).all()
    assert np.abs(got).max() > 0.5                                  # the gyro reads the base's angular velocity
    bare = _run(CONFIGS[0])
    assert bare["dims"][4] == 0 and bare["blocks"]["C"].shape == (N, 0, 2 * bare["dims"][1]) and bare["blocks"]["D"].shape == (N, 0, bare["dims"][2])
    envdef, E, _, _ = make("go2flat", 4, False)
    E.reset(prng.split(prng.PRNGKey(2), 4))
    phys = Physics(E)
    assert phys.fd_C.shape == (4, 0, 2 * nv) and phys.fd_D.shape == (4, 0, nu)
    phys.set_sensors(envdef.sensors)
    phys.transition_fd(nsteps=1)
    torch.cuda.synchronize()
    assert phys.fd_C.shape == (4, nsd, 2 * nv) and phys.fd_D.shape == (4, nsd, nu) and float(phys.fd_C.abs().max()) > 0
    phys.set_sensors(None)
    assert phys.fd_C.shape == (4, 0, 2 * nv)
    # a table that shrinks leaves nothing behind: the rest of every row is written as zero by each call
    phys.transition_fd(nsteps=1)
    torch.cuda.synchronize()
    raw = phys._fetch("rsr_physics_transition_view", 0).cpu().numpy().reshape(4, ncol, -1)
    assert (raw[:, :, 2 * nv:].view(np.int32) == 0).all() and np.abs(raw[:, :, :2 * nv]).max() > 0
