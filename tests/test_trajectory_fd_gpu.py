"""Transition Jacobians along a trajectory (rsr_physics_trajectory_fd, Physics.trajectory_fd) on every built family: block (s, t)
of the columns is, bit for bit, what transition_fd writes on the same batch after t calls of step with the slot's controls; the
nominal rows are those of sample_rollouts with K = 1; nothing but the caller's buffers is written; an id out of range leaves its
slot's rows alone and a repeated id gives equal rows; a larger second call moves the scratch and changes nothing.
No tolerance anywhere: the equalities are bitwise, and tests/test_transition_gpu.py ties transition_fd to the step and the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from physics_support import (ALL_BUFFERS, FAMILIES, GO2, PIPE, applied_forces, assert_bitwise, assert_unchanged, handle_snapshot, handle_views,
                             make, sensor_spec)
from rsr_mjx_amd import prng

N, T, EPS = 8, 3, 1e-3
IDS = [5, 2, 99, 2]             # slot 2: an id out of range; slots 1 and 3: the same env (and the same ctrl rows)
SENTINEL = float("nan")

# name: (family, per-env leaves randomised, applied forces, centred, nsteps or None = n_substeps)
CONFIGS = {kind: (kind, False, False, True, None) for kind in FAMILIES}
CONFIGS.update({"cube-dr": ("cube", True, False, True, None), "go2flat-applied": ("go2flat", False, True, True, None),
                "cube-forward": ("cube", False, False, False, None), "go2flat-nsteps1": ("go2flat", False, False, True, 1)})


def _raw_call(pa, ids, ctrl, nsteps, flags, bufs):
    """the C call itself (Physics.trajectory_fd refuses an id out of range): ids and ctrl on the device, bufs {name: tensor}"""
    import torch
    from rsr_mjx_amd import _lib
    raw = torch.tensor(ids, dtype=torch.int32, device=ctrl.device)
    o = _lib.TrajectoryFdOut()
    for f, b in bufs.items():
        setattr(o, f, b.data_ptr())
    rc = _lib.lib().rsr_physics_trajectory_fd(pa._h, C.c_void_p(raw.data_ptr()), len(ids), C.c_void_p(ctrl.data_ptr()), int(ctrl.shape[1]),
                                              nsteps, EPS, flags, C.byref(o), pa._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rsr_last_error()


def _loop(A, pa, ctrl_of, steps, nsteps, centered):
    """The same result the way the calls before this one allow: for t < steps, ctrl_of(t) [N, nu] into the record, transition_fd,
    its columns kept [N, ncol, 2 nv + nsd], then step.  Returns the kept columns [steps, N, ncol, w]; the record has moved on."""
    import torch
    w = 2 * A.dims.nv + pa.nsensordata
    kept = []
    for t in range(steps):
        c = ctrl_of(t)
        pa.ctrl.copy_(c)
        pa.transition_fd(nsteps=nsteps, eps=EPS, centered=centered)
        torch.cuda.synchronize()
        kept.append(handle_views(pa, "transition")["columns"][:, :, :w].clone())
        pa.step(c, nsteps)
    torch.cuda.synchronize()
    return torch.stack(kept)


@functools.lru_cache(maxsize=None)
def _case(name):
    """An 8-env batch after a reset and 3 random env steps (cube on the table, feet on the ground), ctrl [4, T, nu] uniform in the
    ctrl range (slot 3's rows are slot 1's), the raw call on IDS into sentinel-filled buffers between two snapshots of everything
    the handle owns, and the loop's columns on the same batch; the record is put back.  Computed once and left unchanged."""
    import torch
    from rsr_mjx_amd import _lib
    from rsr_mjx_amd.physics import Physics
    kind, dr_on, applied, centered, nsteps = CONFIGS[name]
    envdef, A, _, scale = make(kind, N, dr_on)
    rng = np.random.default_rng(3)
    A.reset(prng.split(prng.PRNGKey(7), N))
    for _ in range(3):
        A.step(None, np.clip(rng.normal(size=(N, A.dims.nu)) * scale, -1, 1).astype(np.float32))
    pa = Physics(A, sensors=sensor_spec(kind, envdef) if kind in GO2 else None)
    if applied:
        pa.set_applied(*applied_forces(envdef, N, A.dims.nv, rng))
    nsteps = pa.n_substeps if nsteps is None else nsteps
    d, nsd = A.dims, pa.nsensordata
    ncol, w = 2 * d.nv + d.nu, 2 * d.nv + nsd
    lo, hi = envdef.sys.arrays["actuator_ctrlrange"].T
    ctrl = lo + (hi - lo) * rng.uniform(size=(len(IDS), T, d.nu))
    ctrl[3] = ctrl[1]
    ctrl = torch.as_tensor(ctrl.astype(np.float32), device=A.device)
    bufs = dict(columns=torch.full((len(IDS), T, ncol, w), SENTINEL, device=A.device),
                qpos=torch.full((len(IDS), T + 1, d.nq), SENTINEL, device=A.device),
                qvel=torch.full((len(IDS), T + 1, d.nv), SENTINEL, device=A.device))
    before = handle_snapshot(pa)
    pipe_before = {f: A.view(f).clone() for f in PIPE}
    _raw_call(pa, IDS, ctrl, nsteps, _lib.FD_CENTERED if centered else 0, bufs)
    after = handle_snapshot(pa)
    pipe_after = {f: A.view(f).clone() for f in PIPE}
    # the loop on the same batch; envs that no slot names keep the record's ctrl
    rec_ctrl = pa.ctrl.clone()

    def ctrl_of(t):
        c = rec_ctrl.clone()
        c[5], c[2] = ctrl[0, t], ctrl[1, t]
        return c
    ref = _loop(A, pa, ctrl_of, T, nsteps, centered)
    A.record.copy_(before["record"])
    torch.cuda.synchronize()
    return dict(kind=kind, envdef=envdef, A=A, pa=pa, ctrl=ctrl, bufs=bufs, ref=ref, before=before, after=after, pipe_before=pipe_before,
                pipe_after=pipe_after, nsteps=nsteps, centered=centered, rec_ctrl=rec_ctrl)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_columns_are_the_loop_of_transition_fd_and_step_bit_for_bit(name):
    import torch
    c = _case(name)
    col, ref = c["bufs"]["columns"], c["ref"]
    if c["kind"] in GO2:
        assert c["pa"].nsensordata > 0                                     # C and D are exercised
    for s, e in ((0, 5), (1, 2), (3, 2)):
        for t in range(T):
            assert_bitwise(f"{name} slot {s} (env {e}) t {t}", col[s, t], ref[t, e])
        assert torch.isfinite(col[s]).all() and bool((col[s] != 0).any())
    assert_bitwise(f"{name} the two slots of env 2", col[3], col[1])
    assert not torch.equal(col[0, 0], col[0, T - 1])                       # (the trajectory went somewhere)
    for f, b in c["bufs"].items():                                         # the id out of range: its rows in all three buffers
        assert torch.isnan(b[2]).all(), f


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_nominal_rows_are_the_sampled_rollout_with_one_sample(name):
    import torch
    c = _case(name)
    A, pa, bufs = c["A"], c["pa"], c["bufs"]
    one = pa.sample_rollouts(c["ctrl"][:2, None].contiguous(), nsteps=c["nsteps"], fields=("qpos", "qvel"), env_ids=IDS[:2])
    torch.cuda.synchronize()
    for f in ("qpos", "qvel"):
        for s, src in ((0, 0), (1, 1), (3, 1)):
            assert_bitwise(f"{name} {f} slot {s}", bufs[f][s, 1:], one[f][src, 0])
            assert_bitwise(f"{name} {f} slot {s} row 0", bufs[f][s, 0], A.view(f)[IDS[s]])
    assert_bitwise(f"{name} record", A.record, c["before"]["record"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_nothing_but_the_callers_buffers_is_written(name):
    c = _case(name)
    assert set(ALL_BUFFERS) == {"record", "side", "applied", "dynamics", "constraint", "transition", "inverse"}
    assert_unchanged(c["before"], c["after"])
    assert sorted(c["before"]) == sorted(c["after"]) and "fd_columns" in c["before"] and "record" in c["before"]
    assert ("applied_xfrc" in c["before"]) == (name == "go2flat-applied")
    for f in PIPE:
        assert_bitwise(f"{name} record field {f}", c["pipe_after"][f], c["pipe_before"][f])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "go2flat", "go2flat-applied", "cube-forward"])
def test_a_larger_call_moves_the_scratch_and_the_views_are_the_blocks(name):
    import torch
    c = _case(name)
    A, pa, ctrl, first = c["A"], c["pa"], c["ctrl"], c["bufs"]["columns"]
    d, nsd, kw = A.dims, pa.nsensordata, dict(nsteps=c["nsteps"], eps=EPS, centered=c["centered"])
    nv, nu = d.nv, d.nu
    # nominal=False (null members): the same columns, by the method this time; an env may repeat
    bare = pa.trajectory_fd(ctrl[[0, 1, 3]].contiguous(), env_ids=[5, 2, 2], nominal=False, **kw)
    torch.cuda.synchronize()
    assert sorted(bare) == ["A", "B", "C", "D", "columns"]
    assert_bitwise(f"{name} nominal=False", bare["columns"], first[[0, 1, 3]])
    # every env and one control step more: M T grows from 12 to 32, so the scratch is replaced; the first T steps are as before
    lo, hi = c["envdef"].sys.arrays["actuator_ctrlrange"].T
    big_ctrl = torch.as_tensor((lo + (hi - lo) * np.random.default_rng(8).uniform(size=(N, T + 1, nu))).astype(np.float32), device=A.device)
    big_ctrl[5, :T], big_ctrl[2, :T] = ctrl[0], ctrl[1]
    big = pa.trajectory_fd(big_ctrl, **kw)
    torch.cuda.synchronize()
    assert big["columns"].shape == (N, T + 1, 2 * nv + nu, 2 * nv + nsd) and big["qpos"].shape == (N, T + 2, d.nq) and big["qvel"].shape == (N, T + 2, nv)
    for s, e in ((0, 5), (1, 2)):
        assert_bitwise(f"{name} env {e} in the larger call", big["columns"][e, :T], c["ref"][:, e])
        assert_bitwise(f"{name} env {e} qpos in the larger call", big["qpos"][e, :T + 1], c["bufs"]["qpos"][s])
    # and the smaller call again, in the larger scratch
    again = pa.trajectory_fd(ctrl[[0, 1, 3]].contiguous(), env_ids=[5, 2, 2], **kw)
    torch.cuda.synchronize()
    assert_bitwise(f"{name} the first call again", again["columns"], first[[0, 1, 3]])
    assert_bitwise(f"{name} record", A.record, c["before"]["record"])
    # the views alias the columns, one row of the buffer per column of [A B; C D]
    col = big["columns"]
    shapes = dict(A=(N, T + 1, 2 * nv, 2 * nv), B=(N, T + 1, 2 * nv, nu), C=(N, T + 1, nsd, 2 * nv), D=(N, T + 1, nsd, nu))
    at = dict(A=(0, 0), B=(2 * nv, 0), C=(0, 2 * nv), D=(2 * nv, 2 * nv))                   # (first column, first row) of the block
    for k, shape in shapes.items():
        v = big[k]
        assert tuple(v.shape) == shape, k
        c0, r0 = at[k]
        if v.numel():
            assert v.data_ptr() == col[0, 0, c0, r0:].data_ptr() and v.stride() == (col.stride(0), col.stride(1), 1, col.stride(2)), k
            assert_bitwise(f"{name} {k} transposed", v, col[:, :, c0:c0 + shape[3], r0:r0 + shape[2]].transpose(2, 3))
    # ... oriented as fd_A .. fd_D: at t = 0 they are transition_fd's on the record holding ctrl[:, 0]
    pa.ctrl.copy_(big_ctrl[:, 0])
    pa.transition_fd(**kw)
    torch.cuda.synchronize()
    for k in shapes:
        assert_bitwise(f"{name} {k} at t = 0 against fd_{k}", big[k][:, 0], getattr(pa, "fd_" + k))
    A.record.copy_(c["before"]["record"])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_refusals_on_the_device():
    import torch
    from rsr_mjx_amd import _lib
    c = _case("cube")
    A, pa = c["A"], c["pa"]
    L = _lib.lib()
    fn = L.rsr_physics_trajectory_fd
    ctrl = C.c_void_p(c["ctrl"].data_ptr())
    ids = torch.tensor([0, 1], dtype=torch.int32, device=A.device)
    idp = C.c_void_p(ids.data_ptr())
    col = torch.full_like(c["bufs"]["columns"], -7.25)
    o, none = _lib.TrajectoryFdOut(), _lib.TrajectoryFdOut()
    o.columns = col.data_ptr()
    nf, op = pa.n_substeps, C.byref(o)
    torch.cuda.synchronize()
    for what, args in (("T = 0", (pa._h, idp, 2, ctrl, 0, nf, EPS, 1, op)), ("nsteps = 0", (pa._h, idp, 2, ctrl, T, 0, EPS, 1, op)),
                       ("nsteps = 2^30", (pa._h, idp, 2, ctrl, T, 2 ** 30, EPS, 1, op)), ("eps = 0", (pa._h, idp, 2, ctrl, T, nf, 0.0, 1, op)),
                       ("eps = inf", (pa._h, idp, 2, ctrl, T, nf, float("inf"), 1, op)), ("eps = nan", (pa._h, idp, 2, ctrl, T, nf, float("nan"), 1, op)),
                       ("RSR_FD_STATES", (pa._h, idp, 2, ctrl, T, nf, EPS, 3, op)), ("an unknown bit", (pa._h, idp, 2, ctrl, T, nf, EPS, 4, op)),
                       ("count = 0", (pa._h, idp, 0, ctrl, T, nf, EPS, 1, op)), ("null ctrl", (pa._h, idp, 2, None, T, nf, EPS, 1, op)),
                       ("null out", (pa._h, idp, 2, ctrl, T, nf, EPS, 1, None)), ("null columns", (pa._h, idp, 2, ctrl, T, nf, EPS, 1, C.byref(none))),
                       ("T nsteps = 2^31", (pa._h, idp, 2, ctrl, 4, 2 ** 29, EPS, 1, op)),
                       ("M T ncol = 2^31", (pa._h, idp, 2 ** 20, ctrl, 2 ** 11, nf, EPS, 1, op))):
        assert fn(*args, pa._stream()) == -1, what                       # RSR_ERR_ARG
        assert b"rsr_physics_trajectory_fd" in L.rsr_last_error(), what
    torch.cuda.synchronize()
    assert_bitwise("record after the refusals", A.record, c["before"]["record"])
    assert (col == -7.25).all()
