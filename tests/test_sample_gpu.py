"""Sampled rollouts (rsr_physics_sample_rollouts, Physics.sample_rollouts) on every built family: K control sequences per env from
the env's record as it stands are, bit for bit, what Physics.rollout records on a replica batch of N * K envs that hold the same
record rows and per-env leaves; nothing but the caller's buffers is written; rows go by slot; the handle's other buffers do not
enter the dispatch; the refusals hold on the device.
No tolerance anywhere: the existing tests tie rollout_kernel to physics_kernel, to rsr_step and to the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from physics_support import ALL, FAMILIES, applied_forces, assert_bitwise, assert_unchanged, handle_snapshot, pair, replica, sensor_spec

N, K, T = 64, 5, 4              # K odd, no divisor of N; N * K = 320 workgroups


@functools.lru_cache(maxsize=None)
def _case(kind, applied=False):
    """Batch A (reset, 3 random env steps: cube on the table, feet on the ground), its untouched twin, ctrl [N, K, T, nu] uniform
    in the ctrl range, A's sampled rollouts and the replica batch's rollout, each computed once and left unchanged."""
    import torch
    from rsr_mjx_amd.physics import Physics
    envdef, A, twin, scale, rng = pair(kind, N)
    spec = sensor_spec(kind, envdef)
    pa = Physics(A, sensors=spec)
    R = replica(kind, envdef, A, K)
    pr = Physics(R, sensors=spec)
    if applied:
        x, q = applied_forces(envdef, N, A.dims.nv, rng)
        pa.set_applied(x, q)
        pr.set_applied(np.repeat(x, K, 0), np.repeat(q, K, 0))
    rng_c = envdef.sys.arrays["actuator_ctrlrange"]
    lo, hi = rng_c[:, 0], rng_c[:, 1]
    ctrl = torch.as_tensor((lo + (hi - lo) * rng.uniform(size=(N, K, T, A.dims.nu))).astype(np.float32), device=A.device)
    before = handle_snapshot(pa)
    full = pa.sample_rollouts(ctrl, fields=ALL)
    after = handle_snapshot(pa)
    ref = pr.rollout(ctrl.reshape(N * K, T, A.dims.nu), fields=ALL)
    torch.cuda.synchronize()
    del pr, R
    return dict(envdef=envdef, A=A, twin=twin, pa=pa, scale=scale, ctrl=ctrl, full=full, ref=ref, before=before, after=after)


def _check_against_replica(kind, c):
    import torch
    assert c["pa"].nsensordata > 0
    for f in ALL:
        assert c["full"][f].shape[:3] == (N, K, T)
        assert_bitwise(f"{kind} sample {f}", c["full"][f], c["ref"][f].reshape(N, K, T, -1))
        assert torch.isfinite(c["full"][f]).all(), f
    assert (c["full"]["ncon"] > 0).any()                                  # contacts were active
    assert_unchanged(c["before"], c["after"])                             # the whole record and every buffer of the handle


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_samples_are_the_replica_rollout_bit_for_bit(kind):
    import torch
    c = _case(kind)
    _check_against_replica(kind, c)
    # env.step goes on as on a twin that never ran a sampled rollout
    A, twin = c["A"], c["twin"]
    A.record.copy_(c["before"]["record"]); twin.record.copy_(c["before"]["record"])
    c["pa"].sample_rollouts(c["ctrl"], fields=("qpos",))
    act = np.clip(np.random.default_rng(11).normal(size=(N, A.dims.nu)) * c["scale"], -1, 1).astype(np.float32)
    A.step(None, act)
    twin.step(None, act)
    torch.cuda.synchronize()
    assert_bitwise(f"{kind} env.step after sample_rollouts", A.record, twin.record)
    A.record.copy_(c["before"]["record"])
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_applied_forces_are_the_envs_own(kind):
    c = _case(kind, True)
    assert c["pa"].xfrc_applied is not None and bool((c["pa"].xfrc_applied != 0).any())
    _check_against_replica(kind, c)
    plain = _case(kind)
    assert not (c["full"]["qvel"] == plain["full"]["qvel"]).all()         # (the forces were felt)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2rough"])
def test_rows_go_by_slot(kind):
    import torch
    from rsr_mjx_amd import _lib
    c = _case(kind)
    A, pa, full = c["A"], c["pa"], c["full"]
    A.record.copy_(c["before"]["record"])
    ids = [41, 3, 17]
    sub_ctrl = c["ctrl"][ids].contiguous()
    # caller-owned tensors for M = 3, each the head of a larger sentinel-filled buffer: written in full, and nothing beyond
    buf = {f: torch.full((len(ids) + 1,) + tuple(full[f].shape[1:]), -7.25, device=A.device) for f in ALL}
    out = pa.sample_rollouts(sub_ctrl, fields=ALL, env_ids=ids, out={f: b[:len(ids)] for f, b in buf.items()})
    torch.cuda.synchronize()
    for f in ALL:
        assert out[f].data_ptr() == buf[f].data_ptr()
        for s, e in enumerate(ids):
            assert_bitwise(f"{kind} slot {s} (env {e}) {f}", out[f][s], full[f][e])
        assert (buf[f][len(ids)] == -7.25).all(), f
    assert_bitwise(f"{kind} record", A.record, c["before"]["record"])
    # an empty list launches nothing
    empty = pa.sample_rollouts(sub_ctrl[:0], env_ids=[])
    assert {f: tuple(t.shape) for f, t in empty.items()} == dict(qpos=(0, K, T, A.dims.nq), qvel=(0, K, T, A.dims.nv), time=(0, K, T, 1))
    # the raw call: an id of num_envs runs nothing and leaves its slot's rows as they were; the other slots are right
    for b in buf.values():
        b.fill_(-7.25)
    raw = torch.tensor([41, N, 17], dtype=torch.int32, device=A.device)
    o = _lib.RolloutOut()
    for f in ALL:
        setattr(o, f, buf[f].data_ptr())
    rc = _lib.lib().rsr_physics_sample_rollouts(pa._h, C.c_void_p(raw.data_ptr()), 3, C.c_void_p(sub_ctrl.data_ptr()), K, T,
                                                pa.n_substeps, C.byref(o), pa._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rsr_last_error()
    for f in ALL:
        assert_bitwise(f"{kind} raw slot 0 {f}", buf[f][0], full[f][41])
        assert_bitwise(f"{kind} raw slot 2 {f}", buf[f][2], full[f][17])
        assert (buf[f][1] == -7.25).all() and (buf[f][3] == -7.25).all(), f
    assert_bitwise(f"{kind} record after the raw call", A.record, c["before"]["record"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_samples_are_indexed_by_k(kind):
    import torch
    from rsr_mjx_amd.physics import Physics
    c = _case(kind)
    A, twin, pa, ctrl = c["A"], c["twin"], c["pa"], c["ctrl"]
    A.record.copy_(c["before"]["record"])
    same = pa.sample_rollouts(ctrl[:, :1].expand(N, K, T, A.dims.nu).contiguous(), fields=ALL)
    torch.cuda.synchronize()
    for f in ALL:
        for k in range(1, K):
            assert_bitwise(f"{kind} same ctrl, sample {k} {f}", same[f][:, k], same[f][:, 0])
        assert_bitwise(f"{kind} same ctrl is sample 0 of the distinct ones {f}", same[f][:, 0], c["full"][f][:, 0])
    assert any(not torch.equal(c["full"]["qpos"][:, k], c["full"]["qpos"][:, 0]) for k in range(1, K))
    # K = 1 is rollout on a copy of the batch
    one = pa.sample_rollouts(ctrl[:, :1].contiguous(), fields=ALL)
    twin.record.copy_(c["before"]["record"])
    ref = Physics(twin, sensors=sensor_spec(kind, c["envdef"])).rollout(ctrl[:, 0].contiguous(), fields=ALL)
    torch.cuda.synchronize()
    for f in ALL:
        assert_bitwise(f"{kind} K = 1 {f}", one[f][:, 0], ref[f])
    assert_bitwise(f"{kind} record", A.record, c["before"]["record"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_dispatch_ignores_the_handles_other_buffers(kind):
    """Which kernel a call launches depends on the call alone, not on which of the handle's buffers exist: sample_rollouts and
    inverse on a fresh handle, and on a second handle of the same batch that has run dynamics, constraint_forces and
    transition_fd (so that it owns those buffers) and has applied forces on, all zero, give bit-identical outputs from the same
    state.  Nothing about the values is asserted (the tests above and tests/test_inverse_gpu.py do that)."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n, k, t = 2, 2, 2
    envdef, A, _, _, rng = pair(kind, n)
    spec = sensor_spec(kind, envdef)
    lo, hi = envdef.sys.arrays["actuator_ctrlrange"].T
    ctrl = torch.as_tensor((lo + (hi - lo) * rng.uniform(size=(n, k, t, A.dims.nu))).astype(np.float32), device=A.device)
    qacc = (5.0 * torch.randn((n, A.dims.nv), generator=torch.Generator(device="cpu").manual_seed(2))).to(A.device).contiguous()
    state = {f: A.view(f).clone() for f in ("qpos", "qvel", "ctrl")}

    def run(phys):
        phys.set_state(**state)                                           # the same record for both handles
        out = {"sample " + f: v.clone() for f, v in phys.sample_rollouts(ctrl, nsteps=1, fields=ALL).items()}
        phys.inverse(qacc)
        out.update(handle_snapshot(phys, ("inverse",)))
        return out
    first = run(Physics(A, sensors=spec))
    second = Physics(A, sensors=spec)
    second.dynamics()
    second.constraint_forces()
    second.transition_fd(nsteps=1)
    second.set_applied()                                                  # on, zero everywhere
    assert second.xfrc_applied is not None and not bool(second.xfrc_applied.any()) and not bool(second.qfrc_applied.any())
    again = run(second)
    assert sorted(first) == sorted(again) and len(first) == len(ALL) + 6
    for f, v in first.items():
        assert_bitwise(f"{kind} {f}", again[f], v)


@pytest.mark.gpu
def test_refusals_on_the_device():
    import torch
    from rsr_mjx_amd import _lib
    from rsr_mjx_amd.physics import Physics
    c = _case("cube")
    A, pa = c["A"], c["pa"]
    A.record.copy_(c["before"]["record"])
    bare = Physics(A)                                                    # a handle with no sensor table
    L = _lib.lib()
    fn = L.rsr_physics_sample_rollouts
    ctrl = C.c_void_p(c["ctrl"].data_ptr())
    ids = torch.tensor([0, 1], dtype=torch.int32, device=A.device)
    idp = C.c_void_p(ids.data_ptr())
    qpos = torch.full((N, K, T, A.dims.nq), -7.25, device=A.device)
    sd = torch.full((N, K, T, pa.nsensordata), -7.25, device=A.device)
    o, none, osd = _lib.RolloutOut(), _lib.RolloutOut(), _lib.RolloutOut()
    o.qpos = qpos.data_ptr()
    osd.sensordata = sd.data_ptr()
    nf = pa.n_substeps
    torch.cuda.synchronize()
    before = A.record.clone()
    for what, args in (("K = 0", (pa._h, None, 0, ctrl, 0, T, nf, C.byref(o))), ("T = 0", (pa._h, None, 0, ctrl, K, 0, nf, C.byref(o))),
                       ("nsteps = 0", (pa._h, None, 0, ctrl, K, T, 0, C.byref(o))), ("count = 0", (pa._h, idp, 0, ctrl, K, T, nf, C.byref(o))),
                       ("null ctrl", (pa._h, None, 0, None, K, T, nf, C.byref(o))), ("null out", (pa._h, None, 0, ctrl, K, T, nf, None)),
                       ("all-null out", (pa._h, None, 0, ctrl, K, T, nf, C.byref(none))),
                       ("sensordata, no table", (bare._h, None, 0, ctrl, K, T, nf, C.byref(osd)))):
        assert fn(*args, pa._stream()) == -1, what                       # RSR_ERR_ARG
        assert b"rsr_physics_sample_rollouts" in L.rsr_last_error(), what
    torch.cuda.synchronize()
    assert_bitwise("record after the refusals", A.record, before)
    assert (qpos == -7.25).all() and (sd == -7.25).all()
