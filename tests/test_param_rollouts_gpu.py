"""Parameter rollouts (rsr_physics_param_rollouts, Physics.param_rollouts) on every built family: K sets of model leaves per env
from the env's record as it stands are, bit for bit, what Physics.rollout records on a replica batch of N * K envs that hold the
same record rows and, through set_randomization, each sample's leaves; one leaf at a time too; the call reduces to
sample_rollouts; nothing but the caller's buffers is written; rows go by slot; applied forces are the env's; the refusals hold
on the device; tuning.RolloutLoss finds the candidate a trajectory came from.
No tolerance anywhere: the existing tests tie rollout_kernel to physics_kernel, to rsr_step and to the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from physics_support import (ALL, FAMILIES, applied_forces, assert_bitwise, assert_unchanged, default_dr, handle_snapshot, make, pair, replica,
                             sensor_spec)
from rsr_mjx_amd import prng

N, K, T = 64, 5, 4              # K odd, no divisor of N; N * K = 320 workgroups and replica envs
BASE_LEAVES = ("geom_friction", "body_mass", "dof_damping", "dof_frictionloss")
GO2_LEAVES = ("body_ipos", "qpos0", "dof_armature", "actuator_gainprm", "actuator_biasprm")
GO2 = ("go2flat", "go2rough", "footstand")


def _leaves_of(kind):
    return BASE_LEAVES + (GO2_LEAVES if kind in GO2 else ())


def _base(kind, dr_on=True, applied=False):
    return _base_once(kind, bool(dr_on), bool(applied))


@functools.lru_cache(maxsize=None)
def _base_once(kind, dr_on, applied):
    """Batch A (reset, 3 random env steps: cube on the table, feet on the ground) with its handle, its untouched twin, each env's
    own leaves [N, ...] (its per-env values, or the model's), one ctrl sequence per env [N, T, nu] uniform in the ctrl range, and
    a snapshot of everything the handle owns."""
    import torch
    from rsr_mjx_amd.physics import Physics
    if dr_on:
        envdef, A, twin, scale, rng = pair(kind, N)                   # (DR on but for the T-shape, whose batch has none)
        dr = default_dr(kind, envdef, N)
    else:                                                             # pair's steps on batches built with no per-env leaves
        envdef, A, _, scale = make(kind, N, False)
        _, twin, _, _ = make(kind, N, False)
        rng, dr = np.random.default_rng(3), None
        A.reset(prng.split(prng.PRNGKey(7), N))
        twin.reset(prng.split(prng.PRNGKey(7), N))
        for _ in range(3):
            A.step(None, np.clip(rng.normal(size=(N, A.dims.nu)) * scale, -1, 1).astype(np.float32))
        twin.record.copy_(A.record)
        torch.cuda.synchronize()
    spec = sensor_spec(kind, envdef)
    pa = Physics(A, sensors=spec)
    arr = envdef.sys.arrays
    own = {f: np.asarray(dr[f], np.float32).copy() if dr is not None else np.tile(arr[f].astype(np.float32)[None], (N,) + (1,) * arr[f].ndim)
           for f in _leaves_of(kind)}
    lo, hi = arr["actuator_ctrlrange"][:, 0], arr["actuator_ctrlrange"][:, 1]
    ctrl = torch.as_tensor((lo + (hi - lo) * rng.uniform(size=(N, T, A.dims.nu))).astype(np.float32), device=A.device)
    forces = None
    if applied:                                                       # (drawn last: plain and applied share ctrl)
        forces = applied_forces(envdef, N, A.dims.nv, rng)
        pa.set_applied(*forces)
    return dict(kind=kind, envdef=envdef, A=A, twin=twin, pa=pa, scale=scale, spec=spec, dr=dr, own=own, ctrl=ctrl, forces=forces,
                before=handle_snapshot(pa))


def _sampled(c, names, seed=21):
    """{leaf: tensor [N, K, ...]} around each env's own value: friction 0.3 to 1.2, masses, armature and gains kept positive,
    qpos0 +- 0.02 on the joints"""
    import torch
    rng = np.random.default_rng(seed)
    out = {}
    for f in names:
        v = np.repeat(c["own"][f][:, None], K, 1).astype(np.float64)
        u = lambda lo, hi, shape=None: rng.uniform(lo, hi, size=v.shape if shape is None else shape)
        if f == "geom_friction":
            v[..., 0] = u(0.3, 1.2, v.shape[:-1])
        elif f == "body_mass":
            v = v * u(0.8, 1.2)
        elif f == "dof_damping":
            v = v * u(0.7, 1.3) + u(0.0, 0.05)
        elif f == "dof_frictionloss":
            v = v * u(0.7, 1.3) + u(0.0, 0.02)
        elif f == "body_ipos":
            v = v + u(-0.02, 0.02)
        elif f == "qpos0":
            v[..., 7:] = v[..., 7:] + u(-0.02, 0.02, v[..., 7:].shape)
        elif f == "dof_armature":
            v = v * u(0.9, 1.3) + u(0.0, 0.005)
        else:                                                         # actuator_gainprm, actuator_biasprm
            v = v * u(0.9, 1.1)
        out[f] = torch.as_tensor(v.astype(np.float32), device=c["A"].device).contiguous()
    return out


def _replica(kind, dr_on=True, applied=False):
    return _replica_once(kind, bool(dr_on), bool(applied))


@functools.lru_cache(maxsize=None)
def _replica_once(kind, dr_on, applied):
    """N * K envs and their handle, built once per case; _ref gives them their rows and leaves"""
    from rsr_mjx_amd.physics import Physics
    c = _base(kind, dr_on, applied)
    R = replica(kind, c["envdef"], c["A"], K, dr=None)                # (no per-env leaves here: _ref writes them at every use)
    pr = Physics(R, sensors=c["spec"])
    if applied:
        pr.set_applied(np.repeat(c["forces"][0], K, 0), np.repeat(c["forces"][1], K, 0))
    return R, pr


def _ref(c, params, ctrl, dr_on=True, applied=False):
    """Physics.rollout on the replica batch: env e * K + j holds env e's record row, env e's own per-env leaves and, over them,
    sample (e, j)'s; ctrl [N, K, T, nu].  {field: [N, K, T, w]}"""
    import torch
    R, pr = _replica(c["kind"], dr_on, applied)
    torch.cuda.synchronize()
    leaves = {} if c["dr"] is None else {f: torch.as_tensor(np.repeat(np.asarray(v, np.float32), K, 0), device=R.device) for f, v in c["dr"].items()}
    leaves.update({f: v.reshape((N * K,) + tuple(v.shape[2:])) for f, v in params.items()})
    R.set_randomization(leaves)
    R.record.copy_(c["before"]["record"].repeat_interleave(K, 0))
    ref = pr.rollout(ctrl.reshape(N * K, T, -1).contiguous(), fields=ALL)
    torch.cuda.synchronize()
    return {f: v.reshape((N, K, T, -1)).clone() for f, v in ref.items()}


def _each(ctrl):
    """the shared sequences [N, T, nu] as per-sample ones [N, K, T, nu] (ctrl.repeat_interleave(K, 0), by slot and sample)"""
    return ctrl.repeat_interleave(K, 0).reshape(N, K, T, -1).contiguous()


def _case(kind, applied=False):
    return _case_once(kind, bool(applied))


@functools.lru_cache(maxsize=None)
def _case_once(kind, applied):
    """every leaf the family supports sampled, shared ctrl: the call's result, the replica's, and the handle after the call"""
    import torch
    c = _base(kind, True, applied)
    params = _sampled(c, _leaves_of(kind))
    full = c["pa"].param_rollouts(c["ctrl"], params, fields=ALL)
    after = handle_snapshot(c["pa"])
    ref = _ref(c, params, _each(c["ctrl"]), True, applied)
    return dict(c, params=params, full=full, ref=ref, after=after)


@functools.lru_cache(maxsize=None)
def _own(kind):
    """the all-NULL run: no leaf sampled, per-sample copies of the shared ctrl"""
    import torch
    c = _base(kind)
    out = c["pa"].param_rollouts(_each(c["ctrl"]), {}, fields=ALL)
    torch.cuda.synchronize()
    return out


def _check_against_replica(name, got, ref):
    import torch
    for f in ALL:
        assert got[f].shape[:3] == (N, K, T), f
        assert_bitwise(f"{name} {f}", got[f], ref[f])
        assert torch.isfinite(got[f]).all(), f


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_samples_are_the_replica_rollout_bit_for_bit(kind):
    import torch
    c = _case(kind)
    assert c["pa"].nsensordata > 0 and sorted(c["params"]) == sorted(_leaves_of(kind))
    _check_against_replica(f"{kind} all leaves", c["full"], c["ref"])
    assert (c["full"]["ncon"] > 0).any()                                  # contacts were active
    # the leaves were felt: the samples of one env differ from each other
    q = c["full"]["qpos"]
    assert all(not torch.equal(q[:, j], q[:, 0]) for j in range(1, K))
    assert bool((q[:, 1:] != q[:, :1]).flatten(1).any(1).all())           # in every env


ONE_LEAF = [("cube", f) for f in BASE_LEAVES] + [("go2rough", f) for f in BASE_LEAVES + GO2_LEAVES]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,leaf", ONE_LEAF)
def test_one_leaf_at_a_time(kind, leaf):
    """Only `leaf` is sampled; the others stay the env's own per-env values.  Catches an overlay that ignores, mis-indexes or
    mis-maps a leaf (friction goes through the geom slots on the Go2 models)."""
    import torch
    c = _base(kind)
    params = _sampled(c, (leaf,), seed=33)
    got = c["pa"].param_rollouts(c["ctrl"], params, fields=ALL)
    torch.cuda.synchronize()
    _check_against_replica(f"{kind} {leaf} alone", got, _ref(c, params, _each(c["ctrl"])))
    own = _own(kind)
    assert not torch.equal(got["qpos"], own["qpos"]) or not torch.equal(got["qvel"], own["qvel"])
    assert_bitwise(f"{kind} record", c["A"].record, c["before"]["record"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "footstand"])
def test_reduces_to_the_existing_calls(kind):
    import torch
    c = _base(kind)
    pa, A = c["pa"], c["A"]
    rng = np.random.default_rng(5)
    lo, hi = c["envdef"].sys.arrays["actuator_ctrlrange"].T
    each = torch.as_tensor((lo + (hi - lo) * rng.uniform(size=(N, K, T, A.dims.nu))).astype(np.float32), device=A.device)
    # no params, per-sample ctrl: sample_rollouts
    got = pa.param_rollouts(each, {}, fields=ALL)
    want = pa.sample_rollouts(each, fields=ALL)
    torch.cuda.synchronize()
    for f in ALL:
        assert_bitwise(f"{kind} params = {{}} {f}", got[f], want[f])
    # shared ctrl is per-sample ctrl with the row repeated
    params = _sampled(c, _leaves_of(kind), seed=44)
    shared = pa.param_rollouts(c["ctrl"], params, fields=ALL)
    rep = pa.param_rollouts(_each(c["ctrl"]), params, fields=ALL)
    torch.cuda.synchronize()
    for f in ALL:
        assert_bitwise(f"{kind} shared ctrl {f}", shared[f], rep[f])
    assert_bitwise(f"{kind} record", A.record, c["before"]["record"])
    # a batch with no per-env leaves: a leaf that is not sampled is the model's
    d = _base(kind, dr_on=False)
    assert not d["A"]._dr
    some = _sampled(d, ("body_mass", "dof_damping") if kind == "cube" else ("geom_friction", "dof_armature", "actuator_gainprm"), seed=55)
    off = d["pa"].param_rollouts(d["ctrl"], some, fields=ALL)
    torch.cuda.synchronize()
    _check_against_replica(f"{kind} DR off", off, _ref(d, some, _each(d["ctrl"]), dr_on=False))
    assert (off["ncon"] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_nothing_else_is_written(kind):
    import torch
    c = _case(kind)
    A, twin, pa = c["A"], c["twin"], c["pa"]
    assert_unchanged(c["before"], c["after"])                             # the whole record and every buffer of the handle
    # the batch's own leaf tensors, and the caller's
    assert sorted(A._dr) == sorted(_leaves_of(kind))
    own = {f: v.clone() for f, v in A._dr.items()}
    given = {f: v.clone() for f, v in c["params"].items()}
    A.record.copy_(c["before"]["record"]); twin.record.copy_(c["before"]["record"])
    pa.param_rollouts(c["ctrl"], c["params"], fields=("qpos",))
    torch.cuda.synchronize()
    for f, v in own.items():
        assert_bitwise(f"{kind} the batch's {f}", A._dr[f], v)
    for f, v in given.items():
        assert_bitwise(f"{kind} the caller's {f}", c["params"][f], v)
    # env.step goes on as on a twin that never ran a parameter rollout
    act = np.clip(np.random.default_rng(11).normal(size=(N, A.dims.nu)) * c["scale"], -1, 1).astype(np.float32)
    A.step(None, act)
    twin.step(None, act)
    torch.cuda.synchronize()
    assert_bitwise(f"{kind} env.step after param_rollouts", A.record, twin.record)
    A.record.copy_(c["before"]["record"])
    torch.cuda.synchronize()


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
    sub = {f: v[ids].contiguous() for f, v in c["params"].items()}
    # caller-owned tensors for M = 3, each the head of a larger sentinel-filled buffer: written in full, and nothing beyond
    buf = {f: torch.full((len(ids) + 1,) + tuple(full[f].shape[1:]), -7.25, device=A.device) for f in ALL}
    out = pa.param_rollouts(sub_ctrl, sub, fields=ALL, env_ids=ids, out={f: b[:len(ids)] for f, b in buf.items()})
    torch.cuda.synchronize()
    for f in ALL:
        assert out[f].data_ptr() == buf[f].data_ptr()
        for s, e in enumerate(ids):
            assert_bitwise(f"{kind} slot {s} (env {e}) {f}", out[f][s], full[f][e])
        assert (buf[f][len(ids)] == -7.25).all(), f
    assert_bitwise(f"{kind} record", A.record, c["before"]["record"])
    # an empty list launches nothing
    empty = pa.param_rollouts(sub_ctrl[:0], {f: v[:0] for f, v in sub.items()}, env_ids=[])
    assert {f: tuple(t.shape) for f, t in empty.items()} == dict(qpos=(0, K, T, A.dims.nq), qvel=(0, K, T, A.dims.nv), time=(0, K, T, 1))
    # the raw call: an id of num_envs runs nothing and leaves its slot's rows as they were; the other slots are right
    for b in buf.values():
        b.fill_(-7.25)
    raw = torch.tensor([41, N, 17], dtype=torch.int32, device=A.device)
    o, ps = _lib.RolloutOut(), _lib.ParamSamples()
    for f in ALL:
        setattr(o, f, buf[f].data_ptr())
    for f, v in sub.items():
        ps.leaf[_lib.DR_FIELDS.index(f)] = v.data_ptr()
    rc = _lib.lib().rsr_physics_param_rollouts(pa._h, C.c_void_p(raw.data_ptr()), 3, C.c_void_p(sub_ctrl.data_ptr()), C.byref(ps), K, T,
                                               pa.n_substeps, 0, C.byref(o), pa._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rsr_last_error()
    for f in ALL:
        assert_bitwise(f"{kind} raw slot 0 {f}", buf[f][0], full[f][41])
        assert_bitwise(f"{kind} raw slot 2 {f}", buf[f][2], full[f][17])
        assert (buf[f][1] == -7.25).all() and (buf[f][3] == -7.25).all(), f
    assert_bitwise(f"{kind} record after the raw call", A.record, c["before"]["record"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_applied_forces_are_the_envs_own(kind):
    c = _case(kind, True)
    assert c["pa"].xfrc_applied is not None and bool((c["pa"].xfrc_applied != 0).any())
    _check_against_replica(f"{kind} applied", c["full"], c["ref"])
    assert (c["full"]["ncon"] > 0).any()
    assert_unchanged(c["before"], c["after"])
    plain = _case(kind)                                                   # (same seeds: the same leaves and ctrl)
    assert not (c["full"]["qvel"] == plain["full"]["qvel"]).all()         # (the forces were felt)


@pytest.mark.gpu
def test_refusals_on_the_device():
    import torch
    from rsr_mjx_amd import _lib
    c = _case("cube")
    A, pa = c["A"], c["pa"]
    A.record.copy_(c["before"]["record"])
    L = _lib.lib()
    fn = L.rsr_physics_param_rollouts
    ctrl = C.c_void_p(c["ctrl"].data_ptr())
    qpos = torch.full((N, K, T, A.dims.nq), -7.25, device=A.device)
    o = _lib.RolloutOut()
    o.qpos = qpos.data_ptr()
    ok, go2_only = _lib.ParamSamples(), _lib.ParamSamples()
    ok.leaf[_lib.DR_FIELDS.index("body_mass")] = c["params"]["body_mass"].data_ptr()
    ipos = torch.zeros((N, K, A.dims.nbody, 3), device=A.device)
    go2_only.leaf[_lib.DR_FIELDS.index("body_ipos")] = ipos.data_ptr()
    nf = pa.n_substeps
    torch.cuda.synchronize()
    before = handle_snapshot(pa)
    for what, ps, flags, code in (("a Go2-only leaf", go2_only, 0, -2), ("flag bit 1", ok, 2, -1), ("flag bits", ok, 1 | 4, -1),
                                  ("negative flags", ok, -1, -1)):
        assert fn(pa._h, None, 0, ctrl, C.byref(ps), K, T, nf, flags, C.byref(o), pa._stream()) == code, what
        assert b"rsr_physics_param_rollouts" in L.rsr_last_error(), what
    for leaf in range(_lib.DR_FIELDS.index("body_ipos"), len(_lib.DR_FIELDS)):      # each of the last five, one at a time
        one = _lib.ParamSamples()
        one.leaf[leaf] = ipos.data_ptr()
        assert fn(pa._h, None, 0, ctrl, C.byref(one), K, T, nf, 0, C.byref(o), pa._stream()) == -2, _lib.DR_FIELDS[leaf]
    assert_unchanged(before, handle_snapshot(pa))
    assert (qpos == -7.25).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_rollout_loss_finds_the_candidate(kind):
    """tuning.RolloutLoss end to end: K candidate parameter rows, the target the replica batch's Physics.rollout under candidate
    j* = 3 (an existing kernel on a batch that holds those leaves): the loss is exactly 0.0 there and > 0 at every other row."""
    import torch
    from rsr_mjx_amd import tuning
    c = _base(kind)
    arr, j_star = c["envdef"].sys.arrays, 3
    if kind == "cube":                       # sliding friction of every geom, and a scale on the joint damping
        def make_leaves(P):
            fr = np.tile(arr["geom_friction"].astype(np.float32)[None], (len(P), 1, 1))
            fr[:, :, 0] = np.asarray(P, np.float32)[:, :1]
            return dict(geom_friction=fr, dof_damping=arr["dof_damping"].astype(np.float32)[None] * np.asarray(P, np.float32)[:, 1:2])
    else:                                    # sliding friction of every geom, and a scale on kp (gain and bias together)
        def make_leaves(P):
            fr = np.tile(arr["geom_friction"].astype(np.float32)[None], (len(P), 1, 1))
            fr[:, :, 0] = np.asarray(P, np.float32)[:, :1]
            kp = np.asarray(P, np.float32)[:, 1, None, None]
            return dict(geom_friction=fr, actuator_gainprm=arr["actuator_gainprm"].astype(np.float32)[None] * kp,
                        actuator_biasprm=arr["actuator_biasprm"].astype(np.float32)[None] * kp)
    P = np.stack([np.linspace(0.4, 1.1, K), np.linspace(0.85, 1.15, K)], 1)
    cand = {f: torch.as_tensor(np.ascontiguousarray(np.broadcast_to(v[None], (N,) + v.shape)), device=c["A"].device)
            for f, v in make_leaves(P).items()}
    target = _ref(c, cand, _each(c["ctrl"]))["qpos"][:, j_star]                      # [N, T, nq]
    loss = tuning.RolloutLoss(c["pa"], c["ctrl"], target, "qpos", make_leaves)
    got = loss(P)
    print(kind, "RolloutLoss over the candidates:", got)
    assert got.shape == (K,) and got[j_star] == 0.0
    assert all(got[j] > 0.0 for j in range(K) if j != j_star), got
    assert_bitwise(f"{kind} record", c["A"].record, c["before"]["record"])
