"""Inverse kinematics on site pose targets (rsr_physics_ik, Physics.ik) on the GPU: 4-env batches, 32 slots with repeated env ids,
four task sets (tests/test_ik_ref.py: the Airbot endpoint with and without orientation, the Go2's four feet on the twelve leg dofs,
and the Go2 whole body, imu pose and four feet on all 18 dofs: the free-joint branch and the largest J).  Against the fp64
reference after 1 and 3 iterations; convergence on the CPU-checked case sets, judged by fp64 kinematics and end to end by
set_state; limits, masks and failures; layout and independence bit for bit; nothing else written."""
import ctypes as C
import functools

import numpy as np
import pytest

import ik_ref
from physics_support import ALL_BUFFERS, assert_unchanged, handle_snapshot, make, rel, rule
from rsr_mjx_amd import prng
from test_ik_ref import ENV_IDS, ITERS, LAM, M, MAX_STEP, N, TASKS, TOL_POS, TOL_ROT, converged, task_of

KIN = 1e-5              # the project's bound on kinematic fields


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(A, E, Physics, task, cases as device tensors): a 4-env batch after a reset, per-env leaves randomised where the family's
    randomisation is its own (on Go2 it moves qpos0), shared by the tests of a task and never stepped"""
    import torch
    from rsr_mjx_amd.physics import Physics
    kind = TASKS[name][0]
    _, E, dr, _ = make(kind, N, kind != "tshape")
    E.reset(prng.split(prng.PRNGKey(1), N))
    phys = Physics(E)
    A, t, c = task_of(name)
    if t["qpos0"] is not None:
        assert np.array_equal(np.asarray(dr["qpos0"], np.float64)[ENV_IDS], t["qpos0"])         # the CPU case sets saw this leaf
    dev = phys.qvel.device
    tens = {k: None if v is None else torch.tensor(v, dtype=torch.float32, device=dev) for k, v in c.items() if k != "goal"}
    torch.cuda.synchronize()
    return A, E, phys, t, c, tens


def _call(name, slots=None, **over):
    """Physics.ik on the task's case set (or the listed slots of it), numpy results"""
    import torch
    A, E, phys, t, c, tens = _batch(name)
    sl = list(range(M)) if slots is None else list(slots)
    pick = lambda x: None if x is None else x[sl].contiguous()
    kw = dict(sites=t["sites"], target_pos=pick(tens["target_pos"]), target_quat=pick(tens["target_quat"]), pos_weight=t["pos_weight"],
              rot_weight=t["rot_weight"], dofs=t["dofmask"], qpos0=pick(tens["start"]), damping=LAM, iters=ITERS, tol_pos=TOL_POS, tol_rot=TOL_ROT,
              max_step=MAX_STEP, limits=True, env_ids=[ENV_IDS[s] for s in sl])
    kw.update(over)
    res = phys.ik(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _ref(name, dtype, **over):
    A, t, c = task_of(name)
    kw = dict(target_pos=c["target_pos"], target_quat=c["target_quat"], start=c["start"], damping=np.full(M, LAM, np.float32), iters=ITERS,
              tol_pos=TOL_POS, tol_rot=TOL_ROT, max_step=MAX_STEP, limits=True, **t)
    kw.update(over)
    return ik_ref.solve(A, dtype, **kw)


def _same_sign(A, q, ref):
    """q with every free joint's quaternion given the sign of ref's"""
    q = q.copy()
    for j in range(len(A["jnt_type"])):
        if int(A["jnt_type"][j]) == 0:
            a = int(A["jnt_qposadr"][j]) + 3
            q[:, a:a + 4] *= np.where((q[:, a:a + 4] * ref[:, a:a + 4]).sum(1, keepdims=True) < 0, -1.0, 1.0)
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TASKS))
def test_iterates_against_fp64(name):
    """After 1 and 3 iterations at lambda = 1e-2 (J^T J + lambda I then has a condition number of about 1e2 on these models), qpos
    and err against the fp64 reference under the project's rule, the fp32 reference's own distance as the spread"""
    A = _batch(name)[0]
    fails = []
    for iters in (1, 3):
        over = dict(iters=iters, tol_pos=0.0, tol_rot=0.0)
        hip = _call(name, damping=1e-2, **over)
        q64, e64, i64 = _ref(name, np.float64, damping=np.full(M, 1e-2, np.float32), **over)
        q32, e32, _ = _ref(name, np.float32, damping=np.full(M, 1e-2, np.float32), **over)
        assert (hip["info"][:, 0] == iters).all() and (i64[:, 0] == iters).all() and (hip["info"][:, 1] == 1).all()
        rule(name, f"qpos after {iters}", rel(_same_sign(A, hip["qpos"], q64), q64), rel(_same_sign(A, q32.astype(np.float64), q64), q64), fails)
        rule(name, f"err after {iters}", rel(hip["err"], e64), rel(e32, e64), fails)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TASKS))
def test_convergence_on_the_cpu_checked_cases(name):
    import torch
    A, E, phys, t, c, tens = _batch(name)
    assert (converged(name, np.float64)[2][:, 1] == 0).all()                  # the condition tests/test_ik_ref.py asserts
    hip = _call(name)
    print(name, "iterations", hip["info"][:, 0].max(), "status", np.bincount(hip["info"][:, 1]), "err", hip["err"].max(0))
    assert (hip["info"][:, 1] == 0).all() and (hip["info"][:, 0] <= ITERS).all()
    # the error at the returned qpos in fp64 (ik_ref's kinematics: mjcf.forward_kinematics to 1e-12, and it takes the qpos0 leaf)
    tR = None if c["target_quat"] is None else ik_ref.q2m(ik_ref.unit(c["target_quat"].astype(np.float64)))
    _, spos, _, _, perr, rerr = ik_ref.errors(A, hip["qpos"].astype(np.float64), t["sites"], c["target_pos"].astype(np.float64), tR,
                                              t["pos_weight"], t["rot_weight"], t["qpos0"])
    assert (perr <= TOL_POS + KIN).all() and (rerr <= TOL_ROT + KIN).all(), (perr.max(), rerr.max())
    assert np.abs(hip["err"][:, 0] - perr).max() <= KIN and np.abs(hip["err"][:, 1] - rerr).max() <= KIN
    # end to end: the batch adopts one result per env, and its own forward pass puts the sites on the targets
    first = [ENV_IDS.index(e) for e in range(N)]
    rec = E.record.clone()
    phys.set_state(qpos=torch.tensor(hip["qpos"][first], device=phys.qvel.device), env_ids=list(range(N)))
    torch.cuda.synchronize()
    sx = phys.site_xpos.cpu().numpy()[:, t["sites"]].astype(np.float64)
    on = t["pos_weight"] > 0
    d = np.sqrt(((sx - c["target_pos"][first].astype(np.float64)) ** 2).sum(-1))[:, on]
    E.record.copy_(rec)
    torch.cuda.synchronize()
    assert d.max() <= TOL_POS + KIN, d.max()


@pytest.mark.gpu
def test_limits_masks_and_failures():
    A, E, phys, t, c, tens = _batch("cube")
    nq = c["start"].shape[1]
    lim = [j for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) in (2, 3) and int(A["jnt_limited"][j])]
    qa = np.array([int(A["jnt_qposadr"][j]) for j in lim])
    lo, hi = (np.array([A["jnt_range"][j][i] for j in lim], np.float32) for i in (0, 1))
    far = tens["target_pos"] + tens["target_pos"].new_tensor([2.0, 0.0, 0.0])
    hit = _call("cube", target_pos=far, iters=12)
    assert (hit["info"][:, 1] == 1).all() and (hit["info"][:, 0] == 12).all() and np.isfinite(hit["qpos"]).all() and np.isfinite(hit["err"]).all()
    assert (hit["qpos"][:, qa] >= lo).all() and (hit["qpos"][:, qa] <= hi).all()
    assert (hit["err"][:, 0] > 1.0).all()
    # the clamp is what held them
    loose = _call("cube", target_pos=far, iters=12, limits=False)
    assert ((loose["qpos"][:, qa] < lo) | (loose["qpos"][:, qa] > hi)).any()
    # dofs outside the mask keep their start values bit for bit: the free bodies under the default mask (their quaternions come
    # back normalised), and the joints an explicit mask leaves out
    free = np.array([i for i in range(nq) if i not in set(qa.tolist())])
    quat = np.concatenate([np.arange(int(A["jnt_qposadr"][j]) + 3, int(A["jnt_qposadr"][j]) + 7) for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) == 0])
    rest = np.setdiff1d(free, quat)
    done = _call("cube")
    assert np.array_equal(done["qpos"][:, rest].view(np.int32), c["start"][:, rest].view(np.int32))
    sq = c["start"][:, quat].reshape(M, -1, 4).astype(np.float64)
    assert np.abs(done["qpos"][:, quat].reshape(M, -1, 4) - sq / np.linalg.norm(sq, axis=-1, keepdims=True)).max() <= 1e-6
    some = _call("cube", dofs=[0, 1, 2], iters=6)
    kept = np.setdiff1d(np.arange(nq), np.concatenate([qa[:3], quat]))
    assert np.array_equal(some["qpos"][:, kept].view(np.int32), c["start"][:, kept].view(np.int32))
    assert (some["qpos"][:, qa[:3]] != c["start"][:, qa[:3]]).any()
    # a damping that is not finite and positive ends its slot alone
    import torch
    lam = torch.full((M,), LAM, dtype=torch.float32, device=tens["start"].device)
    lam[3], lam[5] = 0.0, float("nan")
    bad, start = _call("cube", damping=lam), _call("cube", iters=0)
    ok = np.ones(M, bool)
    ok[[3, 5]] = False
    assert (bad["info"][~ok, 1] == 2).all() and (bad["info"][~ok, 0] == 0).all()
    assert np.array_equal(bad["qpos"][~ok].view(np.int32), start["qpos"][~ok].view(np.int32))
    for f in ("qpos", "err", "info"):
        assert np.array_equal(bad[f][ok].view(np.int32), done[f][ok].view(np.int32)), f


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "go2whole"])
def test_layout_and_independence_bit_for_bit(name):
    import torch
    from rsr_mjx_amd import _lib
    A, E, phys, t, c, tens = _batch(name)
    full = _call(name, iters=5)
    again = _call(name, iters=5)
    slots = [17, 2, 30, 2, 9]
    part = _call(name, slots=slots, iters=5)
    for f in ("qpos", "err", "info"):
        assert np.array_equal(full[f].view(np.int32), again[f].view(np.int32)), f
        assert np.array_equal(part[f].view(np.int32), full[f][slots].view(np.int32)), f
    # qpos0 = None is the record's qpos; iters = 0 returns the start and the error site_xpos implies
    rec = E.record.clone()
    first = [ENV_IDS.index(e) for e in range(N)]
    phys.set_state(qpos=tens["start"][first], env_ids=list(range(N)))
    torch.cuda.synchronize()
    own = _call(name, qpos0=None, iters=5)
    given = _call(name, qpos0=phys.qpos[ENV_IDS].contiguous(), iters=5)
    query = _call(name, qpos0=None, iters=0)
    sx = phys.site_xpos.cpu().numpy()[ENV_IDS][:, t["sites"]].astype(np.float64)
    qrec = phys.qpos.cpu().numpy()[ENV_IDS]
    E.record.copy_(rec)
    torch.cuda.synchronize()
    for f in ("qpos", "err", "info"):
        assert np.array_equal(own[f].view(np.int32), given[f].view(np.int32)), f
    assert (query["info"][:, 0] == 0).all() and np.abs(_same_sign(A, query["qpos"], qrec) - qrec).max() <= 1e-6
    d = np.sqrt(((sx - c["target_pos"].astype(np.float64)) ** 2).sum(-1))[:, t["pos_weight"] > 0].max(1)
    assert np.abs(query["err"][:, 0] - d).max() <= KIN
    # an id out of range leaves its slot's rows alone (Physics.ik refuses one: the C call itself)
    dev = tens["start"].device
    ids = [1, 99, 0, -1]
    raw = torch.tensor(ids, dtype=torch.int32, device=dev)
    qp = torch.full((4, c["start"].shape[1]), float("nan"), device=dev)
    er = torch.full((4, 2), float("nan"), device=dev)
    nf = torch.full((4, 2), -7, dtype=torch.int32, device=dev)
    K = len(t["sites"])
    task = _lib.IkTask(nsite=K, dofs=int(sum(1 << i for i in np.nonzero(t["dofmask"])[0])))
    for k in range(K):
        task.sites[k], task.pos_weight[k], task.rot_weight[k] = t["sites"][k], float(t["pos_weight"][k]), float(t["rot_weight"][k])
    sl = [ENV_IDS.index(1), 0, ENV_IDS.index(0), 1]
    tp, st = tens["target_pos"][sl].contiguous(), tens["start"][sl].contiguous()
    tq = None if tens["target_quat"] is None else tens["target_quat"][sl].contiguous()
    lam = torch.full((4,), LAM, device=dev)
    ins = _lib.IkIn(tp.data_ptr(), None if tq is None else tq.data_ptr(), st.data_ptr(), lam.data_ptr())
    opt, out = _lib.IkOpt(5, TOL_POS, TOL_ROT, MAX_STEP, 1), _lib.IkOut(qp.data_ptr(), er.data_ptr(), nf.data_ptr())
    rc = _lib.lib().rsr_physics_ik(phys._h, C.c_void_p(raw.data_ptr()), 4, C.byref(task), C.byref(ins), C.byref(opt), C.byref(out), phys._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().rsr_last_error()
    for s in (1, 3):
        assert torch.isnan(qp[s]).all() and torch.isnan(er[s]).all() and bool((nf[s] == -7).all())
    for s in (0, 2):
        assert np.array_equal(qp[s].cpu().numpy().view(np.int32), full["qpos"][sl[s]].view(np.int32))
        assert np.array_equal(nf[s].cpu().numpy(), full["info"][sl[s]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tshape", "go2legs"])
def test_nothing_else_is_written(name):
    A, E, phys, t, c, tens = _batch(name)
    before = handle_snapshot(phys, ALL_BUFFERS)
    _call(name)
    _call(name, qpos0=None, iters=3)
    assert_unchanged(before, handle_snapshot(phys, ALL_BUFFERS))
