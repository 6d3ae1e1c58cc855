"""What rsr_mjx_amd/physics.py hands the library, call by call: each method of Physics on a stand-in without a handle, against a
library that records (tests/api_support.py).  The expectations are include/rsr_physics.h's argument lists; the kernels behind the
calls are covered by the tests/test_*_gpu.py."""
import ctypes as C

import pytest
import torch

from api_support import HANDLE as H, STREAM as S, fields, floats, ints, record, standin
from rsr_mjx_amd import _lib

NU, NQ, NV = 3, 6, 5
f32 = lambda x: C.c_float(x).value


def z(*shape, **kw):
    return torch.zeros(shape, **kw)


@pytest.fixture
def rig(monkeypatch):
    return standin(), record(monkeypatch)


def ptrs(struct, **want):
    """the members of a struct of pointers: those of `want` point at these tensors, every other one is null"""
    return fields(struct) == {n: (want[n].data_ptr() if n in want else None) for n, _ in struct._fields_}


def one(rec):
    """the one call recorded since the last look"""
    (call,), rec.calls[:] = rec.calls, []
    return call


def test_step_forward_and_set_state(rig):
    p, rec = rig
    c = z(4, NU)
    p.step(c)
    assert one(rec) == ("rsr_physics_step", (H, c.data_ptr(), 2, S))
    p.step(nsteps=5)
    assert one(rec) == ("rsr_physics_step", (H, None, 5, S))
    p.forward()
    assert one(rec) == ("rsr_physics_forward", (H, S))
    p.set_state(qpos=torch.ones(4, NQ))
    assert one(rec) == ("rsr_physics_forward", (H, S)) and bool((p.qpos == 1).all())
    p.set_state(qvel=torch.full((2, NV), 2.0), env_ids=[3, 1])
    sym, (h, ids, k, s) = one(rec)
    assert (sym, h, k, s) == ("rsr_physics_forward_envs", H, 2, S) and ints(ids, 2) == [3, 1]
    assert p.qvel[:, 0].tolist() == [0.0, 2.0, 0.0, 2.0]
    p.set_state(qpos=z(0, NQ), env_ids=[])
    assert rec.calls == []


@pytest.mark.parametrize("method, symbol", [("dynamics", "rsr_physics_dynamics"), ("constraint_forces", "rsr_physics_constraint")])
def test_env_list_ops(rig, method, symbol):
    p, rec = rig
    getattr(p, method)()
    assert one(rec) == (symbol, (H, None, 0, S))
    getattr(p, method)([1, 3])
    sym, (h, ids, k, s) = one(rec)
    assert (sym, h, k, s) == (symbol, H, 2, S) and ints(ids, 2) == [1, 3]
    getattr(p, method)([])
    assert rec.calls == []


def test_transition_fd(rig):
    p, rec = rig
    p.transition_fd()
    assert one(rec) == ("rsr_physics_transition_fd", (H, None, 0, 2, 1e-3, _lib.FD_CENTERED, S))
    p.transition_fd([3], nsteps=4, eps=1e-2, centered=False, keep_states=True)
    sym, (h, ids, k, *rest) = one(rec)
    assert (sym, h, k, rest) == ("rsr_physics_transition_fd", H, 1, [4, 1e-2, _lib.FD_STATES, S]) and ints(ids, 1) == [3]
    assert (_lib.FD_CENTERED, _lib.FD_STATES) == (1, 2)
    p.transition_fd([])
    assert rec.calls == []


def test_inverse(rig):
    p, rec = rig
    q = z(4, NV)
    p.inverse(q)
    assert one(rec) == ("rsr_physics_inverse", (H, q.data_ptr(), None, 0, 0, S))
    p.inverse(q, env_ids=[0, 2], discrete=True)
    sym, (h, qa, ids, k, flags, s) = one(rec)
    assert (sym, h, qa, k, flags, s) == ("rsr_physics_inverse", H, q.data_ptr(), 2, _lib.INV_DISCRETE, S) and ints(ids, 2) == [0, 2]
    p.inverse(q, env_ids=[])
    assert rec.calls == []


def test_rollout(rig):
    p, rec = rig
    c = z(4, 3, NU)
    res = p.rollout(c)
    sym, (h, cp, T, nsteps, out, s) = one(rec)
    assert (sym, h, cp, T, nsteps, s) == ("rsr_physics_rollout", H, c.data_ptr(), 3, 2, S) and list(res) == ["qpos", "qvel", "time"]
    assert ptrs(out, **res) and [tuple(t.shape) for t in res.values()] == [(4, 3, NQ), (4, 3, NV), (4, 3, 1)]
    mine = {"ncon": z(4, 3, 1), "actuator_force": z(4, 3, NU), "bogus": None}           # (an unknown key is ignored)
    res = p.rollout(c, nsteps=1, fields=("actuator_force", "ncon"), qpos0=torch.ones(4, NQ), out=mine)
    (first, _), (sym, (h, cp, T, nsteps, out, s)) = rec.calls
    assert first == "rsr_physics_forward" and bool((p.qpos == 1).all())                  # set_state ran first
    assert (sym, cp, T, nsteps) == ("rsr_physics_rollout", c.data_ptr(), 3, 1) and ptrs(out, **res)
    assert res["ncon"] is mine["ncon"] and res["actuator_force"] is mine["actuator_force"] and len(res) == 2
    rec.calls.clear()
    p.rollout(c, fields=())                                                              # advance, record nothing
    assert ptrs(one(rec)[1][4])


def test_sample_rollouts(rig):
    p, rec = rig
    c = z(4, 2, 3, NU)
    res = p.sample_rollouts(c)
    sym, (h, ids, k, cp, K, T, nsteps, out, s) = one(rec)
    assert (sym, h, ids, k, cp, K, T, nsteps, s) == ("rsr_physics_sample_rollouts", H, None, 0, c.data_ptr(), 2, 3, 2, S)
    assert ptrs(out, **res) and [tuple(t.shape) for t in res.values()] == [(4, 2, 3, NQ), (4, 2, 3, NV), (4, 2, 3, 1)]
    c, mine = z(2, 2, 3, NU), {"qvel": z(2, 2, 3, NV)}
    res = p.sample_rollouts(c, nsteps=7, fields=("qvel",), env_ids=[1, 0], out=mine)
    sym, (h, ids, k, cp, K, T, nsteps, out, s) = one(rec)
    assert (k, cp, K, T, nsteps) == (2, c.data_ptr(), 2, 3, 7) and ints(ids, 2) == [1, 0] and ptrs(out, qvel=mine["qvel"])
    assert res["qvel"] is mine["qvel"]
    p.sample_rollouts(z(0, 2, 3, NU), env_ids=[])
    assert rec.calls == []


def test_param_rollouts(rig):
    p, rec = rig
    c, mass, fric = z(4, 3, NU), z(4, 2, 3), z(4, 2, 6, 3)
    res = p.param_rollouts(c, dict(body_mass=mass, geom_friction=fric))
    sym, (h, ids, k, cp, ps, K, T, nsteps, flags, out, s) = one(rec)
    assert (sym, h, ids, k, cp, K, T, nsteps, flags, s) == ("rsr_physics_param_rollouts", H, None, 0, c.data_ptr(), 2, 3, 2, 0, S)
    want = [None] * len(_lib.DR_FIELDS)
    want[_lib.DR_FIELDS.index("body_mass")], want[_lib.DR_FIELDS.index("geom_friction")] = mass.data_ptr(), fric.data_ptr()
    assert list(ps.leaf) == want and ptrs(out, **res) and tuple(res["qpos"].shape) == (4, 2, 3, NQ)
    c, mine = z(1, 2, 3, NU), {"time": z(1, 2, 3, 1)}
    res = p.param_rollouts(c, None, nsteps=1, fields=("time",), env_ids=[2], out=mine)
    sym, (h, ids, k, cp, ps, K, T, nsteps, flags, out, s) = one(rec)
    assert (k, cp, K, T, nsteps, flags) == (1, c.data_ptr(), 2, 3, 1, _lib.PR_CTRL_PER_SAMPLE) and ints(ids, 1) == [2]
    assert not any(ps.leaf) and ptrs(out, time=mine["time"]) and res["time"] is mine["time"]


def test_feedback_rollouts(rig):
    p, rec = rig
    c, g, qr, vr = z(4, 2, 3, NU), z(4, 3, NU, 2 * NV), z(4, 3, NQ), z(4, 3, NV)
    res = p.feedback_rollouts(c, g, qr, vr)
    sym, (h, ids, k, cp, fb, ps, K, T, nsteps, flags, out, applied, s) = one(rec)
    assert (sym, h, ids, k, cp, K, T, nsteps, flags, applied, s) == \
        ("rsr_physics_feedback_rollouts", H, None, 0, c.data_ptr(), 2, 3, 2, _lib.FB_CTRL_PER_SAMPLE, None, S)
    assert ptrs(fb, gain=g, qpos_ref=qr, qvel_ref=vr) and not any(ps.leaf) and ptrs(out, **res)
    c, g, qr, vr, mass = z(2, 3, NU), z(2, 2, 3, NU, 2 * NV), z(2, 2, 3, NQ), z(2, 2, 3, NV), z(2, 2, 3)
    mine = {"ctrl": z(2, 2, 3, NU)}
    res = p.feedback_rollouts(c, g, qr, vr, params=dict(body_mass=mass), nsteps=4, fields=("ctrl", "qpos"), env_ids=[3, 0], clamp=True, out=mine)
    sym, (h, ids, k, cp, fb, ps, K, T, nsteps, flags, out, applied, s) = one(rec)
    assert (k, cp, K, T, nsteps, flags) == (2, c.data_ptr(), 2, 3, 4, _lib.FB_PER_SAMPLE | _lib.FB_CLAMP) and ints(ids, 2) == [3, 0]
    assert ptrs(fb, gain=g, qpos_ref=qr, qvel_ref=vr) and ps.leaf[_lib.DR_FIELDS.index("body_mass")] == mass.data_ptr()
    assert ptrs(out, qpos=res["qpos"]) and applied == mine["ctrl"].data_ptr() and res["ctrl"] is mine["ctrl"]
    assert (_lib.FB_CTRL_PER_SAMPLE, _lib.FB_PER_SAMPLE, _lib.FB_CLAMP) == (1, 2, 4)
    p.feedback_rollouts(z(4, 3, NU), z(4, 3, NU, 2 * NV), z(4, 3, NQ), z(4, 3, NV), K=2, fields=("time",))
    assert one(rec)[1][9] == 0                                                           # nothing per sample: no flag


def test_trajectory_fd(rig):
    p, rec = rig
    c, ncol, w = z(4, 3, NU), 2 * NV + NU, 2 * NV
    res = p.trajectory_fd(c)
    sym, (h, ids, k, cp, T, nsteps, eps, flags, out, s) = one(rec)
    assert (sym, h, ids, k, cp, T, nsteps, eps, flags, s) == ("rsr_physics_trajectory_fd", H, None, 0, c.data_ptr(), 3, 2, 1e-3, _lib.FD_CENTERED, S)
    assert ptrs(out, columns=res["columns"], qpos=res["qpos"], qvel=res["qvel"])
    assert [tuple(res[f].shape) for f in ("columns", "qpos", "qvel", "A", "B")] == \
        [(4, 3, ncol, w), (4, 4, NQ), (4, 4, NV), (4, 3, 2 * NV, 2 * NV), (4, 3, 2 * NV, NU)]
    c, mine = z(3, 3, NU), {"columns": z(3, 3, ncol, w)}
    res = p.trajectory_fd(c, nsteps=1, eps=1e-2, centered=False, env_ids=[1, 3, 1], nominal=False, out=mine)
    sym, (h, ids, k, cp, T, nsteps, eps, flags, out, s) = one(rec)
    assert (k, cp, T, nsteps, eps, flags) == (3, c.data_ptr(), 3, 1, 1e-2, 0) and ints(ids, 3) == [1, 3, 1]
    assert ptrs(out, columns=mine["columns"]) and res["columns"] is mine["columns"] and "qpos" not in res
    p.trajectory_fd(z(0, 3, NU), env_ids=[])
    assert rec.calls == []


def test_lqr_backward(rig):
    p, rec = rig
    M, T, nx = 6, 3, 2 * NV
    col, lx, lu, lxx, luu = z(M, T, nx + NU, nx + 2), z(M, T + 1, nx), z(M, T, NU), z(M, T + 1, nx, nx), z(M, T, NU, NU)
    res = p.lqr_backward(col, lx, lu, lxx, luu, mu=0.5)
    sym, (h, m, t, cp, w, cost, mu, flags, out, s) = one(rec)
    assert (sym, h, m, t, cp, w, flags, s) == ("rsr_physics_lqr_backward", H, M, T, col.data_ptr(), nx + 2, 0, S)
    assert ptrs(cost, lx=lx, lu=lu, lxx=lxx, luu=luu) and floats(mu, M) == [0.5] * M
    assert ptrs(out, gain=res["gain"], k=res["k"], dv=res["dV"], status=res["status"]) and list(res) == ["gain", "k", "dV", "status"]
    assert [tuple(t.shape) for t in res.values()] == [(M, T, NU, nx), (M, T, NU), (M, 2), (M,)]
    lux, mus, mine = z(M, T, NU, nx), torch.ones(M), {"Vx": z(M, T + 1, nx), "gain": z(M, T, NU, nx)}
    res = p.lqr_backward(col, lx, lu, lxx, luu, lux=lux, mu=mus, state_reg=True, values=True, out=mine)
    sym, (h, m, t, cp, w, cost, mu, flags, out, s) = one(rec)
    assert (mu, flags) == (mus.data_ptr(), _lib.LQR_REG_STATE) and ptrs(cost, lx=lx, lu=lu, lxx=lxx, luu=luu, lux=lux)
    assert ptrs(out, gain=mine["gain"], k=res["k"], dv=res["dV"], status=res["status"], vx=mine["Vx"], vxx=res["Vxx"])
    assert res["Vx"] is mine["Vx"] and res["gain"] is mine["gain"]


def test_ik(rig):
    p, rec = rig
    K8 = _lib.MAX_JAC_SITES
    pad = lambda v: list(v) + [0] * (K8 - len(v))
    tp = z(4, 2, 3)
    res = p.ik(["tip", 1], tp)
    sym, (h, ids, k, task, ins, opt, out, s) = one(rec)
    assert (sym, h, ids, k, s) == ("rsr_physics_ik", H, None, 0, S)
    assert fields(task) == dict(nsite=2, sites=pad([2, 1]), pos_weight=pad([1.0, 1.0]), rot_weight=pad([]), dofs=0b11)   # the hinge and the slide
    assert (ins.target_pos, ins.target_quat, ins.qpos0) == (tp.data_ptr(), None, None) and floats(ins.damping, 4) == [f32(1e-3)] * 4
    assert fields(opt) == dict(iters=20, tol_pos=f32(1e-4), tol_rot=f32(1e-3), max_step=f32(0.3), limits=1)
    assert ptrs(out, **res) and [(tuple(t.shape), t.dtype) for t in res.values()] == \
        [((4, NQ), torch.float32), ((4, 2), torch.float32), ((4, 2), torch.int32)] and list(res) == ["qpos", "err", "info"]
    tp, tq, q0, lam = z(3, 2, 3), z(3, 2, 4), z(3, NQ), torch.full((3,), 1e-2)
    mine = {"info": z(3, 2, dtype=torch.int32), "qpos": z(3, NQ)}
    res = p.ik(["tip", 1], tp, target_quat=tq, pos_weight=[2.0, 0.0], rot_weight=[0.25, 0.0], dofs=[4, 0], qpos0=q0, damping=lam, iters=0,
               tol_pos=0.0, tol_rot=0.5, max_step=0.0, limits=False, env_ids=[3, 3, 0], out=mine)
    sym, (h, ids, k, task, ins, opt, out, s) = one(rec)
    assert k == 3 and ints(ids, 3) == [3, 3, 0]
    assert fields(task) == dict(nsite=2, sites=pad([2, 1]), pos_weight=pad([2.0, 0.0]), rot_weight=pad([0.25, 0.0]), dofs=0b10001)
    assert ptrs(ins, target_pos=tp, target_quat=tq, qpos0=q0, damping=lam)
    assert fields(opt) == dict(iters=0, tol_pos=0.0, tol_rot=0.5, max_step=0.0, limits=0)
    assert ptrs(out, qpos=mine["qpos"], err=res["err"], info=mine["info"]) and res["info"] is mine["info"] and res["qpos"] is mine["qpos"]
    res = p.ik("tip", z(0, 1, 3), env_ids=[])                                            # M == 0: no call
    assert rec.calls == [] and tuple(res["qpos"].shape) == (0, NQ)


def test_set_jac_sites(monkeypatch):
    p, rec = standin(), record(monkeypatch, peek={"rsr_physics_set_jac_sites": lambda h, table, n: table and ints(table, n)})
    p._dyn = {}
    p.set_jac_sites(["tip", 1, "base"])
    assert [(sym, a[0], a[2]) for sym, a in rec.calls] == [("rsr_physics_set_jac_sites", H, 3)] and rec.peeked == [[2, 1, 0]] and p._dyn is None
    p.set_jac_sites(None)
    assert rec.calls[1] == ("rsr_physics_set_jac_sites", (H, None, 0))


def held(p, who, *tensors, ids_at=None):
    """`who`'s entry of the held inputs has these very tensors and, with ids_at, the int32 tensor behind that pointer"""
    entry = p._held[who]
    assert all(any(t is x for x in entry) for t in tensors), who
    if ids_at is not None:
        assert [x.dtype for x in entry if torch.is_tensor(x) and x.data_ptr() == ids_at] == [torch.int32], who
    return True


@pytest.mark.parametrize("method, ids_at", [("step", None), ("set_state", 1), ("dynamics", 1), ("constraint_forces", 1), ("transition_fd", 1),
                                            ("inverse", 2), ("rollout", None), ("sample_rollouts", 1), ("param_rollouts", 1),
                                            ("feedback_rollouts", 1), ("trajectory_fd", 1), ("lqr_backward", None), ("ik", 1)])
def test_a_launch_s_inputs_are_held_by_its_method(rig, method, ids_at):
    """The launches are asynchronous: what one reads (the caller's tensors, the tensors the wrapper made, the int32 env ids) stays
    referenced under the method's name, by identity: nothing is copied."""
    p, rec = rig
    nx = 2 * NV
    args = dict(step=[z(4, NU)], inverse=[z(4, NV)], rollout=[z(4, 3, NU)], sample_rollouts=[z(2, 2, 3, NU)],
                param_rollouts=[z(2, 3, NU), dict(body_mass=z(2, 2, 3), dof_damping=z(2, 2, NV))],
                feedback_rollouts=[z(2, 2, 3, NU), z(2, 3, NU, nx), z(2, 3, NQ), z(2, 3, NV), dict(body_mass=z(2, 2, 3))],
                trajectory_fd=[z(2, 3, NU)], lqr_backward=[z(2, 3, nx + NU, nx), z(2, 4, nx), z(2, 3, NU), z(2, 4, nx, nx), z(2, 3, NU, NU), z(2, 3, NU, nx)],
                ik=[["tip"], z(2, 1, 3), z(2, 1, 4)]).get(method, [])
    getattr(p, method)(*args, **({} if ids_at is None else {"env_ids": [3, 1]}))
    passed = rec.calls[-1][1]
    assert held(p, method, *[t for x in args for t in (x.values() if isinstance(x, dict) else [x]) if torch.is_tensor(t)],
                ids_at=None if ids_at is None else passed[ids_at])
    made = dict(lqr_backward=lambda: passed[6], ik=lambda: passed[4].damping).get(method)          # mu and damping, given as floats
    assert made is None or [x.dtype for x in p._held[method] if torch.is_tensor(x) and x.data_ptr() == made()] == [torch.float32]


def test_each_entry_point_keeps_its_own_inputs(rig):
    """Another entry point's launch may follow at once: it must not drop what the launch in flight still reads."""
    p, rec = rig
    p.dynamics([0])
    p.constraint_forces([1])
    (_, (_, a, _, _)), (_, (_, b, _, _)) = rec.calls
    assert a != b and held(p, "dynamics", ids_at=a) and held(p, "constraint_forces", ids_at=b)
    c1, c2 = z(4, NU), z(4, 2, NU)
    p.step(c1)
    p.rollout(c2)
    assert held(p, "step", c1) and held(p, "rollout", c2)
    p.dynamics([])                                                                     # no launch: the entry stays
    assert held(p, "dynamics", ids_at=a) and held(p, "rollout", c2)


def test_the_output_helper():
    p = standin()
    shape = (4, 2, 3)
    new = p._outputs("who", {"x": shape, "n": (shape, torch.int32)}, None, True)
    assert [(tuple(t.shape), t.dtype, t.device) for t in new.values()] == [(shape, torch.float32, p.qvel.device), (shape, torch.int32, p.qvel.device)]
    good = z(*shape)
    assert p._outputs("who", {"x": shape}, {"x": good}, True)["x"] is good
    for bad in (z(4, 2, 4), z(*shape).double(), z(4, 3, 2).transpose(1, 2), z(*shape, device="meta"), z(*shape).numpy()):
        for strict in (True, False):
            with pytest.raises(ValueError, match=r"who: out\['x'\] must be a contiguous float32 tensor of shape \(4, 2, 3\) on cpu"):
                p._outputs("who", {"x": shape}, {"x": bad}, strict)
    with pytest.raises(ValueError, match=r"out\['n'\] must be a contiguous int32 tensor"):
        p._outputs("who", {"n": (shape, torch.int32)}, {"n": good}, True)
    with pytest.raises(ValueError, match=r"who: out has \['y'\]; it may hold \('x',\) \(why\)"):
        p._outputs("who", {"x": shape}, {"y": good}, True, " (why)")
    assert list(p._outputs("who", {"x": shape}, {"y": good}, False)) == ["x"]
