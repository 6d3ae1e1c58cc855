"""The numpy reference of the inverse-kinematics call (tests/ik_ref.py), on the CPU: its kinematics and Jacobians against mjcf.py's,
J dq against the change of the errors under mj_integratePos, and the two conditions on the case sets that tests/test_ik_gpu.py
relies on: every case converges in fp64 within 30 iterations, and the fp32 run takes the same number of iterations on at least
90 % of them."""
import functools

import numpy as np
import pytest

import ik_ref
from model_variants import envdef_of
from rsr_mjx_amd import mjcf

# the convergence recipe; of the seeds 200 .. 215 about two in three give case sets on which every case converges (a case that does
# not sits at a joint limit or in a local minimum of the clamped iteration): the seeds below are among those, and the test asserts it
SIG, LAM, MAX_STEP, WR, TOL_POS, TOL_ROT, ITERS, WITHIN = 0.2, 1e-3, 0.3, 0.2, 1e-4, 1e-3, 40, 30
M, N = 32, 4
ENV_IDS = [(3 * i + i // 7) % N for i in range(M)]           # the env of every slot of the GPU tests: each env many times
# name: (family, sites, orientation rows, dofs: None = hinge and slide, or a list, seed)
TASKS = {"cube": ("cube", ["endpoint"], True, None, 201), "tshape": ("tshape", ["endpoint"], False, None, 201),
         "go2legs": ("go2flat", ["FR", "FL", "RR", "RL"], False, list(range(6, 18)), 202),
         "go2whole": ("go2flat", ["imu", "FR", "FL", "RR", "RL"], True, list(range(18)), 203)}


def leaf_qpos0(kind):
    """[M, nq]: the qpos0 leaf of every slot's env in the GPU tests' batches (physics_support.make with randomisation on: the Go2
    randomisation moves qpos0, and with it the kinematics), or None where the family has no such leaf"""
    if not kind.startswith("go2"):
        return None
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import go2
    return go2.domain_randomize(envdef_of(kind, None).sys, prng.split(prng.PRNGKey(12), N))["qpos0"][ENV_IDS].astype(np.float64)


def task_of(name, seed=None):
    """(A, dict of solve()'s task arguments, case set) of a TASKS entry: orientation rows on the first site only (weight WR)"""
    kind, names, quat, dofs, seed0 = TASKS[name]
    sysm = envdef_of(kind, None).sys
    qpos0 = leaf_qpos0(kind)
    A = sysm.arrays
    sites = [int(sysm.id("site", n)) for n in names]
    nv = len(A["dof_bodyid"])
    mask = np.zeros(nv, bool)
    mask[[int(A["jnt_dofadr"][j]) for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) in (2, 3)] if dofs is None else dofs] = True
    wp, wr = np.ones(len(sites)), np.zeros(len(sites))
    if quat:
        wr[0] = WR
    c = ik_ref.cases(A, sites, M, seed0 if seed is None else seed, SIG, qpos0=qpos0, with_quat=quat)
    return A, dict(sites=sites, pos_weight=wp, rot_weight=wr, dofmask=mask, qpos0=qpos0), c


@functools.lru_cache(maxsize=None)
def converged(name, dtype):
    A, t, c = task_of(name)
    return ik_ref.solve(A, dtype, target_pos=c["target_pos"], target_quat=c["target_quat"], start=c["start"],
                        damping=np.full(M, LAM, np.float32), iters=ITERS, tol_pos=TOL_POS, tol_rot=TOL_ROT, max_step=MAX_STEP,
                        limits=True, **t)


@pytest.mark.parametrize("kind", ["cube", "tshape", "go2flat"])
def test_kinematics_and_jacobians_agree_with_mjcf(kind):
    sysm = envdef_of(kind, None).sys
    A = sysm.arrays
    sites = list(range(sysm.nsite))
    rng = np.random.default_rng(1)
    q = np.tile(np.asarray(A["qpos0"], np.float64)[None], (3, 1)) + rng.normal(size=(3, sysm.nq)) * 0.2
    kin = ik_ref.kinematics(A, q)                   # (normalises the free quaternions of q)
    spos, smat = ik_ref.site_frames(A, kin, sites)
    jacp, jacr = ik_ref.site_jacobians(A, kin, sites, spos)
    for s in range(3):
        k0 = mjcf.forward_kinematics(sysm, q[s])
        for f in ("xpos", "xmat", "xanchor", "xaxis"):
            assert np.abs(kin[f][s] - k0[f]).max() < 1e-12, f
        for k, site in enumerate(sites):
            b = int(A["site_bodyid"][site])
            p0 = k0["xpos"][b] + k0["xmat"][b] @ A["site_pos"][site]
            R0 = mjcf.quat_to_mat(mjcf.quat_mul(k0["xquat"][b], A["site_quat"][site]))
            assert np.abs(spos[s, k] - p0).max() < 1e-12 and np.abs(smat[s, k] - R0).max() < 1e-12
            jp, jr = mjcf.body_jacobian(sysm, k0, p0, b)
            assert np.abs(jacp[s, k] - jp).max() < 1e-12 and np.abs(jacr[s, k] - jr).max() < 1e-12


@pytest.mark.parametrize("name", ["cube", "go2whole"])
def test_J_dq_predicts_the_change_of_the_errors(name):
    """d(e, r) / d dq = -J at the iterate, by central differences through integrate_pos: hinge, slide and all six free-joint dofs
    (the free joint's rotation dofs are a body-frame rotation vector)"""
    A, t, c = task_of(name)
    sites, nv = t["sites"], len(A["dof_bodyid"])
    every = np.ones(nv, bool)
    q = c["start"][:2].astype(np.float64)
    tp = c["target_pos"][:2].astype(np.float64)
    tR = ik_ref.q2m(ik_ref.unit(c["target_quat"][:2].astype(np.float64)))
    one = np.ones(len(sites))
    q0 = None if t["qpos0"] is None else t["qpos0"][:2]
    kin, spos, e, r, _, _ = ik_ref.errors(A, q, sites, tp, tR, one, one, q0)
    jacp, jacr = ik_ref.site_jacobians(A, kin, sites, spos)
    h = 1e-6
    kinds = set()
    for i in range(nv):
        d = np.zeros((2, nv))
        d[:, i] = h
        qp, qm = q.copy(), q.copy()
        ik_ref.integrate_pos(A, qp, d, every)
        ik_ref.integrate_pos(A, qm, -d, every)
        _, _, ep, rp, _, _ = ik_ref.errors(A, qp, sites, tp, tR, one, one, q0)
        _, _, em, rm, _, _ = ik_ref.errors(A, qm, sites, tp, tR, one, one, q0)
        assert np.abs((ep - em) / (2 * h) + jacp[..., i]).max() < 1e-7, i
        # the rotation error is a rotation vector: log(exp(r) exp(-w)) = r - (I + [r]x / 2 + c [r]x^2) w + O(w^2), the inverse of
        # SO(3)'s right Jacobian, c = 1 / th^2 - (1 + cos th) / (2 th sin th), th = |r| (1 / 12 at r = 0)
        w = jacr[..., i]
        th = np.maximum(np.sqrt((r * r).sum(-1, keepdims=True)), 1e-4)
        cc = 1 / th ** 2 - (1 + np.cos(th)) / (2 * th * np.sin(th))
        want = -(w + 0.5 * np.cross(r, w) + cc * np.cross(r, np.cross(r, w)))
        assert np.abs((rp - rm) / (2 * h) - want).max() < 1e-6, i
        kinds.add(int(A["jnt_type"][int(A["dof_jntid"][i])]))
    assert kinds == ({0, 2, 3} if name == "cube" else {0, 3})


@pytest.mark.parametrize("name", list(TASKS))
def test_every_case_converges_in_fp64_and_fp32_takes_the_same_iterations(name):
    q64, err64, info64 = converged(name, np.float64)
    print(name, "fp64 iterations max", info64[:, 0].max(), "status", np.bincount(info64[:, 1]))
    assert (info64[:, 1] == 0).all() and (info64[:, 0] <= WITHIN).all()
    assert (err64[:, 0] <= TOL_POS).all() and (err64[:, 1] <= TOL_ROT).all()
    q32, err32, info32 = converged(name, np.float32)
    same = (info32[:, 0] == info64[:, 0]).mean()
    print(name, "fp32 takes the fp64 iteration count on %.0f %% of the cases" % (100 * same))
    assert same >= 0.9
    assert q32.dtype == np.float32 and err32.dtype == np.float32


def test_failures_and_queries():
    """iters = 0 is a query; a damping that is not finite and positive ends its slot with status 2 at the start, the others as before"""
    A, t, c = task_of("cube")
    kw = dict(target_pos=c["target_pos"], target_quat=c["target_quat"], start=c["start"], tol_pos=TOL_POS, tol_rot=TOL_ROT,
              max_step=MAX_STEP, limits=True, **t)
    lam = np.full(M, LAM, np.float32)
    q, err, info = ik_ref.solve(A, np.float64, damping=lam, iters=0, **kw)
    assert (info[:, 0] == 0).all() and (info[:, 1] == 1).all() and np.array_equal(q.astype(np.float32)[:, :8], c["start"][:, :8])
    bad = lam.copy()
    bad[3], bad[5] = 0.0, np.nan
    q2, _, info2 = ik_ref.solve(A, np.float64, damping=bad, iters=5, **kw)
    q1, _, info1 = ik_ref.solve(A, np.float64, damping=lam, iters=5, **kw)
    ok = np.ones(M, bool)
    ok[[3, 5]] = False
    assert (info2[~ok, 1] == 2).all() and (info2[~ok, 0] == 0).all() and np.array_equal(q2[~ok], q[~ok])
    assert np.array_equal(q2[ok], q1[ok]) and np.array_equal(info2[ok], info1[ok])
