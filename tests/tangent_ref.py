"""mj_integratePos / mj_differentiatePos in fp64 numpy on a model's arrays (free joints, hinges and slides): the reference that
tests/test_transition_gpu.py holds the kernels' perturbations and columns to and tests/test_feedback_gpu.py the control law's state
error.  tests/test_tangent_ref.py checks the functions against each other on the CPU."""
import numpy as np


def columns(A, nv):
    """per qpos-tangent column k < nv: (kind, qpos address): 'add' at one address, or 'rot' about axis k' of the quaternion at it"""
    cols = [None] * nv
    for j in range(len(A["jnt_type"])):
        jt, qa, da = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
        if jt == 0:
            for k in range(3):
                cols[da + k] = ("add", qa + k, 0)
                cols[da + 3 + k] = ("rot", qa + 3, k)
        else:
            assert jt in (2, 3)
            cols[da] = ("add", qa, 0)
    assert all(c is not None for c in cols)
    return cols


def qmul(a, b):
    """Hamilton product.  Every vector component sums its two w terms first, then its cross pair: in conj(q) q each pair cancels
    exactly, so differentiate_pos(q, q) is 0 and not a rounding residue of 1e-17."""
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0)
    w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 + y1 * w2 - x1 * z2 + z1 * x2, w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2], -1)


def integrate_pos(A, nv, qpos, k, dlt):
    """mj_integratePos(qpos, dlt e_k) in fp64 on [n, nq]"""
    q = np.array(qpos, dtype=np.float64)
    kind, qa, ax = columns(A, nv)[k]
    if kind == "add":
        q[:, qa] += dlt
    else:
        r = np.zeros(4); r[0] = np.cos(0.5 * dlt); r[1 + ax] = np.sin(0.5 * dlt)
        p = qmul(q[:, qa:qa + 4], r[None])
        q[:, qa:qa + 4] = p / np.linalg.norm(p, axis=1, keepdims=True)
    return q


def moved(A, nv, qpos, d):
    """qpos [n, nq] moved by d [n, nv] in the tangent space: joints and free-joint translations add, a free joint's quaternion is
    multiplied on the right by the rotation vector's quaternion and renormalised"""
    q = np.array(qpos, dtype=np.float64)
    for k, (kind, qa, ax) in enumerate(columns(A, nv)):
        if kind == "add":
            q[:, qa] += d[:, k]
        elif ax == 0:
            v = d[:, k:k + 3]
            ang = np.linalg.norm(v, axis=1, keepdims=True)
            r = np.concatenate([np.cos(0.5 * ang), np.sin(0.5 * ang) * v / np.maximum(ang, 1e-300)], 1)
            p = qmul(q[:, qa:qa + 4], r)
            q[:, qa:qa + 4] = p / np.linalg.norm(p, axis=1, keepdims=True)
    return q


def differentiate_pos(A, nv, qp, qm):
    """mj_differentiatePos with dt = 1, fp64: qp (-) qm on [n, nq] -> [n, nv]"""
    qp, qm = np.asarray(qp, np.float64), np.asarray(qm, np.float64)
    out = np.zeros((len(qp), nv))
    for k, (kind, qa, ax) in enumerate(columns(A, nv)):
        if kind == "add":
            out[:, k] = qp[:, qa] - qm[:, qa]
        elif ax == 0:
            conj = qm[:, qa:qa + 4] * np.array([1.0, -1.0, -1.0, -1.0])
            dq = qmul(conj, qp[:, qa:qa + 4])
            sn = np.linalg.norm(dq[:, 1:], axis=1)
            speed = 2.0 * np.arctan2(sn, dq[:, 0])
            speed = np.where(speed > np.pi, speed - 2.0 * np.pi, speed)
            out[:, k:k + 3] = dq[:, 1:] * np.where(sn > 0, speed / np.where(sn > 0, sn, 1.0), 0.0)[:, None]
    return out
