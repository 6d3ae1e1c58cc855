"""The algorithm of rsr_physics_ik (include/rsr_physics.h) in numpy, in a chosen dtype: kinematics, site Jacobians, the damped
least-squares step, mj_integratePos and the clamp all run in that dtype, so the float32 run is an honest measure of what fp32
arithmetic costs and the float64 run is the reference.  Batched over the slots; a slot that stopped is frozen.  Also the case sets
the tests share (cases).  The Jacobian is MuJoCo's formula (axis x (point - anchor)), not the kernel's (cdof about the subtree COM):
the two agree in exact arithmetic."""
import numpy as np

FREE, SLIDE, HINGE = 0, 2, 3


def qmul(a, b):
    return np.stack([a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2],
                     a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1],
                     a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]], -1)


def q2m(q):
    w, x, y, z = (q[..., i] for i in range(4))
    two = q.dtype.type(2)
    return np.stack([np.stack([w * w + x * x - y * y - z * z, two * (x * y - w * z), two * (x * z + w * y)], -1),
                     np.stack([two * (x * y + w * z), w * w - x * x + y * y - z * z, two * (y * z - w * x)], -1),
                     np.stack([two * (x * z - w * y), two * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)


def unit(q):
    """q / |q|, the identity where |q| < 1e-15 (the kinematics' rule for a free joint's quaternion)"""
    n = np.sqrt((q * q).sum(-1, keepdims=True))
    one = np.zeros_like(q)
    one[..., 0] = 1
    return np.where(n < 1e-15, one, q / np.where(n < 1e-15, 1, n))


def rot(R, v):
    return (R * v[..., None, :]).sum(-1)


def kinematics(A, q, qpos0=None):
    """q [M, nq] in its own dtype; free-joint quaternions are normalised in place.  qpos0: [M, nq] per-slot leaf, or None: the
    model's.  Returns xpos [M, nb, 3], xquat, xmat, xanchor [M, nj, 3], xaxis."""
    dt, M = q.dtype, len(q)
    c = lambda k: np.asarray(A[k]).astype(dt)
    nb, nj = len(A["body_parentid"]), len(A["jnt_type"])
    q0 = np.broadcast_to(c("qpos0"), q.shape) if qpos0 is None else np.asarray(qpos0).astype(dt)
    xpos, xquat = np.zeros((M, nb, 3), dt), np.zeros((M, nb, 4), dt)
    xquat[:, 0, 0] = 1
    xanchor, xaxis = np.zeros((M, nj, 3), dt), np.zeros((M, nj, 3), dt)
    bpos, bquat, jpos, jaxis = c("body_pos"), c("body_quat"), c("jnt_pos"), c("jnt_axis")
    for b in range(1, nb):
        p = int(A["body_parentid"][b])
        pos = xpos[:, p] + rot(q2m(xquat[:, p]), np.broadcast_to(bpos[b], (M, 3)))
        quat = qmul(xquat[:, p], np.broadcast_to(bquat[b], (M, 4)))
        assert int(A["body_jntnum"][b]) <= 1
        for k in range(int(A["body_jntnum"][b])):
            j = int(A["body_jntadr"][b]) + k
            jt, qa = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j])
            if jt == FREE:
                q[:, qa + 3:qa + 7] = unit(q[:, qa + 3:qa + 7])
                pos, quat = q[:, qa:qa + 3].copy(), q[:, qa + 3:qa + 7].copy()
                xanchor[:, j], xaxis[:, j] = pos, np.array([0, 0, 1], dt)
            else:
                R = q2m(quat)
                anchor, axis = rot(R, np.broadcast_to(jpos[j], (M, 3))) + pos, rot(R, np.broadcast_to(jaxis[j], (M, 3)))
                xanchor[:, j], xaxis[:, j] = anchor, axis
                d = q[:, qa] - q0[:, qa]
                if jt == HINGE:
                    h = d * dt.type(0.5)
                    qloc = np.concatenate([np.cos(h)[:, None], jaxis[j][None] * np.sin(h)[:, None]], 1)
                    quat = qmul(quat, qloc)
                    pos = anchor - rot(q2m(quat), np.broadcast_to(jpos[j], (M, 3)))
                else:
                    assert jt == SLIDE
                    pos = pos + axis * d[:, None]
        xpos[:, b], xquat[:, b] = pos, quat
    return dict(xpos=xpos, xquat=xquat, xmat=q2m(xquat), xanchor=xanchor, xaxis=xaxis)


def site_frames(A, kin, sites):
    """spos [M, K, 3], smat [M, K, 3, 3] of the listed sites"""
    dt = kin["xpos"].dtype
    sb = np.asarray(A["site_bodyid"])[sites]
    sp, sq = np.asarray(A["site_pos"]).astype(dt)[sites], np.asarray(A["site_quat"]).astype(dt)[sites]
    spos = kin["xpos"][:, sb] + rot(kin["xmat"][:, sb], np.broadcast_to(sp, kin["xpos"][:, sb].shape))
    smat = q2m(qmul(kin["xquat"][:, sb], np.broadcast_to(sq, kin["xquat"][:, sb].shape)))
    return spos, smat


def site_jacobians(A, kin, sites, spos):
    """jacp, jacr [M, K, 3, nv] (mj_jacSite, world frame)"""
    dt, M = spos.dtype, len(spos)
    nv = len(A["dof_bodyid"])
    jacp, jacr = np.zeros((M, len(sites), 3, nv), dt), np.zeros((M, len(sites), 3, nv), dt)
    for k, s in enumerate(sites):
        b = int(A["site_bodyid"][s])
        while b > 0:
            for u in range(int(A["body_jntnum"][b])):
                j = int(A["body_jntadr"][b]) + u
                jt, da = int(A["jnt_type"][j]), int(A["jnt_dofadr"][j])
                if jt == FREE:
                    jacp[:, k, :, da:da + 3] = np.eye(3, dtype=dt)
                    for a in range(3):
                        ax = kin["xmat"][:, b, :, a]
                        jacr[:, k, :, da + 3 + a] = ax
                        jacp[:, k, :, da + 3 + a] = np.cross(ax, spos[:, k] - kin["xpos"][:, b])
                elif jt == HINGE:
                    jacr[:, k, :, da] = kin["xaxis"][:, j]
                    jacp[:, k, :, da] = np.cross(kin["xaxis"][:, j], spos[:, k] - kin["xanchor"][:, j])
                else:
                    jacp[:, k, :, da] = kin["xaxis"][:, j]
            b = int(A["body_parentid"][b])
    return jacp, jacr


def rotvec(Rt, R):
    """the rotation vector of Rt R^T [.., 3], angle in [0, pi]: (E - E^T) / 2 = sin(angle) [axis]x, (tr E - 1) / 2 = cos(angle)"""
    E = Rt @ np.swapaxes(R, -1, -2)
    h = E.dtype.type(0.5)
    sv = h * np.stack([E[..., 2, 1] - E[..., 1, 2], E[..., 0, 2] - E[..., 2, 0], E[..., 1, 0] - E[..., 0, 1]], -1)
    cs = h * (E[..., 0, 0] + E[..., 1, 1] + E[..., 2, 2] - 1)
    sn = np.sqrt((sv * sv).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(sn > 0, np.arctan2(sn, cs) / np.where(sn > 0, sn, 1), 0)
    return sv * f[..., None]


def errors(A, q, sites, tpos, tR, wp, wr, qpos0=None):
    """(kin, spos, e [M, K, 3], r [M, K, 3], perr [M], rerr [M]) at q (whose free quaternions get normalised)"""
    kin = kinematics(A, q, qpos0)
    spos, smat = site_frames(A, kin, sites)
    e = tpos - spos
    r = rotvec(tR, smat) if tR is not None else np.zeros_like(e)
    nrm = lambda v, w: np.where(w[None] > 0, np.sqrt((v * v).sum(-1)), 0)

    def mx(n):       # the largest norm; a NaN is kept
        out = np.zeros(len(n), n.dtype)
        for k in range(n.shape[1]):
            out = np.where(~(n[:, k] <= out), n[:, k], out)
        return out
    return kin, spos, e, r, mx(nrm(e, wp)), mx(nrm(r, wr))


def integrate_pos(A, q, dq, dofmask):
    """mj_integratePos in place on the dofs of the mask; a free joint's rotation dofs are a body-frame rotation vector"""
    dt = q.dtype
    for j in range(len(A["jnt_type"])):
        jt, qa, da = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
        if jt == FREE:
            for c in range(3):
                if dofmask[da + c]:
                    q[:, qa + c] += dq[:, da + c]
            if dofmask[da + 3:da + 6].any():
                v = dq[:, da + 3:da + 6]
                ang = np.sqrt((v * v).sum(-1))
                on = ang > 0
                h = ang * dt.type(0.5)
                with np.errstate(invalid="ignore", divide="ignore"):
                    f = np.where(on, np.sin(h) / np.where(on, ang, 1), 0)
                qn = unit(qmul(q[:, qa + 3:qa + 7], np.concatenate([np.cos(h)[:, None], v * f[:, None]], 1)))
                q[:, qa + 3:qa + 7] = np.where(on[:, None], qn, q[:, qa + 3:qa + 7])
        elif dofmask[da]:
            q[:, qa] += dq[:, da]


def clamp(A, q):
    for j in range(len(A["jnt_type"])):
        if int(A["jnt_type"][j]) in (SLIDE, HINGE) and int(A["jnt_limited"][j]):
            qa = int(A["jnt_qposadr"][j])
            lo, hi = (q.dtype.type(x) for x in A["jnt_range"][j])
            q[:, qa] = np.where(q[:, qa] < lo, lo, np.where(q[:, qa] > hi, hi, q[:, qa]))


def solve(A, dtype, sites, target_pos, target_quat, pos_weight, rot_weight, dofmask, start, damping, iters, tol_pos, tol_rot,
          max_step, limits, qpos0=None):
    """The algorithm, as the header states it.  A: the model's arrays; sites: ids; target_pos [M, K, 3]; target_quat [M, K, 4] or
    None; pos_weight, rot_weight [K]; dofmask bool [nv]; start [M, nq]; damping [M]; qpos0: the per-slot leaf or None.
    Returns qpos [M, nq], err [M, 2], info [M, 2] (iterations, status) in `dtype` / int."""
    dt = np.dtype(dtype)
    q = np.array(start, dtype=dt)
    M, nv = len(q), len(A["dof_bodyid"])
    sites = [int(s) for s in sites]
    tpos = np.asarray(target_pos).astype(dt)
    tR = None if target_quat is None else q2m(unit(np.asarray(target_quat).astype(dt)))
    wp, wr = np.asarray(pos_weight).astype(dt), np.asarray(rot_weight).astype(dt)
    lam = np.asarray(damping).astype(dt)
    dofmask = np.asarray(dofmask, bool)
    tol_pos, tol_rot, max_step = dt.type(np.float32(tol_pos)), dt.type(np.float32(tol_rot)), dt.type(np.float32(max_step))
    live = np.ones(M, bool)
    its, status = np.zeros(M, int), np.zeros(M, int)
    err = np.zeros((M, 2), dt)
    rows = [(k, h) for k in range(len(sites)) for h in (0, 1) if (wr if h else wp)[k] != 0]
    for it in range(iters + 1):
        if not live.any():
            break
        qa = q.copy()
        kin, spos, e, r, perr, rerr = errors(A, qa, sites, tpos, tR, wp, wr, qpos0)
        q[live] = qa[live]                                                  # (the normalised quaternions)
        err[live] = np.stack([perr, rerr], 1)[live]
        its[live] = it
        conv = (perr <= tol_pos) & (rerr <= tol_rot)
        stop = live & (conv | (it == iters))
        status[stop] = np.where(conv[stop], 0, 1)
        live = live & ~stop
        bad = live & ~(np.isfinite(lam) & (lam > 0))
        status[bad] = 2
        live = live & ~bad
        if not live.any():
            break
        jacp, jacr = site_jacobians(A, kin, sites, spos)
        J = np.concatenate([(wr[k] * jacr if h else wp[k] * jacp)[:, k] for k, h in rows], 1) * dofmask.astype(dt)     # [M, R, nv]
        b = np.concatenate([(wr[k] * r if h else wp[k] * e)[:, k] for k, h in rows], 1)                                 # [M, R]
        H = np.swapaxes(J, 1, 2) @ J + lam[:, None, None] * np.eye(nv, dtype=dt)
        g = (np.swapaxes(J, 1, 2) @ b[..., None])[..., 0]
        dq = np.zeros((M, nv), dt)
        for s_ in np.nonzero(live)[0]:
            with np.errstate(all="ignore"):
                try:
                    dq[s_] = np.linalg.solve(H[s_], g[s_]).astype(dt)
                except np.linalg.LinAlgError:
                    dq[s_] = np.nan
        bad = live & ~np.isfinite(dq).all(1)
        status[bad] = 2
        live = live & ~bad
        mx = np.abs(dq).max(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            sc = np.where((max_step > 0) & (mx > max_step), max_step / np.where(mx > 0, mx, 1), 1).astype(dt)
        qn = q.copy()
        integrate_pos(A, qn, np.nan_to_num(dq * sc[:, None]).astype(dt), dofmask)
        if limits:
            clamp(A, qn)
        q[live] = qn[live]
    return q, err, np.stack([its, status], 1)


# ---- the case sets

def limited(A):
    """(qposadr, mid, halfwidth) of every limited hinge / slide joint"""
    js = [j for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) in (SLIDE, HINGE) and int(A["jnt_limited"][j])]
    qa = np.array([int(A["jnt_qposadr"][j]) for j in js])
    rng = np.array([A["jnt_range"][j] for j in js], np.float64)
    return qa, rng.mean(1), 0.5 * (rng[:, 1] - rng[:, 0])


def cases(A, sites, M, seed, sig, qpos0=None, with_quat=True):
    """Reachable by construction.  start [M, nq] fp32: the model's qpos0 with every limited joint at mid + 0.5 halfwidth U(-1, 1);
    goal: the start with every limited joint moved by N(0, sig min(1, halfwidth)), clipped to 0.9 of its range; the targets are
    the fp64 forward kinematics of the goal: target_pos [M, K, 3], target_quat [M, K, 4] fp32 (site frames) and goal [M, nq]."""
    from rsr_mjx_amd.mjcf import mat_to_quat
    rng = np.random.default_rng(seed)
    qa, mid, hw = limited(A)
    start = np.tile(np.asarray(A["qpos0"], np.float64)[None], (M, 1))
    start[:, qa] = mid + 0.5 * hw * rng.uniform(-1, 1, size=(M, len(qa)))
    start = start.astype(np.float32)
    goal = start.astype(np.float64)
    goal[:, qa] = np.clip(goal[:, qa] + rng.normal(size=(M, len(qa))) * sig * np.minimum(1.0, hw), mid - 0.9 * hw, mid + 0.9 * hw)
    kin = kinematics(A, goal, qpos0)
    spos, smat = site_frames(A, kin, [int(s) for s in sites])
    tq = np.array([[mat_to_quat(smat[s, k]) for k in range(len(sites))] for s in range(M)]) if with_quat else None
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)        # (a fancy-indexed array keeps its strides through astype)
    return dict(start=start, goal=goal, target_pos=f32(spos), target_quat=None if tq is None else f32(tq))
