"""The control-limited LQR backward pass (rsr_physics_lqr_box, Physics.lqr_backward_box) in plain numpy, and the bounds its tests
share.  Not a test.

`backward_box` is lqr_ref.backward with k_t the minimiser of the step's box-constrained QP (Tassa, Mansard and Todorov 2014) by the
projected Newton iteration include/rsr_physics.h states line by line, at a given dtype, a slot at a time; with infinite bounds it
runs the very numpy calls of lqr_ref.backward and returns its bits.  `kkt` is the optimality residual of one QP, independent of the
iteration.  tests/test_lqr_box_ref.py checks the reference and the conditioning of the shared inputs on the CPU.

Conditioning of `bounds` on lqr_ref.inputs(32, T, nx, nu, 100 + T), mu = 1e-3, seed 700 + T (test_lqr_box_ref.test_conditioning):
fp32 and fp64 take the same clamped set and end with the same code at every step of every slot, and every slot's smallest margin
(below) is >= 1e-4, so a kernel whose fp32 sums differ from numpy's in the last bits takes the same branches."""
import numpy as np

import lqr_ref

TRIALS, SHRINK, ARMIJO = 20, 0.6, 0.1
# The directed case of the tests: backtrack_inputs(32, 6, nx, nu, 1) with bounds(32, 6, nu, 801).  Of the seeds 0 .. 3, searched on the
# CPU, seed 1 has the widest margins: at (40, 5), (36, 12), (28, 5) the line search shrinks the step 54, 252 and 39 times, fp32 and
# fp64 agree on every set and code, and the smallest margins are 4.3e-4, 5.8e-4 and 3.5e-3.
BACKTRACK = dict(T=6, seed=1, bseed=801)


def bounds(M, T, nu, seed):
    """(lo, hi) fp32 [M, T, nu] from default_rng(seed), drawn in this order: lo = -U(0.1, 1), hi = U(0.1, 1), u = U(0, 1),
    l2 = U(0.05, 0.3), h2 = l2 + U(0.1, 1); where 0.15 <= u < 0.20 the box is (l2, h2), so that zero is infeasible; where u < 0.15
    it is (-inf, +inf)."""
    rng = np.random.default_rng(seed)
    U = lambda a, b: rng.uniform(a, b, size=(M, T, nu))
    lo, hi, u = -U(0.1, 1), U(0.1, 1), U(0, 1)
    l2 = U(0.05, 0.3)
    h2 = l2 + U(0.1, 1)
    shifted, free = (u >= 0.15) & (u < 0.20), u < 0.15
    lo, hi = np.where(shifted, l2, lo), np.where(shifted, h2, hi)
    lo, hi = np.where(free, -np.inf, lo), np.where(free, np.inf, hi)
    return np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(hi, np.float32)


def backtrack_inputs(M, T, nx, nu, seed):
    """lqr_ref.inputs(M, T, nx, nu, seed) with luu = R R^T + 0.01 I, R = N + 3 (1 1^T) / sqrt(nu): a strong coupling between the
    controls, under which a clipped Newton step often overshoots and the line search has to shrink it"""
    inp = dict(lqr_ref.inputs(M, T, nx, nu, seed))
    rng = np.random.default_rng(seed + 5000)
    R = (rng.normal(size=(M, T, nu, nu)) + 3.0) / np.sqrt(nu)
    luu = R @ R.transpose(0, 1, 3, 2) + 0.01 * np.eye(nu)
    inp["luu"] = (0.5 * (luu + luu.transpose(0, 1, 3, 2))).astype(np.float32)
    return inp


def kkt(H, g, l, h, x):
    """The largest violation of the optimality conditions of min 1/2 x^T H x + g^T x, l <= x <= h, at x: feasibility, a zero
    gradient where l < x < h, a gradient >= 0 at x = l < h and <= 0 at x = h > l.  With H positive definite on the free set these
    are sufficient."""
    H, g, l, h, x = (np.asarray(a, np.float64) for a in (H, g, l, h, x))
    grad = g + H @ x
    feas = np.maximum(np.maximum(l - x, x - h), 0.0)
    at_l, at_h = x == l, x == h
    free = ~at_l & ~at_h
    res = np.where(free, np.abs(grad), 0.0)
    res = np.where(at_l & ~at_h, np.maximum(-grad, 0.0), res)
    res = np.where(at_h & ~at_l, np.maximum(grad, 0.0), res)
    return float(max(feas.max(), res.max()))


def _clip(v, l, h):
    return np.where(v < l, l, np.where(v > h, h, v))


def _qp(H, g, l, h, max_iter, dtype, chol):
    """One step's QP.  Returns x, c (the last clamped set), grad, steps, code, the factor of the last c (None: code 1), and what the
    census counts: (clipped start, line searches run, line searches that shrank the step, a control clamped on the way and free
    at the end).  Raises LinAlgError at a bad pivot."""
    nu = g.shape[0]
    half, shrink, armijo = dtype(0.5), dtype(SHRINK), dtype(ARMIJO)
    f = lambda z: ((half * (H @ z) + g) * z).sum(dtype=dtype)
    x = _clip(np.zeros(nu, dtype), l, h).astype(dtype)
    clipped_start = bool((x != 0).any())
    full, c_prev, L, c_fac = False, None, None, None
    searches = shrunk = 0
    ever = np.zeros(nu, bool)
    it = 0
    while True:
        grad = (g + H @ x).astype(dtype)
        c = ((x == l) & (grad > 0)) | ((x == h) & (grad < 0))
        ever |= c
        if c.all():
            code = 1
            break
        if full and (c == c_prev).all():
            code = 0
            break
        if it == max_iter:
            code = 2
            break
        Hm = H.copy()
        Hm[c, :], Hm[:, c] = 0, 0
        Hm[c, c] = 1
        L, c_fac = chol(Hm), c
        r = np.where(c, dtype(0), g + H[:, c] @ x[c]).astype(dtype)
        y = -np.linalg.solve(L.T, np.linalg.solve(L, r)).astype(dtype)
        xs = np.where(c, x, y)
        d = (xs - x).astype(dtype)
        c_prev = c
        it += 1
        xn = (x + d).astype(dtype)
        if ((l <= xn) & (xn <= h)).all():
            x, full = xs, True
            continue
        full = False
        searches += 1
        f0, a, taken = f(x), dtype(1), False
        for n in range(TRIALS):
            z = _clip((x + a * d).astype(dtype), l, h).astype(dtype)
            if f0 - f(z) >= armijo * (grad @ (x - z)):
                taken = True
                break
            a = dtype(a * shrink)
        if not taken:
            it -= 1                                   # (the step that was not taken is not counted)
            code = 3
            break
        shrunk += n > 0
        x = z
    if code != 1 and (c_fac is None or (c != c_fac).any()):
        Hm = H.copy()
        Hm[c, :], Hm[:, c] = 0, 0
        Hm[c, c] = 1
        L = chol(Hm)
    x = np.where(c, np.where(grad > 0, l, h), x).astype(dtype)
    return x, c, grad, it, code, (None if code == 1 else L), (clipped_start, searches, shrunk, bool((ever & ~c).any()))


def backward_box(A, B, lx, lu, lxx, luu, lo, hi, lux=None, mu=0.0, state_reg=False, max_iter=32, dtype=np.float64):
    """lqr_ref.backward with lo <= k_t <= hi.  Returns its dict and clamped [M, T, nu] (-1 at lo, +1 at hi, 0 free), qp [M, T, 2]
    (Newton steps, code), margin [M, T] (the smaller of the smallest |grad_j| over the clamped j and the smallest distance of a free
    x_j to its bounds: how far the step is from another set of clamped controls) and census [M, T, 4] (clipped start, line searches
    run, line searches that shrank the step, a control clamped on the way and free at the end).  A slot whose bounds at step t are
    not ordered (a NaN included), or whose masked Quu~ is not positive definite there, stops with status t and dV = 0."""
    M, T, nx, nu = B.shape
    c_ = lambda a: np.asarray(a, dtype)
    A, B, lx, lu, lxx, luu, lo, hi = c_(A), c_(B), c_(lx), c_(lu), c_(lxx), c_(luu), c_(lo), c_(hi)
    lux = np.zeros((M, T, nu, nx), dtype) if lux is None else c_(lux)
    mu = np.broadcast_to(c_(mu), (M,))
    gain, k = np.zeros((M, T, nu, nx), dtype), np.zeros((M, T, nu), dtype)
    dV, status = np.zeros((M, 2), dtype), -np.ones(M)
    Vx, Vxx = np.zeros((M, T + 1, nx), dtype), np.zeros((M, T + 1, nx, nx), dtype)
    clamped, qp = np.zeros((M, T, nu), dtype), np.zeros((M, T, 2), dtype)
    margin, census = np.full((M, T), np.inf), np.zeros((M, T, 4), int)
    half = dtype(0.5)

    def chol(Hm):
        if not np.isfinite(Hm).all():
            raise np.linalg.LinAlgError
        return np.linalg.cholesky(Hm)

    for s in range(M):
        vx, vxx = lx[s, T], lxx[s, T]
        Vx[s, T], Vxx[s, T] = vx, vxx
        for t in range(T - 1, -1, -1):
            a, b = A[s, t], B[s, t]
            qx, qu = lx[s, t] + a.T @ vx, lu[s, t] + b.T @ vx
            w = vxx @ a
            qxx, qux, quu = lxx[s, t] + a.T @ w, lux[s, t] + b.T @ w, luu[s, t] + b.T @ (vxx @ b)
            if state_reg:
                quu_r, qux_r = quu + mu[s] * (b.T @ b), qux + mu[s] * (b.T @ a)
            else:
                quu_r, qux_r = quu + mu[s] * np.eye(nu, dtype=dtype), qux
            l, h = lo[s, t], hi[s, t]
            try:
                if not (l <= h).all():
                    raise np.linalg.LinAlgError
                kt, c, grad, steps, code, Lc, cen = _qp(quu_r, qu, l, h, max_iter, dtype, chol)
            except np.linalg.LinAlgError:
                status[s], dV[s] = t, 0
                break
            if code == 1:
                Kt = np.zeros((nu, nx), dtype)
            else:
                solve = lambda r: np.linalg.solve(Lc.T, np.linalg.solve(Lc, r)).astype(dtype)
                Kt = -solve(np.where(c[:, None], dtype(0), qux_r) if c.any() else qux_r)
                Kt[c] = 0
            vx = qx + Kt.T @ (quu @ kt) + Kt.T @ qu + qux.T @ kt
            vxx = qxx + Kt.T @ (quu @ Kt) + Kt.T @ qux + qux.T @ Kt
            vxx = half * (vxx + vxx.T)
            dV[s, 0] += kt @ qu
            dV[s, 1] += half * (kt @ (quu @ kt))
            gain[s, t], k[s, t], Vx[s, t], Vxx[s, t] = Kt, kt, vx, vxx
            clamped[s, t] = np.where(c, np.where(grad > 0, -1, 1), 0)
            qp[s, t] = steps, code
            free = ~c
            dist = np.minimum(kt - l, h - kt)[free]
            margin[s, t] = min(np.abs(grad[c]).min() if c.any() else np.inf, dist.min() if free.any() else np.inf)
            census[s, t] = cen
    return dict(gain=gain, k=k, dV=dV, status=status, Vx=Vx, Vxx=Vxx, clamped=clamped, qp=qp, margin=margin, census=census)


_CASES = {}


def case(M, T, nx, nu, seed, bseed, mu=1e-3, state_reg=False, max_iter=32, directed=False):
    """(inputs with lo and hi, fp64 reference, fp32 reference) of one case, computed once and shared: the arrays are read-only.
    directed: backtrack_inputs in place of lqr_ref.inputs."""
    key = (M, T, nx, nu, seed, bseed, mu, state_reg, max_iter, directed)
    if key not in _CASES:
        inp = dict((backtrack_inputs if directed else lqr_ref.inputs)(M, T, nx, nu, seed))
        inp["lo"], inp["hi"] = bounds(M, T, nu, bseed)
        refs = [backward_box(**inp, mu=mu, state_reg=state_reg, max_iter=max_iter, dtype=dt) for dt in (np.float64, np.float32)]
        for group in [inp] + refs:
            for a in group.values():
                a.flags.writeable = False
        _CASES[key] = (inp, refs[0], refs[1])
    return _CASES[key]
