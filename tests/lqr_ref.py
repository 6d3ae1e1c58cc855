"""The LQR backward pass (rsr_physics_lqr_backward, Physics.lqr_backward) in plain numpy, and the inputs its tests share.  Not a test.

The recursion is Tassa, Erez and Todorov 2012 with the unregularised Q in the value update (include/rsr_physics.h states it line by
line); `backward` runs it at a given dtype, every product rounded to that dtype, a slot at a time.  tests/test_lqr_ref.py checks it
against the stacked finite-horizon QP, independently of the kernel.

Conditioning of `inputs`, checked on the CPU (test_lqr_ref.test_conditioning): at mu = 1e-3, M = 32, T in {1, 6, 64} and
(nx, nu) in {(40, 5), (36, 12), (28, 5)} the fp32 recursion stays within 1.4e-6 of the fp64 one on every output
(physics_support.rel, the largest value over the slots) and every |output| <= 1e3, so these inputs sit far inside the floors of
physics_support.rule (1e-5 on the p99, 1e-4 per slot) for any sane summation order."""
import numpy as np

OUTPUTS = ("gain", "k", "dV", "Vx", "Vxx")


def inputs(M, T, nx, nu, seed):
    """dict of fp32 arrays from default_rng(seed): A [M, T, nx, nx] = I + 0.3 N / sqrt(nx), B [M, T, nx, nu] = N / sqrt(nx),
    lxx [M, T+1, nx, nx] = L L^T + 0.1 I with L = N / sqrt(nx), luu [M, T, nu, nu] = R R^T + 0.5 I with R = N / sqrt(nu) (both
    symmetrised in fp32), lux [M, T, nu, nx] = 0.1 N, lx [M, T+1, nx] and lu [M, T, nu] ~ N"""
    rng = np.random.default_rng(seed)
    N = lambda *s: rng.normal(size=s)
    A = np.eye(nx) + 0.3 * N(M, T, nx, nx) / np.sqrt(nx)
    B = N(M, T, nx, nu) / np.sqrt(nx)
    L = N(M, T + 1, nx, nx) / np.sqrt(nx)
    lxx = (L @ L.transpose(0, 1, 3, 2) + 0.1 * np.eye(nx)).astype(np.float32)
    R = N(M, T, nu, nu) / np.sqrt(nu)
    luu = (R @ R.transpose(0, 1, 3, 2) + 0.5 * np.eye(nu)).astype(np.float32)
    lxx = (0.5 * (lxx + lxx.transpose(0, 1, 3, 2))).astype(np.float32)
    luu = (0.5 * (luu + luu.transpose(0, 1, 3, 2))).astype(np.float32)
    lux = 0.1 * N(M, T, nu, nx)
    lx, lu = N(M, T + 1, nx), N(M, T, nu)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(A=f(A), B=f(B), lx=f(lx), lu=f(lu), lxx=lxx, luu=luu, lux=f(lux))


def pack(A, B, stride=None, fill=0.0):
    """columns [M, T, nx + nu, stride] of A [M, T, nx, nx] and B [M, T, nx, nu]: row j holds column j of [A B] in its first nx
    entries (the layout rsr_physics_trajectory_fd writes), `fill` in the rest; stride defaults to nx"""
    M, T, nx, nu = B.shape
    stride = nx if stride is None else stride
    col = np.full((M, T, nx + nu, stride), fill, np.float32)
    col[:, :, :nx, :nx] = A.transpose(0, 1, 3, 2)
    col[:, :, nx:, :nx] = B.transpose(0, 1, 3, 2)
    return col


def backward(A, B, lx, lu, lxx, luu, lux=None, mu=0.0, state_reg=False, dtype=np.float64):
    """The recursion at `dtype`.  mu: a float or [M].  Returns gain [M, T, nu, nx], k [M, T, nu], dV [M, 2], status [M], Vx [M, T+1, nx],
    Vxx [M, T+1, nx, nx]; a slot whose Quu~ is not positive definite at step t (numpy's Cholesky refuses it, or it is not finite) stops
    there with status t and dV = 0, its rows t' <= t zeros."""
    M, T, nx, nu = B.shape
    c = lambda a: np.asarray(a, dtype)
    A, B, lx, lu, lxx, luu = c(A), c(B), c(lx), c(lu), c(lxx), c(luu)
    lux = np.zeros((M, T, nu, nx), dtype) if lux is None else c(lux)
    mu = np.broadcast_to(c(mu), (M,))
    gain, k = np.zeros((M, T, nu, nx), dtype), np.zeros((M, T, nu), dtype)
    dV, status = np.zeros((M, 2), dtype), -np.ones(M)
    Vx, Vxx = np.zeros((M, T + 1, nx), dtype), np.zeros((M, T + 1, nx, nx), dtype)
    half = dtype(0.5)
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
            try:
                if not np.isfinite(quu_r).all():
                    raise np.linalg.LinAlgError
                Lc = np.linalg.cholesky(quu_r)
            except np.linalg.LinAlgError:
                status[s], dV[s] = t, 0
                break
            solve = lambda r: np.linalg.solve(Lc.T, np.linalg.solve(Lc, r)).astype(dtype)
            kt, Kt = -solve(qu), -solve(qux_r)
            vx = qx + Kt.T @ (quu @ kt) + Kt.T @ qu + qux.T @ kt
            vxx = qxx + Kt.T @ (quu @ Kt) + Kt.T @ qux + qux.T @ Kt
            vxx = half * (vxx + vxx.T)
            dV[s, 0] += kt @ qu
            dV[s, 1] += half * (kt @ (quu @ kt))
            gain[s, t], k[s, t], Vx[s, t], Vxx[s, t] = Kt, kt, vx, vxx
    return dict(gain=gain, k=k, dV=dV, status=status, Vx=Vx, Vxx=Vxx)


_CASES = {}


def case(M, T, nx, nu, seed, mu=1e-3, state_reg=False):
    """(inputs, fp64 reference, fp32 reference) of one case, computed once and shared: the arrays are read-only"""
    key = (M, T, nx, nu, seed, mu, state_reg)
    if key not in _CASES:
        inp = inputs(M, T, nx, nu, seed)
        refs = [backward(**inp, mu=mu, state_reg=state_reg, dtype=dt) for dt in (np.float64, np.float32)]
        for group in [inp] + refs:
            for a in group.values():
                a.flags.writeable = False
        _CASES[key] = (inp, refs[0], refs[1])
    return _CASES[key]
