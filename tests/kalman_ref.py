"""The Kalman filter and RTS smoother (rsr_physics_kalman, Physics.kalman_smooth) in plain numpy, and the inputs its tests share.
Not a test.

`smooth` runs the recursion include/rsr_physics.h states line by line at a given dtype, every product rounded to that dtype: the
measurement update one sensor entry at a time, ascending (R is diagonal), the predict symmetrised, the smoother on the Cholesky
factor of the predicted covariance.  The M slots run side by side (the arrays carry a leading M); a slot that fails stops alone.
tests/test_kalman_ref.py checks it against the stacked weighted least-squares problem, independently of the kernel.

Conditioning of `inputs`, checked on the CPU (test_kalman_ref.test_conditioning): every innovation variance s >= r >= 0.1 and every
Cholesky pivot of Pm >= min q = 0.01 while |P| stays of order 1, so neither is near zero in fp32, and the fp32 recursion stays far
inside the floors of physics_support.rule (1e-5 on the p99, 1e-4 per slot)."""
import numpy as np

OUTPUTS = ("xf", "Pf", "xs", "Ps", "nll")
LOG_2PI = float(np.log(2.0 * np.pi))


def inputs(M, T, nx, ny, seed):
    """dict of fp32 arrays from default_rng(seed): A [M, T, nx, nx] = 0.8 I + 0.2 N / sqrt(nx) (spectral radius about 1 at most, so
    the covariance stays of order 1 over 64 steps), C [M, T, ny, nx] = N / sqrt(nx), dy [M, T, ny] ~ N, r [M, T, ny] ~ U(0.1, 1),
    q [M, T, nx] ~ U(0.01, 0.1), P0 [M, nx, nx] = L L^T + 0.1 I with L = N / sqrt(nx) (symmetrised in fp32), x0 [M, nx] ~ 0.1 N"""
    rng = np.random.default_rng(seed)
    N = lambda *s: rng.normal(size=s)
    A = 0.8 * np.eye(nx) + 0.2 * N(M, T, nx, nx) / np.sqrt(nx)
    C = N(M, T, ny, nx) / np.sqrt(nx)
    dy = N(M, T, ny)
    r = rng.uniform(0.1, 1.0, size=(M, T, ny))
    q = rng.uniform(0.01, 0.1, size=(M, T, nx))
    L = N(M, nx, nx) / np.sqrt(nx)
    P0 = (L @ L.transpose(0, 2, 1) + 0.1 * np.eye(nx)).astype(np.float32)
    P0 = (0.5 * (P0 + P0.transpose(0, 2, 1))).astype(np.float32)
    x0 = 0.1 * N(M, nx)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(A=f(A), C=f(C), dy=f(dy), r=f(r), q=f(q), P0=P0, x0=f(x0))


def pack(A, C, nu, stride=None, fill=0.0):
    """columns [M, T, nx + nu, stride] of A [M, T, nx, nx] and C [M, T, ny, nx]: row j < nx holds column j of A in its first nx
    entries and column j of C in the next ny (the layout rsr_physics_trajectory_fd writes); `fill` in the rest of those rows and in
    the whole of rows j >= nx (B and D, which the filter never reads); stride defaults to nx + ny"""
    M, T, ny, nx = C.shape
    stride = nx + ny if stride is None else stride
    col = np.full((M, T, nx + nu, stride), fill, np.float32)
    col[:, :, :nx, :nx] = A.transpose(0, 1, 3, 2)
    col[:, :, :nx, nx:nx + ny] = C.transpose(0, 1, 3, 2)
    return col


def unpack(col, nx, ny):
    """(A, C) of a columns array"""
    return (np.ascontiguousarray(col[:, :, :nx, :nx].transpose(0, 1, 3, 2)),
            np.ascontiguousarray(col[:, :, :nx, nx:nx + ny].transpose(0, 1, 3, 2)))


def smooth(A, C, dy, r, q, P0, x0=None, smoothing=True, dtype=np.float64):
    """The recursion at `dtype`.  Returns xf [M, T+1, nx], Pf [M, T+1, nx, nx], xs, Ps (zeros without `smoothing`), nll [M],
    status [M, 2] (filter, smoother: -1 or the failed step) and, for the conditioning test, min_s and min_pivot [M] (the smallest
    innovation variance and Cholesky pivot met).  A slot that fails in the filter at t has its rows >= t zeros, nll 0 and no
    smoother; one that fails in the smoother at t has its xs / Ps rows <= t zeros."""
    M, T, ny, nx = C.shape
    c = lambda a: np.asarray(a, dtype)
    A, C, dy, r, q, P0 = c(A), c(C), c(dy), c(r), c(q), c(P0)
    x = np.zeros((M, nx), dtype) if x0 is None else c(x0).copy()
    P = P0.copy()
    half, lg = dtype(0.5), dtype(LOG_2PI)
    xf, Pf = np.zeros((M, T + 1, nx), dtype), np.zeros((M, T + 1, nx, nx), dtype)
    xs, Ps = np.zeros_like(xf), np.zeros_like(Pf)
    nll, status = np.zeros(M, dtype), -np.ones((M, 2))
    min_s, min_piv = np.full(M, np.inf), np.full(M, np.inf)
    alive = np.ones(M, bool)
    eye = np.eye(nx, dtype=dtype)

    def predict(a, p, qt):
        s_ = a @ p @ a.transpose(0, 2, 1)
        return (half * (s_ + s_.transpose(0, 2, 1)) + qt[:, :, None] * eye).astype(dtype)

    with np.errstate(all="ignore"):
        for t in range(T):
            for j in range(ny):
                rj = r[:, t, j]
                on = alive & ~(rj == np.inf)
                if not on.any():
                    continue
                cj = C[:, t, j]
                w = np.einsum("mik,mk->mi", P, cj).astype(dtype)
                s = (np.einsum("mi,mi->m", cj, w) + rj).astype(dtype)
                nu = (dy[:, t, j] - np.einsum("mi,mi->m", cj, x)).astype(dtype)
                good = np.isfinite(rj) & (rj > 0) & np.isfinite(s) & (s > 0)
                bad = on & ~good
                status[bad, 0], alive[bad] = t, False
                on &= good
                so = np.where(on, s, 1).astype(dtype)
                min_s[on] = np.minimum(min_s[on], s[on])
                g = (nu / so).astype(dtype)
                x = np.where(on[:, None], x + w * g[:, None], x).astype(dtype)
                P = np.where(on[:, None, None], P - (w[:, :, None] * w[:, None, :]) * (dtype(1) / so)[:, None, None], P).astype(dtype)
                nll = np.where(on, nll + half * (nu * g + np.log(so) + lg), nll).astype(dtype)
            xf[alive, t], Pf[alive, t] = x[alive], P[alive]
            x = np.einsum("mik,mk->mi", A[:, t], x).astype(dtype)
            P = predict(A[:, t], P, q[:, t])
        xf[alive, T], Pf[alive, T] = x[alive], P[alive]
        nll[~alive] = 0
        if smoothing:
            xs[alive, T], Ps[alive, T] = xf[alive, T], Pf[alive, T]
            for t in range(T - 1, -1, -1):
                Pm = predict(A[:, t], Pf[:, t], q[:, t])
                for m in np.nonzero(alive)[0]:
                    try:
                        if not np.isfinite(Pm[m]).all():
                            raise np.linalg.LinAlgError
                        Lc = np.linalg.cholesky(Pm[m])
                    except np.linalg.LinAlgError:
                        status[m, 1], alive[m] = t, False
                        continue
                    min_piv[m] = min(min_piv[m], float(np.diag(Lc).min()) ** 2)
                    a, pf = A[m, t], Pf[m, t]
                    rhs = (a @ pf).astype(dtype)                                           # G^T = Pm^-1 A Pf
                    G = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs)).astype(dtype).T
                    xs[m, t] = xf[m, t] + G @ (xs[m, t + 1] - a @ xf[m, t])
                    E = G @ (Ps[m, t + 1] - Pm[m]) @ G.T
                    Ps[m, t] = pf + half * (E + E.T)
    return dict(xf=xf, Pf=Pf, xs=xs, Ps=Ps, nll=nll, status=status, min_s=min_s, min_pivot=min_piv)


def drop_columns(inp, keep):
    """the inputs with only the sensor entries `keep` (indices, ascending)"""
    keep = list(keep)
    return dict(inp, C=np.ascontiguousarray(inp["C"][:, :, keep]), dy=np.ascontiguousarray(inp["dy"][:, :, keep]),
                r=np.ascontiguousarray(inp["r"][:, :, keep]))


def failing(inp, kind, slot, t0=None):
    """`inp` with slot `slot` made to fail: "r" (a non-positive variance at step t0), "s" (a negative-definite P0: the first
    innovation variance is < 0) or "pm" (P0 = e1 e1^T, A = I, q = 0: Pm has exact zeros on its diagonal from the second pivot on,
    so the smoother's first step, T - 1, fails)"""
    mod = {k: v.copy() for k, v in inp.items()}
    nx = inp["P0"].shape[-1]
    if kind == "r":
        mod["r"][slot, t0, 0] = -0.5
    elif kind == "s":
        mod["P0"][slot] = -10.0 * np.eye(nx, dtype=np.float32)
    else:
        mod["P0"][slot] = 0.0
        mod["P0"][slot, 0, 0] = 1.0
        mod["A"][slot] = np.eye(nx, dtype=np.float32)
        mod["q"][slot] = 0.0
    return mod


M = 32
FAMILY_NX = dict(cube=40, go2flat=36, tshape=28)


def shapes(kind):
    """the (T, ny) the device tests run for a family: T in {1, 6} by ny in {1, 55, 64}, and 64 steps on the cube"""
    return [(T, ny) for T in (1, 6) for ny in (1, 55, 64)] + ([(64, 55)] if kind == "cube" else [])


def family_case(kind, T, ny):
    return case(M, T, FAMILY_NX[kind], ny, seed=100 + T + ny)


_CASES = {}


def case(M, T, nx, ny, seed):
    """(inputs, fp64 reference, fp32 reference) of one case, computed once and shared: the arrays are read-only"""
    key = (M, T, nx, ny, seed)
    if key not in _CASES:
        inp = inputs(M, T, nx, ny, seed)
        refs = [smooth(**inp, dtype=dt) for dt in (np.float64, np.float32)]
        for group in [inp] + refs:
            for a in group.values():
                a.flags.writeable = False
        _CASES[key] = (inp, refs[0], refs[1])
    return _CASES[key]
