"""tests/lqr_ref.py, the numpy reference of the LQR backward pass, verified independently of the kernel: against the stacked
finite-horizon QP it is the dynamic-programming solution of, against its regularisation formulas evaluated directly, and for the
conditioning of the shared inputs that the GPU tests' bounds rest on."""
import numpy as np
import pytest

import lqr_ref
from physics_support import rel


def _qp(inp, s, x0):
    """The finite-horizon problem of slot s in the controls alone: J(U) = 1/2 U^T H U + g^T U + c with dx_{t+1} = A_t dx_t + B_t du_t
    from dx_0 = x0, cost sum_t [lx.dx + lu.du + 1/2 dx' lxx dx + 1/2 du' luu du + du' lux dx] + terminal.  Returns H, g and the maps
    dx_t = Sx[t] x0 + Su[t] U."""
    A, B = inp["A"][s].astype(np.float64), inp["B"][s].astype(np.float64)
    T, nx, nu = B.shape
    Sx, Su = [np.eye(nx)], [np.zeros((nx, T * nu))]
    for t in range(T):
        E = np.zeros((nu, T * nu))
        E[:, t * nu:(t + 1) * nu] = np.eye(nu)
        Sx.append(A[t] @ Sx[t])
        Su.append(A[t] @ Su[t] + B[t] @ E)
    H, g = np.zeros((T * nu, T * nu)), np.zeros(T * nu)
    f64 = lambda k: inp[k][s].astype(np.float64)
    lx, lu, lxx, luu, lux = f64("lx"), f64("lu"), f64("lxx"), f64("luu"), f64("lux")
    for t in range(T + 1):
        xc = Sx[t] @ x0
        H += Su[t].T @ lxx[t] @ Su[t]
        g += Su[t].T @ (lx[t] + lxx[t] @ xc)
        if t < T:
            E = np.zeros((nu, T * nu))
            E[:, t * nu:(t + 1) * nu] = np.eye(nu)
            H += E.T @ luu[t] @ E + E.T @ lux[t] @ Su[t] + Su[t].T @ lux[t].T @ E
            g += E.T @ (lu[t] + lux[t] @ xc)
    return H, g, Sx, Su


def _cost(inp, s, x0, U):
    """the cost of the controls U [T, nu] from dx_0 = x0, in fp64"""
    f64 = lambda k: inp[k][s].astype(np.float64)
    A, B, lx, lu, lxx, luu, lux = (f64(k) for k in ("A", "B", "lx", "lu", "lxx", "luu", "lux"))
    x, J = x0.copy(), 0.0
    for t in range(len(U)):
        u = U[t]
        J += lx[t] @ x + lu[t] @ u + 0.5 * x @ lxx[t] @ x + 0.5 * u @ luu[t] @ u + u @ lux[t] @ x
        x = A[t] @ x + B[t] @ u
    return J + lx[-1] @ x + 0.5 * x @ lxx[-1] @ x


def test_closed_loop_controls_minimise_the_stacked_qp():
    T, nx, nu = 3, 6, 2
    inp = lqr_ref.inputs(2, T, nx, nu, seed=4)
    out = lqr_ref.backward(**inp, mu=0.0, dtype=np.float64)
    assert (out["status"] == -1).all()
    rng = np.random.default_rng(9)
    for s in range(2):
        x0 = rng.normal(size=nx)
        H, g, _, _ = _qp(inp, s, x0)
        U = np.linalg.solve(H, -g).reshape(T, nu)
        x, mine = x0.copy(), []
        for t in range(T):
            u = out["k"][s, t] + out["gain"][s, t] @ x
            mine.append(u)
            x = inp["A"][s, t].astype(np.float64) @ x + inp["B"][s, t].astype(np.float64) @ u
        assert np.abs(np.array(mine) - U).max() <= 1e-9
        # at dx_0 = 0 the expected change of the full step, dV[0] + dV[1], is the QP's optimum
        H0, g0, _, _ = _qp(inp, s, np.zeros(nx))
        U0 = np.linalg.solve(H0, -g0)
        assert abs(out["dV"][s].sum() - (0.5 * U0 @ H0 @ U0 + g0 @ U0)) <= 1e-9


def test_value_at_t0_is_the_optimal_cost_to_go():
    """J*(x0) = min_U J(x0, U) is quadratic in x0: Vx[0] is its gradient at 0 and Vxx[0] its Hessian (central differences of an exact
    quadratic are exact up to rounding)."""
    T, nx, nu = 3, 6, 2
    inp = lqr_ref.inputs(1, T, nx, nu, seed=5)
    out = lqr_ref.backward(**inp, mu=0.0, dtype=np.float64)

    def Jstar(x0):
        H, g, _, _ = _qp(inp, 0, x0)
        return _cost(inp, 0, x0, np.linalg.solve(H, -g).reshape(T, nu))

    h, I = 0.5, np.eye(nx)
    grad = np.array([(Jstar(h * I[i]) - Jstar(-h * I[i])) / (2 * h) for i in range(nx)])
    hess = np.array([[(Jstar(h * (I[i] + I[j])) - Jstar(h * (I[i] - I[j])) - Jstar(h * (I[j] - I[i])) + Jstar(-h * (I[i] + I[j]))) / (4 * h * h)
                      for j in range(nx)] for i in range(nx)])
    assert np.abs(grad - out["Vx"][0, 0]).max() <= 1e-9
    assert np.abs(hess - out["Vxx"][0, 0]).max() <= 1e-9
    assert np.array_equal(out["Vxx"][0, 0], out["Vxx"][0, 0].T)


@pytest.mark.parametrize("state_reg", [False, True])
def test_regularised_gains_are_the_formula(state_reg):
    """at the last step Vx, Vxx are the terminal cost, so K and k follow from the inputs directly"""
    T, nx, nu, mu = 3, 6, 2, 0.37
    inp = lqr_ref.inputs(2, T, nx, nu, seed=6)
    out = lqr_ref.backward(**inp, mu=mu, state_reg=state_reg, dtype=np.float64)
    plain = lqr_ref.backward(**inp, mu=0.0, state_reg=state_reg, dtype=np.float64)
    assert np.abs(out["gain"] - plain["gain"]).max() > 1e-3                       # (the regularisation acts)
    for s in range(2):
        f64 = lambda k: inp[k][s].astype(np.float64)
        A, B, V, v = f64("A")[T - 1], f64("B")[T - 1], f64("lxx")[T], f64("lx")[T]
        Quu, Qux, Qu = f64("luu")[T - 1] + B.T @ V @ B, f64("lux")[T - 1] + B.T @ V @ A, f64("lu")[T - 1] + B.T @ v
        Quu_r = Quu + mu * (B.T @ B if state_reg else np.eye(nu))
        Qux_r = Qux + (mu * B.T @ A if state_reg else 0.0)
        assert np.abs(out["gain"][s, T - 1] + np.linalg.inv(Quu_r) @ Qux_r).max() <= 1e-9
        assert np.abs(out["k"][s, T - 1] + np.linalg.inv(Quu_r) @ Qu).max() <= 1e-9
        # the value update takes the unregularised Q
        K, k = out["gain"][s, T - 1], out["k"][s, T - 1]
        Qxx = f64("lxx")[T - 1] + A.T @ V @ A
        Vxx = Qxx + K.T @ Quu @ K + K.T @ Qux + Qux.T @ K
        assert np.abs(out["Vxx"][s, T - 1] - 0.5 * (Vxx + Vxx.T)).max() <= 1e-9
        assert np.abs(out["Vx"][s, T - 1] - (f64("lx")[T - 1] + A.T @ v + K.T @ Quu @ k + K.T @ Qu + Qux.T @ k)).max() <= 1e-9


def test_failure_stops_the_slot():
    inp = {k: v.copy() for k, v in lqr_ref.inputs(3, 4, 6, 2, seed=7).items()}
    inp["luu"][1, 2] = -1e4 * np.eye(2, dtype=np.float32)
    out = lqr_ref.backward(**inp, mu=1e-3)
    assert list(out["status"]) == [-1, 2, -1] and (out["dV"][1] == 0).all() and (out["gain"][1, :3] == 0).all()
    assert np.abs(out["gain"][1, 3]).max() > 0
    assert (lqr_ref.backward(**inp, mu=np.array([1e-3, 2e4, 1e-3]))["status"] == -1).all()


def test_pack_layout():
    inp = lqr_ref.inputs(2, 3, 6, 2, seed=8)
    col = lqr_ref.pack(inp["A"], inp["B"], 9, fill=np.nan)
    assert col.shape == (2, 3, 8, 9) and np.isnan(col[..., 6:]).all()
    assert col[1, 2, 4, 3] == inp["A"][1, 2, 3, 4] and col[1, 2, 6 + 1, 5] == inp["B"][1, 2, 5, 1]
    assert lqr_ref.pack(inp["A"], inp["B"]).shape == (2, 3, 8, 6)


@pytest.mark.parametrize("nx,nu", [(40, 5), (36, 12), (28, 5)])
@pytest.mark.parametrize("T", [1, 6, 64])
def test_conditioning(nx, nu, T):
    """the statement of lqr_ref's docstring: fp32 within 1.4e-6 of fp64 on every output, every |output| <= 1e3"""
    _, r64, r32 = lqr_ref.case(32, T, nx, nu, seed=100 + T, mu=1e-3)
    assert (r64["status"] == -1).all() and (r32["status"] == -1).all()
    for k in lqr_ref.OUTPUTS:
        spread = rel(r32[k], r64[k]).max()
        print(nx, nu, T, k, "fp32 - fp64 %.2e" % spread, "max |.| %.2e" % np.abs(r64[k]).max())
        assert spread <= 1.4e-6, (k, spread)
        assert np.abs(r64[k]).max() <= 1e3, k
