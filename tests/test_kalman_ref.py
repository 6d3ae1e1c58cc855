"""tests/kalman_ref.py, the numpy reference of the Kalman filter and RTS smoother, checked without the kernel: the fp64 smoother
against the stacked weighted least-squares problem solved densely, nll against the Gaussian log-density of the measurements under
the stacked model, missing entries against removed columns, the failure protocol, the packing, and the conditioning of the shared
inputs at the shapes the device tests run."""
import numpy as np
import pytest

import kalman_ref
from physics_support import rel


def _stacked(inp, m):
    """slot m's stacked problem: (mean [T+1, nx], covariance blocks [T+1, nx, nx], nll) in fp64.  Unknowns z = (dx_0 .. dx_T); rows:
    the prior dx_0 ~ N(x0, P0), T dynamics rows dx_{t+1} - A_t dx_t ~ N(0, Q_t), the measurement rows dy_t - C_t dx_t ~ N(0, R_t)."""
    A, C, dy, r, q = (inp[k][m].astype(np.float64) for k in ("A", "C", "dy", "r", "q"))
    P0, x0 = inp["P0"][m].astype(np.float64), inp["x0"][m].astype(np.float64)
    T, ny, nx = C.shape
    n = (T + 1) * nx
    H0, b0, W0 = np.zeros((n, n)), np.zeros(n), np.zeros((n, n))
    H0[:nx, :nx], b0[:nx], W0[:nx, :nx] = np.eye(nx), x0, np.linalg.inv(P0)
    for t in range(T):
        rows = slice((t + 1) * nx, (t + 2) * nx)
        H0[rows, (t + 1) * nx:(t + 2) * nx], H0[rows, t * nx:(t + 1) * nx] = np.eye(nx), -A[t]
        W0[rows, rows] = np.diag(1.0 / q[t])
    Hc = np.zeros((T * ny, n))
    for t in range(T):
        Hc[t * ny:(t + 1) * ny, t * nx:(t + 1) * nx] = C[t]
    y, Wc = dy.reshape(-1), np.diag(1.0 / r.reshape(-1))
    L0 = H0.T @ W0 @ H0
    lam = L0 + Hc.T @ Wc @ Hc
    cov = np.linalg.inv(lam)
    mean = cov @ (H0.T @ W0 @ b0 + Hc.T @ Wc @ y)
    blocks = np.stack([cov[t * nx:(t + 1) * nx, t * nx:(t + 1) * nx] for t in range(T + 1)])
    # the marginal of the measurements: y ~ N(Hc mz, Hc Sz Hc^T + R) with z ~ N(mz, Sz) from the prior and the dynamics alone
    Sz = np.linalg.inv(L0)
    mz = Sz @ (H0.T @ W0 @ b0)
    Sy = Hc @ Sz @ Hc.T + np.diag(r.reshape(-1))
    e = y - Hc @ mz
    nll = 0.5 * (e @ np.linalg.solve(Sy, e) + np.linalg.slogdet(Sy)[1] + len(y) * np.log(2.0 * np.pi))
    return mean.reshape(T + 1, nx), blocks, nll


@pytest.mark.parametrize("T, nx, ny", [(1, 4, 1), (4, 6, 3), (5, 4, 7)])
def test_the_recursion_solves_the_stacked_least_squares_problem(T, nx, ny):
    M = 3
    inp = kalman_ref.inputs(M, T, nx, ny, seed=5)
    got = kalman_ref.smooth(**inp, dtype=np.float64)
    assert (got["status"] == -1).all()
    for m in range(M):
        mean, blocks, nll = _stacked(inp, m)
        assert np.abs(got["xs"][m] - mean).max() < 1e-9
        assert np.abs(got["Ps"][m] - blocks).max() < 1e-9
        assert abs(got["nll"][m] - nll) < 1e-9 * max(1.0, abs(nll))
        # the last filtered row is the smoothed one, and the filter's row t is the smoother of the log cut at t
        assert np.array_equal(got["xs"][m, T], got["xf"][m, T]) and np.array_equal(got["Ps"][m, T], got["Pf"][m, T])
    cut = {k: (v[:, :T - 1] if k in ("A", "C", "dy", "r", "q") else v) for k, v in inp.items()}
    if T > 1:
        short = kalman_ref.smooth(**cut, dtype=np.float64)
        assert np.abs(short["xs"][:, T - 2] - got["xf"][:, T - 2]).max() < 1e-9          # (the last row that has a measurement)
        assert np.abs(short["Ps"][:, T - 2] - got["Pf"][:, T - 2]).max() < 1e-9


def test_no_x0_is_a_zero_x0_and_the_filter_alone_is_the_same_filter():
    inp = kalman_ref.inputs(3, 4, 6, 3, seed=6)
    for dt in (np.float64, np.float32):
        full = kalman_ref.smooth(**inp, dtype=dt)
        lean = kalman_ref.smooth(**inp, smoothing=False, dtype=dt)
        for k in ("xf", "Pf", "nll"):
            assert np.array_equal(full[k], lean[k]), k
        assert not lean["xs"].any() and not lean["Ps"].any()
        zero = kalman_ref.smooth(**dict(inp, x0=np.zeros_like(inp["x0"])), dtype=dt)
        none = kalman_ref.smooth(**dict(inp, x0=None), dtype=dt)
        for k in kalman_ref.OUTPUTS:
            assert np.array_equal(zero[k], none[k]), k
        assert np.array_equal(full["Pf"], full["Pf"].transpose(0, 1, 3, 2)) and np.array_equal(full["Ps"], full["Ps"].transpose(0, 1, 3, 2))


def test_missing_entries_equal_removed_columns():
    inp = kalman_ref.inputs(3, 5, 6, 5, seed=7)
    gone, keep = [1, 3], [0, 2, 4]
    r = inp["r"].copy()
    r[:, :, gone] = np.inf
    for dt in (np.float64, np.float32):
        a = kalman_ref.smooth(**dict(inp, r=r), dtype=dt)
        b = kalman_ref.smooth(**kalman_ref.drop_columns(inp, keep), dtype=dt)
        for k in kalman_ref.OUTPUTS + ("status",):
            assert np.array_equal(a[k], b[k]), k
        c = kalman_ref.smooth(**inp, dtype=dt)
        assert not np.array_equal(a["xs"], c["xs"])
    # a single missing sample changes the result from its step on only
    r = inp["r"].copy()
    r[1, 3, 2] = np.inf
    a, c = kalman_ref.smooth(**dict(inp, r=r)), kalman_ref.smooth(**inp)
    assert np.array_equal(a["xf"][:, :3], c["xf"][:, :3]) and not np.array_equal(a["xf"][1, 3], c["xf"][1, 3])
    assert np.array_equal(a["xs"][[0, 2]], c["xs"][[0, 2]])


def test_the_failure_protocol():
    M, T, nx, ny = 4, 5, 6, 3
    inp = kalman_ref.inputs(M, T, nx, ny, seed=8)
    base = kalman_ref.smooth(**inp)
    for kind, slot, t0, want in (("r", 2, 3, (3, -1)), ("s", 1, None, (0, -1)), ("pm", 3, None, (-1, T - 1)),
                                 ("r", 0, 0, (0, -1))):
        got = kalman_ref.smooth(**kalman_ref.failing(inp, kind, slot, t0))
        rest = [m for m in range(M) if m != slot]
        assert tuple(got["status"][slot]) == want and (got["status"][rest] == -1).all(), (kind, got["status"])
        for k in kalman_ref.OUTPUTS:
            assert np.array_equal(got[k][rest], base[k][rest]), (kind, k)
        if want[0] >= 0:
            t = want[0]
            assert got["nll"][slot] == 0 and not got["xs"][slot].any() and not got["Ps"][slot].any()
            assert not got["xf"][slot, t:].any() and not got["Pf"][slot, t:].any()
            if kind == "r":
                assert np.array_equal(got["xf"][slot, :t], base["xf"][slot, :t]) and np.array_equal(got["Pf"][slot, :t], base["Pf"][slot, :t])
        else:
            t = want[1]
            assert np.isfinite(got["xf"][slot]).all() and got["nll"][slot] != 0
            assert not got["xs"][slot, :t + 1].any() and not got["Ps"][slot, :t + 1].any()
            assert np.array_equal(got["xs"][slot, t + 1:], got["xf"][slot, t + 1:])
    # a NaN or -inf variance fails like a non-positive one; +inf does not
    for bad in (np.nan, -np.inf, 0.0):
        mod = {k: v.copy() for k, v in inp.items()}
        mod["r"][1, 2, 1] = bad
        assert tuple(kalman_ref.smooth(**mod)["status"][1]) == (2, -1), bad


def test_pack_round_trips():
    inp = kalman_ref.inputs(2, 3, 8, 5, seed=9)
    nu = 3
    tight = kalman_ref.pack(inp["A"], inp["C"], nu)
    assert tight.shape == (2, 3, 11, 13) and tight.dtype == np.float32
    A, C = kalman_ref.unpack(tight, 8, 5)
    assert np.array_equal(A, inp["A"]) and np.array_equal(C, inp["C"])
    assert tight[0, 1, 2, 4] == inp["A"][0, 1, 4, 2] and tight[0, 1, 2, 8 + 3] == inp["C"][0, 1, 3, 2]
    wide = kalman_ref.pack(inp["A"], inp["C"], nu, stride=20, fill=777.0)
    assert wide.shape == (2, 3, 11, 20) and (wide[:, :, :, 13:] == 777.0).all() and (wide[:, :, 8:] == 777.0).all()
    assert np.array_equal(wide[:, :, :8, :13], tight[:, :, :8])
    A, C = kalman_ref.unpack(wide, 8, 5)
    assert np.array_equal(A, inp["A"]) and np.array_equal(C, inp["C"])


@pytest.mark.parametrize("kind", list(kalman_ref.FAMILY_NX))
def test_conditioning(kind):
    """The shared inputs at the device tests' shapes: every innovation variance and every Cholesky pivot of Pm stays well away from
    zero, in fp64 and in fp32, every output is of moderate size, and fp32 stays far inside the floors of physics_support.rule."""
    for T, ny in kalman_ref.shapes(kind):
        _, r64, r32 = kalman_ref.family_case(kind, T, ny)
        for ref in (r64, r32):
            assert (ref["status"] == -1).all()
            assert ref["min_s"].min() >= 0.09, (T, ny, ref["min_s"].min())           # s >= r >= 0.1
            assert ref["min_pivot"].min() >= 0.009, (T, ny, ref["min_pivot"].min())   # Pm >= q >= 0.01
        for k in kalman_ref.OUTPUTS:
            assert np.abs(r64[k]).max() <= 1e3 * (T * ny if k == "nll" else 1), (T, ny, k, np.abs(r64[k]).max())
            spread = rel(r32[k], r64[k]).max()
            print(kind, T, ny, k, "%.2e" % spread)
            assert spread <= 1e-5, (T, ny, k, spread)
