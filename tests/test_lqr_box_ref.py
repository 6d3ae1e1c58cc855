"""The numpy reference of the control-limited backward pass (tests/lqr_box_ref.py) and the inputs its GPU tests share, on the CPU:
the fp64 reference's k_t satisfies the KKT conditions of every step's QP (which does not depend on the iteration), infinite bounds
give lqr_ref.backward bit for bit, and the shared cases are conditioned: fp32 and fp64 take the same clamped sets and codes with
every margin >= 1e-4, and the cases reach every branch of the iteration."""
import numpy as np
import pytest

import lqr_box_ref as box
import lqr_ref
from physics_support import rel

M, MU = 32, 1e-3
CASES = [(nx, nu, T) for (nx, nu), Ts in (((40, 5), (1, 6, 64)), ((36, 12), (1, 6)), ((28, 5), (1, 6))) for T in Ts]
SHAPES = [(40, 5), (36, 12), (28, 5)]


def _case(nx, nu, T, **kw):
    return box.case(M, T, nx, nu, 100 + T, 700 + T, mu=MU, **kw)


def _directed(nx, nu):
    b = box.BACKTRACK
    return box.case(M, b["T"], nx, nu, b["seed"], b["bseed"], mu=MU, directed=True)


@pytest.mark.parametrize("nx,nu,T", CASES)
def test_fp64_reference_satisfies_kkt(nx, nu, T):
    inp, r64, _ = _case(nx, nu, T)
    assert (r64["status"] == -1).all()
    worst = 0.0
    for s in range(M):
        for t in range(T):
            B = inp["B"][s, t].astype(np.float64)
            H = inp["luu"][s, t] + B.T @ r64["Vxx"][s, t + 1] @ B + MU * np.eye(nu)
            g = inp["lu"][s, t] + B.T @ r64["Vx"][s, t + 1]
            worst = max(worst, box.kkt(H, g, inp["lo"][s, t], inp["hi"][s, t], r64["k"][s, t]))
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_infinite_bounds_are_the_plain_recursion(nx, nu, dtype):
    T = 6
    inp = lqr_ref.inputs(M, T, nx, nu, 100 + T)
    inf = np.full((M, T, nu), np.inf, np.float32)
    for state_reg in (False, True):
        plain = lqr_ref.backward(**inp, mu=MU, state_reg=state_reg, dtype=dtype)
        got = box.backward_box(**inp, lo=-inf, hi=inf, mu=MU, state_reg=state_reg, dtype=dtype)
        for k in plain:
            assert got[k].dtype == plain[k].dtype and got[k].tobytes() == plain[k].tobytes(), k
        assert (got["clamped"] == 0).all() and (got["qp"] == (1, 0)).all()


def _conditioned(r64, r32):
    assert (r64["status"] == -1).all() and (r32["status"] == -1).all()
    assert (r64["clamped"] == r32["clamped"]).all() and (r64["qp"][..., 1] == r32["qp"][..., 1]).all()
    margin = r64["margin"].min(axis=1)
    assert (margin >= 1e-4).all(), (np.flatnonzero(margin < 1e-4), margin.min())          # every slot: none is left out
    worst = max(float(rel(r32[k], r64[k]).max()) for k in lqr_ref.OUTPUTS)
    return margin.min(), worst


@pytest.mark.parametrize("nx,nu,T", CASES)
def test_conditioning(nx, nu, T):
    _, r64, r32 = _case(nx, nu, T)
    margin, worst = _conditioned(r64, r32)
    print(f"({nx}, {nu}) T={T}: smallest margin {margin:.2e}, fp32-fp64 {worst:.2e}, Newton steps <= {int(r64['qp'][..., 0].max())}, "
          f"clamped {float((r64['clamped'] != 0).mean()):.0%}")
    assert set(np.unique(r64["qp"][..., 1])) <= {0.0, 1.0} and r64["qp"][..., 0].max() <= 5
    assert worst <= 2e-6                         # a fifth of the floor of physics_support.rule (1e-5): measured 3.5e-7 .. 1.23e-6
    assert 0.17 <= (r64["clamped"] != 0).mean() <= 0.42


def _census(r):
    c = r["census"]
    return dict(all_free=int((r["clamped"] == 0).all(-1).sum()), all_clamped=int((r["qp"][..., 1] == 1).sum()), clipped_start=int(c[..., 0].sum()),
                line_search=int(c[..., 1].sum()), shrunk=int(c[..., 2].sum()), released=int(c[..., 3].sum()))


def test_census():
    """Every branch of the iteration is taken somewhere: the counts of the cube's T = 64 case are pinned (a change of the generator or of the iteration shows here), and
    each case has steps with nothing clamped, clipped starts and line searches."""
    _, r64, _ = _case(40, 5, 64)
    got = _census(r64)
    assert {k: got[k] for k in ("all_free", "all_clamped", "clipped_start", "line_search", "released")} == \
        dict(all_free=805, all_clamped=1, clipped_start=447, line_search=1117, released=32), got
    for nx, nu, T in CASES:
        c = _census(_case(nx, nu, T)[1])
        assert c["clipped_start"] > 0 and c["line_search"] > 0, (nx, nu, T, c)
        assert c["all_free"] > 0 or (nx, nu, T) == (36, 12, 1), (nx, nu, T, c)             # (12 controls, 32 steps: none is all free)
    assert sum(_census(_case(nx, nu, T)[1])["all_clamped"] for nx, nu, T in CASES) >= 2


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_directed_inputs_backtrack(nx, nu):
    """backtrack_inputs at the recorded seed: the line search shrinks the step in at least one step (in both precisions), under the
    conditioning every other case meets"""
    _, r64, r32 = _directed(nx, nu)
    margin, worst = _conditioned(r64, r32)
    print(f"({nx}, {nu}) directed: shrunk {_census(r64)['shrunk']}, smallest margin {margin:.2e}, fp32-fp64 {worst:.2e}")
    assert _census(r64)["shrunk"] > 0 and _census(r32)["shrunk"] > 0


def agreed_slots(nx, nu, T):
    """max_iter = 1: (inputs, fp64 reference, the slots on which fp32 and fp64 agree in clamped and qp at every step)"""
    inp, r64, r32 = _case(nx, nu, T, max_iter=1)
    ok = [s for s in range(M) if (r64["clamped"][s] == r32["clamped"][s]).all() and (r64["qp"][s] == r32["qp"][s]).all()]
    return inp, r64, ok


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_max_iter_one(nx, nu):
    for T in (1, 6):
        _, r64, ok = agreed_slots(nx, nu, T)
        assert (r64["status"] == -1).all() and (r64["qp"][..., 1] == 2).any() and r64["qp"][..., 0].max() <= 1
        assert len(ok) >= M - M // 4, ok
