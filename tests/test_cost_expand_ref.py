"""tests/cost_expand_ref.py against the cost it expands, and Physics.differentiate_state against tests/tangent_ref.py, on the CPU.

The float64 expansion is held to central differences of cost_expand_ref.cost, the cost 1/2 sum w r^2 under the linear sensor
model ds + C dx + D du.  That cost is quadratic in the deviations, so a central first difference and a four-point mixed second
difference have no truncation error at any step h; what is left is rounding.  Every cost value is a sum of N = T (2 nv + nu + ny)
terms (w r) r, each within 3 u of its exact value plus the (ncol + 2) u of its sensor residual's dot product, summed with at most
N u more: within (N + ncol + 5) u |c| <= 64 u c_max for the sizes here (N = 36, ncol = 8).  A gradient entry divides the difference
of two by 2 h, a Hessian entry the signed sum of four by 4 h^2: both within 64 u c_max / min(h, h^2) <= BOUND = 64 eps c_max with
h = 1 and eps = 2^-52 = 2 u, c_max the largest cost evaluated.

differentiate_state is held to the bound of tests/test_tangent_ref.py (32 eps max(1, |q|_inf + |d|_inf)), whose derivation covers
it: against tangent_ref.differentiate_pos on the same inputs the two sides share steps 1 to 3 exactly and differ by steps 4 and 5
on either side (at most 2 x 15 u); after integrate_state the chain is the one that derivation follows (57 u)."""
import types

import numpy as np
import pytest

import cost_expand_ref as R
import tangent_ref
from test_tangent_ref import _bound, _inputs

EPS64 = 2.0 ** -52
M, T, NV, NU, NY = 2, 3, 3, 2, 4
NX = 2 * NV
CASES = [R.TERMS, ("w_qpos",), ("w_qvel",), ("w_ctrl",), ("w_sensor",)]


def _flat(x, u):
    return np.concatenate([x.reshape(-1), u.reshape(-1)])


def _cost_of(inp, s, z, terms, refs):
    x, u = z[:(T + 1) * NX].reshape(T + 1, NX), z[(T + 1) * NX:].reshape(T, NU)
    return R.cost(inp, s, x, u, terms, refs)


@pytest.mark.parametrize("refs", [("ctrl_ref", "sensor_ref"), ()])
@pytest.mark.parametrize("terms", CASES, ids=lambda t: "+".join(t))
def test_expansion_is_the_gradient_and_hessian_of_the_cost(terms, refs):
    inp = R.inputs(M, T, NV, NU, NY, seed=5, stride=NX + NY + 3)
    e = R.expand(inp, np.float64, terms, refs)
    n, h = (T + 1) * NX + T * NU, 1.0
    for s in range(M):
        cmax = 0.0

        def c(z):
            nonlocal cmax
            v = _cost_of(inp, s, z, terms, refs)
            cmax = max(cmax, abs(v))
            return v
        unit = np.eye(n) * h
        grad = np.array([(c(unit[i]) - c(-unit[i])) / (2 * h) for i in range(n)])
        hess = np.array([[(c(unit[i] + unit[j]) - c(unit[i] - unit[j]) - c(unit[j] - unit[i]) + c(-unit[i] - unit[j])) / (4 * h * h)
                          for j in range(n)] for i in range(n)])
        # the expansion laid out over the same variables: the state block of index t, the ctrl block of step t, lux between them;
        # every other block is zero, i.e. perturbing x_{t+1} moves only the state term of cost row t
        want_g = _flat(e["lx"][s], e["lu"][s])
        want_h = np.zeros((n, n))
        for t in range(T + 1):
            xs = slice(t * NX, (t + 1) * NX)
            want_h[xs, xs] = e["lxx"][s, t]
            if t < T:
                us = slice((T + 1) * NX + t * NU, (T + 1) * NX + (t + 1) * NU)
                want_h[us, us] = e["luu"][s, t]
                want_h[us, xs] = e["lux"][s, t]
                want_h[xs, us] = e["lux"][s, t].T
        bound = 64 * EPS64 * cmax
        print(terms, refs, s, "grad err %.2e hess err %.2e bound %.2e" % (np.abs(grad - want_g).max(), np.abs(hess - want_h).max(), bound))
        assert np.abs(grad - want_g).max() <= bound and np.abs(hess - want_h).max() <= bound
        # the rows: index 0 has no state part, index T nothing but the state part of cost row T-1
        if "w_sensor" not in terms:
            assert not e["lx"][s, 0].any() and not e["lxx"][s, 0].any() and not e["lux"][s].any()
        if not {"w_qpos", "w_qvel"} & set(terms):
            assert not e["lx"][s, T].any() and not e["lxx"][s, T].any()


def test_hessian_blocks_are_symmetric_and_positive_semidefinite():
    inp = R.inputs(M, T, NV, NU, NY, seed=6)
    for dt in (np.float64, np.float32):
        e = R.expand(inp, dt)
        for k in ("lxx", "luu"):
            assert np.array_equal(e[k], np.swapaxes(e[k], -1, -2)), (dt, k)                 # bit for bit, in float32 too
            ev = np.linalg.eigvalsh(e[k].astype(np.float64))
            assert ev.min() >= -64 * np.finfo(dt).eps * np.abs(e[k]).max(), (dt, k, ev.min())
    # the whole step Hessian [[lxx, lux^T], [lux, luu]] as well
    e = R.expand(inp, np.float64)
    full = np.block([[e["lxx"][:, :T], np.swapaxes(e["lux"], -1, -2)], [e["lux"], e["luu"]]])
    assert np.linalg.eigvalsh(full).min() >= -64 * EPS64 * np.abs(full).max()


def _standin(A, nq, nv):
    from rsr_mjx_amd.physics import Physics
    p = Physics.__new__(Physics)
    p.dims = types.SimpleNamespace(nq=nq, nv=nv)
    p.env = types.SimpleNamespace(sys=types.SimpleNamespace(arrays=A))
    return p


@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_differentiate_state(kind):
    import torch
    A, nv, q, d = _inputs(kind)
    n, nq = q.shape
    p = _standin(A, nq, nv)
    rng = np.random.default_rng(8)
    v, dv = rng.normal(size=(n, nv)), rng.normal(scale=0.3, size=(n, nv))
    t = lambda a: torch.as_tensor(np.array(a), dtype=torch.float64)
    bound = _bound(q, d)
    # against mj_differentiatePos in numpy, on states a tangent step apart
    q1 = tangent_ref.moved(A, nv, q, d)
    got = p.differentiate_state(t(q1), t(v + dv), t(q), t(v)).numpy()
    assert got.shape == (n, 2 * nv)
    err = np.abs(got[:, :nv] - tangent_ref.differentiate_pos(A, nv, q1, q)).max()
    print(kind, "vs differentiate_pos %.3e, bound %.3e" % (err, bound))
    assert err <= bound and np.array_equal(got[:, nv:], (v + dv) - v)
    # it inverts integrate_state
    dx = np.concatenate([d, dv], 1)
    qi, vi = p.integrate_state(t(q), t(v), t(dx))
    back = p.differentiate_state(qi, vi, t(q), t(v)).numpy()
    err = np.abs(back[:, :nv] - d).max()
    print(kind, "after integrate_state %.3e, bound %.3e" % (err, bound))
    assert err <= bound and np.abs(back[:, nv:] - dv).max() <= 4 * EPS64 * max(1.0, np.abs(v).max() + np.abs(dv).max())
    # exactly 0 on equal states, in both precisions and with leading dims [4, n / 4]
    for dt in (torch.float64, torch.float32):
        f = lambda a: torch.as_tensor(np.array(a), dtype=dt).reshape(4, n // 4, -1)
        z = p.differentiate_state(f(q), f(v), f(q), f(v))
        assert tuple(z.shape) == (4, n // 4, 2 * nv) and z.dtype == dt and not bool(z.any())
    for bad, msg in (((t(q)[:, :-1], t(v), t(q), t(v)), "expects qpos"), ((t(q), t(v), t(q), t(v)[:, :-1]), "expects qvel_ref"),
                     ((t(q), t(v)[:3], t(q), t(v)), "same leading dims"), ((q, t(v), t(q), t(v)), "expects qpos")):
        with pytest.raises(ValueError, match=msg):
            p.differentiate_state(*bad)
