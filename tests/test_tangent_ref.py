"""tests/tangent_ref.py against itself, on the CPU: the functions the GPU tests of transition_fd and feedback_rollouts take as their
fp64 reference had so far run inside those tests only.  On the cube and the Go2 flat model (free joints, hinges and slides), with
seeded inputs on unit quaternions.

The bound, BOUND = 32 eps x max(1, |q|_inf + |d|_inf) with eps = 2^-52 (u = eps / 2 the unit roundoff), first-order in u:
  add columns: fl(fl(q + d) - q) is off d by at most u |q + d| + u |d| <= eps (|q| + |d|): one eps of the condition.
  rot columns, |q| = 1 and |d| <= 1 (the condition is 1):
    1. r = (cos(a / 2), sin(a / 2) v / a), a = |v|: a carries 2.5 u (three squares summed: 3 u, halved by the root, plus the root's u);
       cos, sin and the division add u each and pass a's error on: every component of r within 6 u, r within 12 u in the 2-norm;
    2. p = q r: each component is a sum of four products, within 4 u |q| |r|; with r's error, p is within 16 u;
    3. the renormalisation (four squares, root, division) adds at most 4 u: 20 u;
    4. dq = conj(q) p: 4 u more, 24 u in the 2-norm;
    5. the rotation vector 2 atan2(|dq_v|, dq_w) dq_v / |dq_v| moves by at most 2 x 1.05 times an error of dq for angles up to 1
       ((t / 2) / sin(t / 2) <= 1.05 there): 51 u; its own norm, atan2, division and product add 6 u |d|: 57 u < 32 eps.
  integrate_pos against moved: both sides are within the 20 u of steps 1 to 3 of the exact quaternion, so within 40 u = 20 eps of
  each other; a quaternion that moved() multiplies by the identity is renormalised (4 u), integrate_pos leaves it as it is."""
import functools

import numpy as np
import pytest

from rsr_mjx_amd.envs import families
from tangent_ref import columns, differentiate_pos, integrate_pos, moved

N = 64
EPS64 = 2.0 ** -52
KINDS = ["cube", "go2flat"]


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    """(A, nv, q [N, nq] with unit quaternions, d [N, nv] with every entry and every rotation vector within 1)"""
    A = families.envdef(kind).sys.arrays
    nv = len(A["dof_bodyid"])
    rng = np.random.default_rng(17)
    q = np.tile(np.asarray(A["qpos0"], np.float64)[None], (N, 1)) + rng.normal(scale=0.3, size=(N, len(A["qpos0"])))
    d = np.clip(rng.normal(scale=0.3, size=(N, nv)), -1.0, 1.0)
    rot = [(k, qa) for k, (what, qa, ax) in enumerate(columns(A, nv)) if what == "rot" and ax == 0]
    assert rot and len(rot) < nv / 3, kind                     # free joints and hinges
    for k, qa in rot:
        quat = rng.normal(size=(N, 4))
        q[:, qa:qa + 4] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        d[:, k:k + 3] /= np.maximum(1.0, np.linalg.norm(d[:, k:k + 3], axis=1, keepdims=True))
    q.flags.writeable = d.flags.writeable = False
    return A, nv, q, d


def _bound(q, d):
    return 32.0 * EPS64 * max(1.0, np.abs(q).max() + np.abs(d).max())


@pytest.mark.parametrize("kind", KINDS)
def test_differentiate_pos_undoes_moved(kind):
    A, nv, q, d = _inputs(kind)
    back = differentiate_pos(A, nv, moved(A, nv, q, d), q)
    err = np.abs(back - d).max()
    print(kind, "max |differentiate_pos(moved(q, d), q) - d| %.3e, bound %.3e" % (err, _bound(q, d)))
    assert err <= _bound(q, d)


@pytest.mark.parametrize("kind", KINDS)
def test_integrate_pos_is_moved_along_one_column(kind):
    A, nv, q, _ = _inputs(kind)
    for dlt in (1e-3, -0.3):
        for k in range(nv):
            d = np.zeros((N, nv))
            d[:, k] = dlt
            err = np.abs(integrate_pos(A, nv, q, k, dlt) - moved(A, nv, q, d)).max()
            assert err <= _bound(q, d), (kind, k, dlt, err)


@pytest.mark.parametrize("kind", KINDS)
def test_differentiate_pos_of_a_state_with_itself_is_zero(kind):
    A, nv, q, _ = _inputs(kind)
    assert (differentiate_pos(A, nv, q, q) == 0.0).all()
