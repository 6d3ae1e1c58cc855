"""The Newton solver's leaf functions (rsr_mjx_amd/csrc/rsr_solver.hpp) called directly on the device (tests/device/solver_rows.hip,
one wave per problem) and held to plain fp64 (tests/solver_rows_ref.py, checked on the CPU by tests/test_solver_rows_ref.py):
rows_cost, the line search's 1-D model (ls_prepare, ls_point, ls_eval<3>, ls_costs) and the Jacobian products jdot / jt_force, for
the four row shapes the product ships (CubeDims, TShapeDims, Go2FlatDims, HandDims), 256 waves each, on the build with the
product's flags and on the one without fma contraction.  Nothing here is about convergence, iteration counts or the Hessian.

Every bound is c x 2^-24 x (sum of the magnitudes of the terms as the kernel forms them), c counted from the code
(solver_rows_ref's docstring); none was fitted to a measurement.  Each test prints the worst err / bound per Dims and build.

Padding.  ls_prepare guards the rows >= nefc itself (test_ls_ignores_what_padding_lanes_hold gives those lanes values that would
contribute).  rows_cost and jdot have no such guard in a chunk that is partly live: they RELY on make_constraint's padding
{D 0, floss -1, mu 0, bn = bk = NBASE}, jaref = 0 and bval[NBASE] = 0, and are tested under that padding only.

Measured (MI355X), worst err / bound over the 256 waves, the larger of the two builds:

                 rows_cost              1-D model                  J products
    Dims         cost   shares lane    d0     2 q2   cost         jdot   jt_force adjoint
    CubeDims     0.298  0.337  0.358   0.306  0.234  0.241        0.271  0.132    0.070
    TShapeDims   0.182  0.313  0.479   0.235  0.306  0.216        0.290  0.127    0.064
    Go2FlatDims  0.364  0.302  0.407   0.234  0.223  0.310        0.253  0.261    0.092
    HandDims     0.223  0.273  0.342   0.232  0.190  0.216        0.266  0.213    0.097
    force, hw, the thresholds' q1 / q2 / force / hw / row cost and the padding test: bit for bit.  ls_eval<3> against three
    ls_point: q1, q2 and the costs bit for bit on BOTH builds (0 of 1536 values differ under the product's flags).

Single edits of rsr_solver.hpp this file catches (each built apart and loaded through RSR_SOLVER_ROWS_LIB / _STRICT_LIB):
x <= -rf -> < in rows_cost, x >= thi -> > in ls_eval, x < 0 -> <= in ls_costs' later chunks, the sign of c1p
(test_thresholds_exactly; the last also test_line_search_model_against_fp64); ls_prepare's per-chunk `lane + 64 ch >= nefc` guard
dropped (test_ls_ignores_what_padding_lanes_hold); the - of one pyramid edge in jt_force's fold, the quartet tail reading row
b + 3 instead of the null row (Go2Flat, Hand: NBC = 3; with NBC = 4 a contact's base rows fill quartets and there is no tail),
dgw skipped in the one-group branch (test_jdot_and_jt_force_against_fp64; the tail also the poison test).  Dropping ls_prepare's
LAST line (`if (lane >= nefc)` tlo = thi = inf) changes nothing and no test can see it: such a lane is a unilateral row, the
per-chunk guard has already set its ja = 1, v = 0 and b0 = b1 = b2 = 0, so x = 1 takes the upper piece c0p = c1p = 0 where the
guarded lane takes the quadratic piece 0 -- the same +0 in q0, q1 and q2.
"""
import numpy as np
import pytest

import device_harness as DH
import solver_rows_ref as R
from test_solver_rows_ref import cases

pytestmark = pytest.mark.gpu

BUILDS = [pytest.param(False, id="product"), pytest.param(True, id="strict")]
_RUN = {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def worst(err, bound):
    """(every error within its bound, the largest err / bound); a zero bound asks for a zero error"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    ok = bool((err <= bound).all())
    pos = bound > 0
    return ok, float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def report(what, name, strict, **ratios):
    print("%-10s %-12s %-8s " % (what, name, "strict" if strict else "product") + "  ".join("%s %.3f" % kv for kv in ratios.items()))


def _model_args(c):
    return c["nefc"], c["jaref"], c["jv"], c["D"], c["R"], c["floss"], c["g"], c["alpha"]


def run(name, strict):
    """the kernels' outputs on the Dims' shared cases, once per build"""
    if (name, strict) not in _RUN:
        d, c, j = cases(name)
        rc = DH.rows_cost(name, c["nefc"], c["jaref"], c["D"], c["R"], c["floss"], strict=strict)
        ls = DH.linesearch(name, *_model_args(c), strict=strict)
        jp = DH.jproducts(name, *[j[k] for k in ("nl", "ncon", "B", "bmu", "sdof", "mu", "bn", "bk", "v", "force")], strict=strict)
        _RUN[(name, strict)] = (rc, ls, jp)
    return _RUN[(name, strict)]


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_rows_cost_against_fp64(name, strict):
    d, c, _ = cases(name)
    rc = run(name, strict)[0]
    ref = R.rows_cost_ref(d, c)
    assert same_bits(rc.cost, np.repeat(rc.cost[:, :1], 64, 1))                      # the reduced cost: the same bits in every lane
    ok, ratio = worst(np.abs(rc.cost[:, 0].astype(np.float64) - ref["cost"]), ref["bound"])
    # the shares of the lanes, summed in fp64, against the reduced cost: the six levels of wave_sum (+ 2, as every bound)
    share = rc.cost_lane.astype(np.float64)
    ok_s, ratio_s = worst(np.abs(share.sum(1) - rc.cost[:, 0]), (6 + 2) * R.U * np.abs(share).sum(1))
    # a lane's share is the sum of its rows' costs (the terms' roundings and the NCHUNK - 1 serial adds)
    ok_l, ratio_l = worst(np.abs(share - ref["lane"]), ref["lane_bound"])
    report("rows_cost", name, strict, cost=ratio, shares=ratio_s, lane=ratio_l)
    assert ok and ok_s and ok_l, (ratio, ratio_s, ratio_l)
    # force: float32(-(D x)) on active rows, +-floss on saturated friction rows, 0 elsewhere; hw: D or +0 -- bit for bit, from
    # both instantiations (the solver compares hw with != to decide whether the factor can be reused)
    for k in range(2):
        assert same_bits(R.by_row(rc.force[:, k]), ref["force"].astype(np.float32)), k
        assert same_bits(R.by_row(rc.hw[:, k]), ref["hw"].astype(np.float32)), k
    act = ref["piece"] == R.QUAD
    assert same_bits(R.by_row(rc.hw[:, 0])[act], R.by_row(c["D"])[act]) and (bits(R.by_row(rc.hw[:, 0])[~act]) == 0).all()


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_line_search_model_against_fp64(name, strict):
    d, c, _ = cases(name)
    ls = run(name, strict)[1]
    m = R.model_ref(d, c)
    assert np.isfinite(ls.pt).all() and np.isfinite(ls.ev).all() and np.isfinite(ls.cost).all()      # 1e15 included
    ratios, good = {}, True
    for tag, p, cost in (("point", ls.pt, ls.cost[:, 0]), ("eval3", ls.ev, ls.cost[:, 1])):
        p = p.astype(np.float64)
        for what, err, bound in (("d0", np.abs(p[:, :, 2] - m["dphi"]), m["b_d0"]), ("2q2", np.abs(2 * p[:, :, 1] - m["ddphi"]), m["b_q2"]),
                                 ("cost", np.abs(cost.astype(np.float64) - m["phi"]), m["b_cost"])):
            ok, ratios[f"{tag}.{what}"] = worst(err, bound)
            good &= ok
    report("linesearch", name, strict, **ratios)
    assert good, ratios
    # d1(): RSR_MINVAL exactly where no row is on its quadratic piece and g2 = 0, 2 q2 everywhere else
    floor = (m["nquad"] == 0) & (c["g"][:, 2:3] == 0)
    assert floor.sum() >= 48 and (c["alpha"][floor.any(1)] == np.float32(1e15)).any()
    for p in (ls.pt, ls.ev):
        assert (bits(p[:, :, 3][floor]) == bits(R.MINVAL)).all() and (p[:, :, 1][floor] == 0).all()
        assert same_bits(p[:, :, 3][~floor], np.float32(2) * p[:, :, 1][~floor]) and (p[:, :, 3][~floor] != R.MINVAL).all()
        if strict:                                                              # d0() as written, every operation rounded
            assert same_bits(p[:, :, 2], np.float32(2) * c["alpha"] * p[:, :, 1] + p[:, :, 0])


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_thresholds_exactly(name, strict):
    """Single rows on dyadic numbers (solver_rows_ref.threshold_cases): x == -rf takes the lower linear piece, x == +rf the upper
    one, x == 0 leaves a unilateral row off (chunk 0 and chunk 1); one fp32 step inside is quadratic.  q1, q2, force, hw and the
    row cost are the reference's, bit for bit (a sum of zeros may come out as -0: compared after + 0), from rows_cost, ls_point
    and ls_eval<3> alike; at the thresholds themselves, where every number is exact, so is ls_costs' cost."""
    d = DH.sr_dims(name)
    c, want = R.threshold_cases(d)
    m = R.model_ref(d, c)
    ls = DH.linesearch(name, *_model_args(c), strict=strict)
    al = c["alpha"].astype(np.float64)
    q2 = (0.5 * m["ddphi"]).astype(np.float32)
    q1 = (m["dphi"] - al * m["ddphi"]).astype(np.float32)
    x = (R.by_row(c["jaref"]).astype(np.float64) + al[:, :1] * R.by_row(c["jv"])).astype(np.float32)
    cx = dict(c, jaref=x.reshape(c["jaref"].shape))
    rc = DH.rows_cost(name, c["nefc"], cx["jaref"], c["D"], c["R"], c["floss"], strict=strict)
    ref = R.rows_cost_ref(d, cx)
    zero = np.float32(0)
    for i, (r, p, what) in enumerate(want):
        assert m["piece"][i, 0, r] == p and ref["piece"][i, r] == p, what
        for k in (0, 2):
            for pts in (ls.pt, ls.ev):
                assert same_bits(pts[i, k, 0] + zero, q1[i, k] + zero) and same_bits(pts[i, k, 1] + zero, q2[i, k] + zero), (what, pts[i, k], q1[i, k], q2[i, k])
        assert (q2[i, 0] != 0) == (p == R.QUAD), what                               # the case can tell the pieces apart
        for k in range(2):
            assert same_bits(R.by_row(rc.force[:, k])[i], ref["force"][i].astype(np.float32)), what
            assert same_bits(R.by_row(rc.hw[:, k])[i], ref["hw"][i].astype(np.float32)), what
        assert (R.by_row(rc.hw[:, 0])[i, r] != 0) == (ls.pt[i, 0, 1] != 0) == (p == R.QUAD), what          # rows_cost and ls_eval agree
        assert rc.cost[i, 0] == np.float32(ref["cost"][i]), (what, rc.cost[i, 0], ref["cost"][i])
        if "==" in what:
            assert (ls.cost[i, :, 0] == np.float32(m["phi"][i, 0])).all(), (what, ls.cost[i], m["phi"][i, 0])
    ok, ratio = worst(np.abs(ls.cost.astype(np.float64) - m["phi"][:, None, :]), m["b_cost"][:, None, :] + 0 * ls.cost)
    report("thresholds", name, strict, cost=ratio, cases=len(want))
    assert ok


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_ls_ignores_what_padding_lanes_hold(name, strict):
    d, c, _ = cases(name)
    ls = run(name, strict)[1]
    pad = (R.row_kinds(d, c["nefc"]) == R.PAD).reshape(c["jaref"].shape)
    assert pad.any(2).all(1).sum() > 0 and pad.sum() > 1000                 # waves with padding lanes in every chunk among them
    loud = dict(c)
    for k, v in (("jaref", -5.0), ("jv", 3.0), ("D", 2.0)):
        loud[k] = np.where(pad, np.float32(v), c[k])
    got = DH.linesearch(name, *_model_args(loud), strict=strict)
    for a, b in zip(got, ls):
        assert same_bits(a, b)
    report("padding", name, strict, lanes=float(pad.sum()))


@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_ls_eval3_is_three_ls_points(name):
    """q1 and q2 bit for bit on the build without contraction (device_harness.UNITS: under the product's flags the compiler
    fuses x = ja + alpha v as it likes in each instantiation); within the derived bounds of d0 and 2 q2 on the product's."""
    d, c, _ = cases(name)
    strict, prod = run(name, True)[1], run(name, False)[1]
    assert same_bits(strict.pt[:, :, :2], strict.ev[:, :, :2]) and same_bits(strict.cost[:, 0], strict.cost[:, 1])
    m = R.model_ref(d, c)
    p, e = prod.pt.astype(np.float64), prod.ev.astype(np.float64)
    ok1, r1 = worst(np.abs(p[:, :, 2] - e[:, :, 2]), m["b_d0"])
    ok2, r2 = worst(2 * np.abs(p[:, :, 1] - e[:, :, 1]), m["b_q2"])
    report("eval3", name, False, d0=r1, q2=r2, differing=float((bits(prod.pt[:, :, :2]) != bits(prod.ev[:, :, :2])).sum()))
    assert ok1 and ok2


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_jdot_and_jt_force_against_fp64(name, strict):
    d, _, j = cases(name)
    jp = run(name, strict)[2]
    ref = R.j_ref(d, j)
    jd, qfc = R.by_row(jp.jd).astype(np.float64), jp.qfc.astype(np.float64)
    assert np.isfinite(jd).all() and np.isfinite(qfc).all()                  # no poisoned word was read
    live = np.arange(d.NCHUNK * 64)[None, :] < j["nefc"][:, None]
    assert (jd[~live] == 0).all() and (bits(jp.qfc[:, d.NV:]) == 0).all()     # rows >= nefc, lanes >= NV: exactly 0
    ok_v, r_v = worst(np.abs(jd - ref["jv"]), ref["b_jv"])
    ok_f, r_f = worst(np.abs(qfc[:, :d.NV] - ref["qfc"]), ref["b_qfc"])
    # adjointness, from the kernels' own fp32 outputs: f.(J v) = (J^T f).v within the two bounds
    f, v = R.by_row(R.f64(j["force"])), R.f64(j["v"])
    lhs, rhs = (f * jd).sum(1), (qfc[:, :d.NV] * v).sum(1)
    ok_a, r_a = worst(np.abs(lhs - rhs), (np.abs(f) * ref["b_jv"]).sum(1) + (np.abs(v) * ref["b_qfc"]).sum(1))
    report("jproducts", name, strict, jdot=r_v, jt_force=r_f, adjoint=r_a, c_jt=ref["c_qfc"])
    assert ok_v and ok_f and ok_a, (r_v, r_f, r_a)
    assert np.abs(ref["jv"]).max() > 1 and np.abs(ref["qfc"]).max() > 1


@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_j_products_do_not_depend_on_the_poison(name):
    """the words outside the contract (solver_rows.hip) hold NaN in every other test; with a finite value there instead, every
    output keeps its bits"""
    d, _, j = cases(name)
    jp = run(name, False)[2]
    other = DH.jproducts(name, *[j[k] for k in ("nl", "ncon", "B", "bmu", "sdof", "mu", "bn", "bk", "v", "force")], poison=-12345.678)
    assert same_bits(other.jd, jp.jd) and same_bits(other.qfc, jp.qfc)
