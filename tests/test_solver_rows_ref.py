"""The test-only HIP unit of the Newton solver's leaf functions (tests/device/solver_rows.hip, tests/device_harness.py) on the CPU:
it compiles for gfx950 on both builds and exports its entry points; and the plain fp64 reference that
tests/test_solver_rows_gpu.py holds the kernels to (tests/solver_rows_ref.py), checked against itself and against the oracle:
central differences of phi confirm phi' and phi'' where no row changes its piece, a row's cost and force are continuous across
its thresholds, phi(0) - g0 is the sum of the row costs, the generators leave no row inside the threshold margin, drop no wave
and cover every row kind, piece and chunk they claim.

The oracle reports the pyramid Jacobian efc_J, not the contact-frame base rows or the friction coefficients the reference
assembles it from, so "J_pyr equals the oracle's Jacobian" is checked as far as that allows: the base rows are read off the
oracle's own rows (normal = half the sum of an edge pair, mu_k x direction k = half its difference) and the reference's
assembly -- row layout r_lim / r_con, bn / bk, the sign by (e & 1) -- must give back every row of efc_J, which it does only if
all edge pairs of a contact share one normal row and come in the order the reference assumes."""
import os

import numpy as np
import pytest

import device_harness as DH
import solver_rows_ref as R

_CASES = {}


def cases(name):
    """(d, model_cases, j_cases) of one Dims, built once and read-only"""
    if name not in _CASES:
        d = DH.sr_dims(name)
        _CASES[name] = (d, R.model_cases(d), R.j_cases(d))
    return _CASES[name]


def test_solver_rows_unit_compiles_and_exports():
    path = DH.build(unit="solver_rows")
    assert os.path.exists(path) and os.path.dirname(path) == DH.BUILD_DIR
    u, us = DH.UNITS["solver_rows"], DH.UNITS["solver_rows_strict"]
    assert u.flags == [] and us.flags == ["-ffp-contract=off"] and us.src == u.src
    assert (u.env, us.env) == ("RSR_SOLVER_ROWS_LIB", "RSR_SOLVER_ROWS_STRICT_LIB")
    strict = DH.build(unit="solver_rows_strict")
    assert os.path.exists(strict) and strict != path
    for L in (DH.sr_lib(), DH.sr_lib(strict=True)):
        for sym in DH.SR_SYMBOLS:
            getattr(L, sym)
        assert L.rsr_sr_rows_cost(0, 0, *[None] * 9) == -1 and L.rsr_sr_linesearch(0, 0, *[None] * 11) == -1
        assert L.rsr_sr_jproducts(0, 0, *[None] * 6, 0.0, *[None] * 7) == -1
    assert not DH._stale("solver_rows") and not DH._stale("solver_rows_strict")
    want = {"CubeDims": (3, 1), "TShapeDims": (4, 1), "Go2FlatDims": (1, 0), "HandDims": (2, 0)}
    for name in DH.SR_DIMS:
        d = DH.sr_dims(name)
        assert (d.NCHUNK, d.NEQ) == want[name]
        assert d.NEFC == d.NEQ + d.NF + d.NL + d.NPYR * d.NCON and d.NBASE == d.NEQ + d.NF + d.NL + d.NBC * d.NCON
        assert d.NCHUNK == (d.NEFC + 63) // 64 and d.NPYR == 2 * (d.NBC - 1) and d.LDJ >= d.NV and d.LDJ % 4 == 0
    assert DH.sr_lib().rsr_sr_dims(DH.DIMS["Go2Dims"], (DH.C.c_int * 11)()) == -1


@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_generators_keep_the_margin_drop_nothing_and_cover_what_they_claim(name):
    d, c, j = cases(name)
    assert len(c["nefc"]) == R.NWAVE and len(j["nefc"]) == R.NWAVE                   # no wave dropped
    assert not R.threshold_violations(d, c).any()
    # the margin is meant: a row moved onto its threshold is found
    moved = {k: np.array(v) for k, v in c.items()}
    r = d.NEQ + d.NF                                                                 # the first limit row, at the first step size
    e = int(np.argmax(c["nefc"] > r))
    moved["jaref"][e, 0, r] = -np.float32(c["alpha"][e, 1]) * c["jv"][e, 0, r]
    assert c["nefc"][e] > r and c["alpha"][e, 1] != 0 and R.threshold_violations(d, moved)[e, r]
    kind = R.row_kinds(d, c["nefc"])
    pad = kind == R.PAD
    for k, v in (("jaref", 0), ("jv", 0), ("D", 0), ("R", 1), ("floss", -1)):
        assert (R.by_row(c[k])[pad] == v).all(), k
    assert (R.by_row(c["floss"])[kind == R.FRIC] >= 0).all() and (R.by_row(c["floss"])[(kind == R.EQ) | (kind == R.UNI)] == -1).all()
    D = R.by_row(c["D"])[~pad]
    assert D[D > 0].min() < 0.02 and D.max() > 5e5
    census = R.model_census(d, c)
    print(name, census)
    empty = [k for k, v in census.items() if v == 0 and k != "ja redrawn for the margin"]
    assert not empty, empty
    m = R.model_ref(d, c)
    assert (m["nquad"][c["flat"]] == 0).all() and (c["g"][c["flat"], 2] == 0).all() and c["flat"].sum() >= 16
    al = np.abs(c["alpha"])
    assert (c["alpha"] == 0).any() and (c["alpha"] < 0).any() and (al == np.float32(1e6)).any() and (al == np.float32(1e15)).any()
    assert np.abs(m["phi"]).max() < 2.0 ** 120 and (m["b_cost"] / R.U).max() < 2.0 ** 125      # the model stays inside fp32
    # Jacobian products: the structures, and the rows as make_constraint leaves them
    sc = R.structure_census(d, j["nl"], j["ncon"])
    assert all(v > 0 for v in sc.values()), sc
    live = np.arange(d.NCHUNK * 64)[None, :] < j["nefc"][:, None]
    bn, bk, mu, f = (R.by_row(j[k]) for k in ("bn", "bk", "mu", "force"))
    assert (bn[~live] == d.NBASE).all() and (bk[~live] == d.NBASE).all() and (mu[~live] == 0).all() and (f[~live] == 0).all()
    assert (mu == 0).any() and ((np.abs(mu) > 0) & (np.abs(mu) < 0.01)).any() and (np.abs(mu) > 1).any() and (mu < 0).any()
    assert (f[live] == 0).mean() > 0.2 and j["nbase"].max() == d.NBASE and (bn[live] < j["nbase"][:, None].repeat(bn.shape[1], 1)[live]).all()
    for e in (0, 17, 255):                                   # friction and limit rows: one +-1 each, on distinct dofs of their kind
        rl, rc = d.NEQ + d.NF, d.NEQ + d.NF + j["nl"][e]
        assert (np.abs(j["B"][e, d.NEQ:rc]).sum(1) == 1).all()
        assert len(set(j["sdof"][e, d.NEQ:rl])) == d.NF and len(set(j["sdof"][e, rl:rc])) == j["nl"][e]
        assert (np.abs(j["B"][e, np.arange(d.NEQ, rc), j["sdof"][e, d.NEQ:rc]]) == 1).all()
    shared = [len(set(j["sdof"][e, d.NEQ:d.NEQ + d.NF]) & set(j["sdof"][e, d.NEQ + d.NF:d.NEQ + d.NF + j["nl"][e]])) for e in range(R.NWAVE)]
    assert max(shared) > 0                                   # a friction row and a limit row on one dof


@pytest.mark.parametrize("name", DH.SR_DIMS)
def test_derivatives_by_central_differences(name):
    """phi' and phi'' against central differences of phi itself, fp64, at every (wave, step size) where no row changes its piece
    within the stencil (most: asserted).  phi is piecewise quadratic, so both differences are exact up to the rounding of phi,
    64 x 2^-53 x (sum of the magnitudes of phi's terms) / h and / h^2."""
    d, c, _ = cases(name)
    al = c["alpha"].astype(np.float64)
    h = 1e-4 * np.maximum(1.0, np.abs(al))
    m0, mp, mm = R.model_ref(d, c), R.model_ref(d, c, al + h), R.model_ref(d, c, al - h)
    same = (mp["piece"] == m0["piece"]).all(2) & (mm["piece"] == m0["piece"]).all(2)
    assert same.mean() > 0.5, same.mean()
    mag = np.maximum.reduce([x["b_cost"] for x in (m0, mp, mm)]) / R.U
    e1 = np.abs((mp["phi"] - mm["phi"]) / (2 * h) - m0["dphi"])
    e2 = np.abs((mp["phi"] - 2 * m0["phi"] + mm["phi"]) / (h * h) - m0["ddphi"])
    t1, t2 = 64 * 2.0 ** -53 * mag / h, 64 * 2.0 ** -53 * mag / (h * h)
    print(name, "points %d of %d; worst err / tol: phi' %.3g, phi'' %.3g" % (same.sum(), same.size, (e1 / t1)[same].max(), (e2 / t2)[same].max()))
    assert (e1 <= t1)[same].all() and (e2 <= t2)[same].all()
    # and the check can see an error: the tolerance is far below the derivative on most points
    assert np.median((t1 / np.maximum(np.abs(m0["dphi"]), 1e-300))[same]) < 1e-3


def test_row_cost_is_continuous_across_its_thresholds_and_phi0_is_the_row_sum():
    rng = np.random.default_rng(5)
    n = 4096
    D, fl = 10.0 ** rng.uniform(-2, 6, n), 10.0 ** rng.uniform(-3, 3, n)
    R_ = 1.0 / D                        # (the friction row's pieces meet only where D R = 1, as make_constraint sets them)
    rf, eps = R_ * fl, 1e-9
    for kind, thr in ((R.FRIC, -rf), (R.FRIC, rf), (R.UNI, np.zeros(n))):
        k = np.full(n, kind)
        step = eps * np.where(thr == 0, 1.0, np.abs(thr))
        c0, f0, _, p0 = R.row_cost(k, thr - step, D, R_, fl)
        c1, f1, _, p1 = R.row_cost(k, thr + step, D, R_, fl)
        ca, fa, _, pa = R.row_cost(k, thr, D, R_, fl)
        assert (p0 != p1).all()                                                    # a threshold: the piece changes across it
        scale_c, scale_f = np.abs(ca) + D * step * step + fl * step, np.abs(fa) + D * step
        assert (np.abs(c1 - c0) <= 4 * eps * scale_c + 4 * (np.abs(f0) + np.abs(f1)) * step).all(), kind
        assert (np.abs(f1 - f0) <= 4 * D * step + 1e-12 * scale_f).all(), kind
    # at the thresholds themselves: the linear pieces own +-rf, the unilateral row is off at 0
    assert (R.row_cost(np.full(n, R.FRIC), -rf, D, R_, fl)[3] == R.LOWER).all() and (R.row_cost(np.full(n, R.FRIC), rf, D, R_, fl)[3] == R.UPPER).all()
    assert (R.row_cost(np.full(n, R.UNI), np.zeros(n), D, R_, fl)[3] == R.OFF).all()
    for name in DH.SR_DIMS:
        d, c, _ = cases(name)
        m = R.model_ref(d, c, np.zeros((R.NWAVE, 3)))
        rc = R.rows_cost_ref(d, c)
        g0 = c["g"][:, 0].astype(np.float64)
        assert (np.abs(m["phi"][:, 0] - g0 - rc["cost"]) <= 1e-13 * (rc["S"] + np.abs(g0))).all(), name
        # force and weight are the derivatives of the cost (central differences in x, away from the thresholds)
        kind, ja, D_, R2, f2 = R._rows(d, c)
        hx = 1e-5 * np.maximum(np.abs(ja), 1e-3)
        cp, _, _, pp = R.row_cost(kind, ja + hx, D_, R2, f2)
        cm, _, _, pm = R.row_cost(kind, ja - hx, D_, R2, f2)
        same = (pp == rc["piece"]) & (pm == rc["piece"])
        tol = 1e-9 * (np.abs(cp) + np.abs(cm) + 1e-300) / hx
        assert same.mean() > 0.9 and (np.abs(-(cp - cm) / (2 * hx) - rc["force"]) <= tol + 1e-9 * np.abs(rc["force"]))[same].all(), name


def test_threshold_cases_are_exact_in_fp32():
    for name in DH.SR_DIMS:
        d = DH.sr_dims(name)
        c, want = R.threshold_cases(d)
        m = R.model_ref(d, c)
        for i, (r, p, what) in enumerate(want):
            ja, v, a = (np.float32(x) for x in (R.by_row(c["jaref"])[i, r], R.by_row(c["jv"])[i, r], c["alpha"][i, 0]))
            assert np.float64(np.float32(ja + a * v)) == m["x"][i, 0, r], what                  # x is exact in fp32
            assert m["piece"][i, 0, r] == p, (name, what)
            others = np.delete(np.arange(d.NCHUNK * 64), r)
            assert (R.by_row(c["D"])[i, others] == 0).all() and (m["piece"][i, 0, others] != R.LOWER).all()
        assert len(want) == (12 if d.NCHUNK > 1 else 9)


@pytest.mark.parametrize("kind,name", [("cube", "CubeDims"), ("go2flat", "Go2FlatDims")])
def test_assembly_gives_back_the_oracles_pyramid_jacobian(oracle_mod, kind, name):
    from test_model_variants import case
    d = DH.sr_dims(name)
    rows = case(oracle_mod, None, kind)["ref"]["f64"]
    # the first state with two contacts or more, one with active limits if there is any
    e = min((i for i, r in enumerate(rows) if r["ncon"] >= 2), key=lambda i: (rows[i]["nefc"] == rows[i]["ne"] + rows[i]["nf"] + d.NPYR * rows[i]["ncon"], i))
    r = rows[e]
    nefc, ncon, J = r["nefc"], r["ncon"], r["efc_J"]
    assert (r["ne"], r["nf"]) == (d.NEQ, d.NF) and J.shape == (nefc, d.NV)
    nl = nefc - d.NEQ - d.NF - d.NPYR * ncon
    rcon = d.NEQ + d.NF + nl
    nr = d.NCHUNK * 64
    B, bmu = np.zeros((1, d.NBASE, d.NV)), np.zeros((1, d.NBASE))
    mu, bn, bk = np.zeros((1, nr)), np.full((1, nr), d.NBASE), np.full((1, nr), d.NBASE)
    B[0, :rcon] = J[:rcon]
    bn[0, :rcon] = bk[0, :rcon] = np.arange(rcon)
    for c in range(ncon):
        r0, b0 = rcon + d.NPYR * c, rcon + d.NBC * c
        B[0, b0] = 0.5 * (J[r0] + J[r0 + 1])
        for k in range(1, d.NBC):
            B[0, b0 + k], bmu[0, b0 + k] = 0.5 * (J[r0 + 2 * (k - 1)] - J[r0 + 2 * (k - 1) + 1]), 1.0
        for ed in range(d.NPYR):
            bn[0, r0 + ed], bk[0, r0 + ed], mu[0, r0 + ed] = b0, b0 + 1 + (ed >> 1), -1.0 if ed & 1 else 1.0
    sh = (1, d.NCHUNK, 64)
    c = dict(nefc=np.array([nefc]), B=B, mu=mu.reshape(sh), bn=bn.reshape(sh), bk=bk.reshape(sh))
    Jp, _ = R.j_pyramid(d, c)
    err = np.abs(Jp[0, :nefc] - J).max() / np.abs(J).max()
    print(kind, "state", e, "nefc", nefc, "nl", nl, "ncon", ncon, "max |J_pyr - efc_J| / max |efc_J| = %.3g" % err)
    assert err <= 4 * R.U and (Jp[0, nefc:] == 0).all()                      # (j_pyramid takes its base rows as fp32 numbers)
    assert np.abs(J[rcon:]).max() > 0 and np.abs(B[0, rcon + 1]).max() > 0
