"""The in-register L D L^T layouts (chol / rowchol / rowtree / arrow factor and solve), the wave sums and the reciprocals of
rsr_mjx_amd/csrc/rsr_device.hpp, called directly (tests/device/primitives.hip: one wave per problem, raw lane registers dumped)
and compared with plain fp64 -- independent of the oracle's solver, the contact model and the Newton loop.

Inputs: 256 matrices per case, built in fp64 and rounded to fp32 (every reference below starts from the rounded matrix):
synthetic SPD matrices S (I + J^T D J) S in the sparsity each layout assumes, condition numbers 1e1 .. 1e5
(test_device_primitives.synthetic_spd), and the fp64 oracle's mass matrices at perturbed poses of each shipped model.

Accuracy rule (set before measuring): the normwise backward error eta = |b - H x|_inf / (|H|_inf |x|_inf + |b|_inf) of the
kernel's solve, and |H - L D L^T|_inf / |H|_inf of the dumped factors, both in fp64, may be at most 4 x the maximum of the same
figure of test_device_primitives.ldlt / ldlt_solve on the same inputs -- natural-order L D L^T in numpy float32: exact division,
no fusion -- with a floor of NV * 2^-24.  The margin covers rcp + one Newton step for the division, fused updates and the arrow
layout's elimination order.

Combinations covered = every one rsr_solver.hpp instantiates (hessian_factor, forward, integrate), each with the scratch
aliased onto the matrix and apart; the natural order is the bit reference and compiles for every Dims:

    layout   template arguments                      Dims
    natural  <C>, <C,true>  (+ the caller's diag)    CubeDims TShapeDims Go2FlatDims Go2Dims HandDims
    rowchol  <C,false>, <C,true>, <C,true,true>      CubeDims TShapeDims
    rowtree  <C>, <C,true>                           CubeDims TShapeDims
    arrow    <C>, <C,true>                           Go2FlatDims Go2Dims HandDims

Measured maxima over all modes, both alias settings and both input families (MI355X; kernel / numpy-float32 reference):

    layout   Dims          eta (kernel / reference)   |H - L D L^T| / |H| (kernel / reference)
    natural  CubeDims      1.04e-07 / 7.55e-08        1.64e-07 / 1.21e-07
    natural  TShapeDims    1.14e-07 / 1.28e-07        1.35e-07 / 1.31e-07
    natural  Go2FlatDims   1.65e-07 / 1.65e-07        2.08e-07 / 1.96e-07
    natural  Go2Dims       1.44e-07 / 1.34e-07        1.25e-07 / 1.21e-07
    natural  HandDims      1.31e-07 / 1.45e-07        1.75e-07 / 1.68e-07
    rowchol  CubeDims      1.04e-07 / 7.55e-08        1.64e-07 / 1.21e-07
    rowchol  TShapeDims    1.14e-07 / 1.28e-07        1.35e-07 / 1.31e-07
    rowtree  CubeDims      8.13e-08 / 7.55e-08        1.44e-07 / 1.11e-07
    rowtree  TShapeDims    1.14e-07 / 1.28e-07        1.16e-07 / 1.22e-07
    arrow    Go2FlatDims   1.36e-07 / 1.65e-07        1.91e-07 / 1.96e-07
    arrow    Go2Dims       1.50e-07 / 1.34e-07        1.85e-07 / 1.21e-07
    arrow    HandDims      1.15e-07 / 1.45e-07        1.99e-07 / 1.68e-07

Every bit identity the header claims held on all inputs (and the solutions x of rowchol / rowtree equal the natural order's too).

Reciprocals, distance in fp32 ulps between the result and the correctly rounded fp64 result, measured maxima:

    frcp 0 (every argument with a normal reciprocal came back correctly rounded), frsq 1, fsqrt 1.  frcp of the largest subnormal
    is NaN and a reciprocal below the normal range comes back as zero: both outside the header's stated domain (see the test).
"""
import numpy as np
import pytest

import device_harness as DH
from test_device_primitives import (MINVAL, SPARSITY_OF_DIMS, U32, backward_error, decode, elimination_order, in_block, lane_table,
                                    lanes_of_dof, ldlt, ldlt_solve, rebuild_error, synthetic_spd)

pytestmark = pytest.mark.gpu

N = 256
MO, HD = DH.MASS_ONLY, DH.HAS_DIAG
AIRBOT, GO2 = ("CubeDims", "TShapeDims"), ("Go2FlatDims", "Go2Dims", "HandDims")
# (layout, Dims, mode, sparsity of the synthetic input): everything the product instantiates
CASES = ([("natural", dn, m, sp) for dn in AIRBOT for m, sp in ((0, "coupled"), (MO, "trees"), (HD, "trees"), (MO | HD, "trees"))]
         + [("natural", dn, m, "arrow") for dn in GO2 for m in (0, MO, HD, MO | HD)]
         + [("rowchol", dn, m, sp) for dn in AIRBOT for m, sp in ((0, "coupled"), (MO, "trees"), (MO | HD, "trees"))]
         + [("rowtree", dn, m, "trees") for dn in AIRBOT for m in (0, HD)]
         + [("arrow", dn, m, "arrow") for dn in GO2 for m in (0, HD)])
CASE_IDS = ["%s-%s-%d-%s" % c for c in CASES]
MODEL_OF_DIMS = {"CubeDims": "cube", "TShapeDims": "tshape", "Go2FlatDims": "Go2JoystickFlatTerrain",
                 "Go2Dims": "Go2JoystickRoughTerrain", "HandDims": "Go2Handstand"}

_CACHE = {}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _synthetic(dims_name, sparsity):
    key = ("syn", dims_name, sparsity)
    if key not in _CACHE:
        H, b, diag, dropped, _ = synthetic_spd(dims_name, sparsity, N)
        assert dropped <= 0.05 and len(H) == N
        for v in (H, b, diag):
            v.setflags(write=False)
        _CACHE[key] = (H, b, diag)
    return _CACHE[key]


def _mass_matrices(dims_name, oracle_mod):
    """The fp64 oracle's qM at N perturbed poses of the Dims' shipped model, rounded to fp32; a right-hand side and a damping-like
    diagonal to go with it."""
    key = ("qM", dims_name)
    if key in _CACHE:
        return _CACHE[key]
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.model import model_fields, pack_blob
    name = MODEL_OF_DIMS[dims_name]
    env = airbot.AirbotPlayBase() if name == "cube" else airbot.AirbotTShape() if name == "tshape" else go2.load(name)
    f = model_fields(env.sys)
    f.update(env._fields_fn(env.sys, 0, False, **getattr(env, "_kwargs", {})))
    o = oracle_mod.Oracle(pack_blob(f), "f64")
    A = env.sys.arrays
    nq, nv, nu = env.sys.nq, env.sys.nv, len(A["actuator_ctrlrange"])
    rng = np.random.default_rng([7, DH.DIMS[dims_name]])
    Ms = np.zeros((N, nv, nv))
    for e in range(N):
        qpos = np.array(A["qpos0"], dtype=np.float64)
        if name in ("cube", "tshape"):
            qpos[:6] += np.array([0, -0.5422302, 0.45173569, 1.5718, -1.4794435, 1.1731174])
        for jt, qa in zip(A["jnt_type"], A["jnt_qposadr"]):
            if jt == 0:                                             # free joint: position and orientation
                qpos[qa:qa + 3] += rng.uniform(-0.05, 0.05, 3)
                q = qpos[qa + 3:qa + 7] + rng.uniform(-0.3, 0.3, 4)
                qpos[qa + 3:qa + 7] = q / np.linalg.norm(q)
            elif jt == 3:
                qpos[qa] += rng.uniform(-0.3, 0.3)
        o.forward(qpos, np.zeros(nv), np.zeros(nu), np.zeros(nv))
        Ms[e] = o.get("M").reshape(nv, nv)
    H = Ms.astype(np.float32)
    assert (H == H.transpose(0, 2, 1)).all()
    xt = rng.normal(size=(N, nv))
    b = np.einsum("nij,nj->ni", H.astype(np.float64), xt).astype(np.float32)
    diag = (np.diagonal(H, axis1=1, axis2=2) * 10.0 ** rng.uniform(-3, -1, size=(N, nv))).astype(np.float32)
    for v in (H, b, diag):
        v.setflags(write=False)
    _CACHE[key] = (H, b, diag)
    return _CACHE[key]


def _reference(H, b, diag, mode):
    """(eta, rebuild error, effective fp64 matrix) of the numpy-float32 natural-order restatement."""
    Hd = np.array(H, dtype=np.float32)
    Heff = H.astype(np.float64)
    if mode & HD:
        i = np.arange(H.shape[1])
        Hd[:, i, i] = Hd[:, i, i] + diag                           # one fp32 rounding, as the kernels add it
        Heff[:, i, i] += diag.astype(np.float64)
    L, D, raw = ldlt(Hd)
    assert (raw > 0).all()
    return backward_error(Heff, ldlt_solve(L, D, b), b), rebuild_error(Heff, L, D), Heff


def _kernel_errors(kind, dims_name, mode, alias, H, b, diag, Heff):
    d = DH.dims(dims_name)
    f = DH.factor(kind, dims_name, mode, H, diag=diag, b=b, alias=alias)
    L, dinv, x = decode(kind, d, f)
    assert np.isfinite(L).all() and np.isfinite(x).all() and (dinv > 0).all()
    return backward_error(Heff, x, b), rebuild_error(Heff, L, 1.0 / dinv.astype(np.float64))


@pytest.mark.parametrize("kind,dims_name,mode,sparsity", CASES, ids=CASE_IDS)
def test_factor_and_solve_accuracy_against_fp64(oracle_mod, kind, dims_name, mode, sparsity):
    """Assertion 1: eta and the rebuild error of every (layout, mode, Dims), scratch aliased and apart, on the synthetic and on
    the real mass matrices, against 4 x the numpy-float32 reference (floor NV * 2^-24)."""
    d = DH.dims(dims_name)
    fails = []
    for what, (H, b, diag) in (("synthetic " + sparsity, _synthetic(dims_name, sparsity)), ("qM", _mass_matrices(dims_name, oracle_mod))):
        ref_eta, ref_reb, Heff = _reference(H, b, diag, mode)
        for alias in (0, 1):
            eta, reb = _kernel_errors(kind, dims_name, mode, alias, H, b, diag, Heff)
            print("ACCURACY %s %s mode %d alias %d %s: eta kernel %.3e ref %.3e | rebuild kernel %.3e ref %.3e"
                  % (kind, dims_name, mode, alias, what, eta.max(), ref_eta.max(), reb.max(), ref_reb.max()))
            for label, got, ref in (("eta", eta, ref_eta), ("rebuild", reb, ref_reb)):
                bound = max(4.0 * ref.max(), d.NV * U32)
                if not got.max() <= bound:
                    fails.append(f"{what} alias {alias} {label}: kernel {got.max():.3e} > bound {bound:.3e} (reference {ref.max():.3e})")
    assert not fails, fails


def _inputs_for_identities(dims_name, sparsity, oracle_mod):
    """Synthetic and real matrices of one Dims in one batch (the identities are exact: they hold on anything)."""
    Hs, bs, ds = _synthetic(dims_name, sparsity)
    Hm, bm, dm = _mass_matrices(dims_name, oracle_mod)
    return np.concatenate([Hs, Hm]), np.concatenate([bs, bm]), np.concatenate([ds, dm])


@pytest.mark.parametrize("dims_name", AIRBOT)
def test_rowchol_bits_equal_natural_order(oracle_mod, dims_name):
    """'the factors are bit-identical to chol_factor's': rowchol_factor<C,false> against chol_factor<C> after un-permutation, and
    the mass-only variants with and without the diagonal against chol_factor<C,true>."""
    d = DH.dims(dims_name)
    for mode, sparsity in ((0, "coupled"), (MO, "trees"), (MO | HD, "trees")):
        H, b, diag = _inputs_for_identities(dims_name, sparsity, oracle_mod) if sparsity == "trees" else _synthetic(dims_name, sparsity)
        Ln, dn, xn = decode("natural", d, DH.factor("natural", dims_name, mode, H, diag=diag, b=b))
        Lr, dr, xr = decode("rowchol", d, DH.factor("rowchol", dims_name, mode, H, diag=diag, b=b))
        print("BITS rowchol-vs-natural %s mode %d: L %s dinv %s x %s" % (dims_name, mode, _same_bits(Ln, Lr), _same_bits(dn, dr), _same_bits(xn, xr)))
        assert (Ln[:, ~in_block("rowchol", d)] == 0).all()
        assert _same_bits(Ln, Lr) and _same_bits(dn, dr), (dims_name, mode)


@pytest.mark.parametrize("dims_name", AIRBOT)
def test_rowtree_bits_equal_rowchol_without_cross_tree_coupling(oracle_mod, dims_name):
    """'both layouts give the same bits': rowtree_factor<C> against rowchol_factor<C,false> (and the natural order) on matrices that
    are block diagonal over the trees; rowtree_factor<C,true> against the natural order with the caller's diagonal."""
    d = DH.dims(dims_name)
    H, b, diag = _inputs_for_identities(dims_name, "trees", oracle_mod)
    Lt, dt, xt = decode("rowtree", d, DH.factor("rowtree", dims_name, 0, H, b=b))
    Lr, dr, xr = decode("rowchol", d, DH.factor("rowchol", dims_name, 0, H, b=b))
    Ln, dn, xn = decode("natural", d, DH.factor("natural", dims_name, 0, H, b=b))
    print("BITS rowtree-vs-rowchol %s: L %s dinv %s x %s" % (dims_name, _same_bits(Lt, Lr), _same_bits(dt, dr), _same_bits(xt, xr)))
    assert _same_bits(Lt, Lr) and _same_bits(dt, dr)
    assert _same_bits(Lt, Ln) and _same_bits(dt, dn)
    Lt, dt, _ = decode("rowtree", d, DH.factor("rowtree", dims_name, HD, H, diag=diag, b=b))
    Ln, dn, _ = decode("natural", d, DH.factor("natural", dims_name, HD, H, diag=diag, b=b))
    assert _same_bits(Lt, Ln) and _same_bits(dt, dn)


@pytest.mark.parametrize("dims_name", AIRBOT + GO2)
def test_mass_only_bits_equal_the_full_variants(oracle_mod, dims_name):
    """MASS_ONLY only folds updates by structural zeros: on tree-block-diagonal input every raw register equals the full variant's."""
    d = DH.dims(dims_name)
    H, b, diag = _inputs_for_identities(dims_name, "trees" if d.ROWCHOL else "arrow", oracle_mod)
    for kind in ["natural"] + (["rowchol"] if d.ROWCHOL else []):
        full, mass = DH.factor(kind, dims_name, 0, H, b=b), DH.factor(kind, dims_name, MO, H, b=b)
        for name, u, v in zip(full._fields, full, mass):
            assert _same_bits(u[:, :d.NV] if kind == "natural" else u, v[:, :d.NV] if kind == "natural" else v), (kind, name)


def _raw_structure(kind, d, f):
    """lt[] is exactly the transpose of a[] within each block, a[] is zero from the lane's own position on, idle lanes hold zeros."""
    dof, cols, pos = lane_table(kind, d)
    nreg = f.a.shape[2]
    if kind == "natural":
        a = f.a[:, :d.NV]
        assert _same_bits(f.lt[:, :d.NV], a.transpose(0, 2, 1)), "lt != a^T"
        assert (f.lt[:, d.NV:] == 0).all() and (f.x[:, d.NV:] == 0).all()
        assert (np.triu(np.ones((d.NV, d.NV), bool))[None] * a == 0).all()
        return
    for row in range(4):
        blk = f.a[:, 16 * row:16 * row + 16]                        # [n, 16 lanes, nreg]
        want = np.zeros((f.a.shape[0], 16, nreg), dtype=np.float32)
        m = min(16, nreg)
        want[:, :m, :m] = blk[:, :m, :m].transpose(0, 2, 1)         # lt[(row, p)][k] = a[(row, k)][p]
        assert _same_bits(f.lt[:, 16 * row:16 * row + 16], want), (kind, row, "lt != a^T")
    for lane in range(64):
        if dof[lane] < 0:
            assert (f.a[:, lane] == 0).all() and (f.lt[:, lane] == 0).all(), (kind, lane, "idle lane")
        else:
            assert (f.a[:, lane, pos[lane]:] == 0).all() and (f.a[:, lane][:, cols[lane] < 0] == 0).all(), (kind, lane)


@pytest.mark.parametrize("kind,dims_name,mode,sparsity", CASES, ids=CASE_IDS)
def test_transposes_alias_and_never_read_entries(kind, dims_name, mode, sparsity):
    """Assertions 2 (lt = a^T within each block, the four arrow rows agree on the trunk, alias = no alias) and 3 (NaN in the strict
    upper triangle, in every entry outside the layout's blocks and in the rows' padding words changes no bit of the output)."""
    d = DH.dims(dims_name)
    H, b, diag = _synthetic(dims_name, sparsity)
    clean = DH.factor(kind, dims_name, mode, H, diag=diag, b=b, alias=0)
    _raw_structure(kind, d, clean)
    live = slice(0, d.NV) if kind == "natural" else slice(0, 64)    # natural order: lanes >= NV hold a copy of row 0 nobody reads
    if kind == "arrow":
        for row in range(1, 4):
            t0, tr = slice(d.ALEGN, d.ALEGN + d.ANT), slice(16 * row + d.ALEGN, 16 * row + d.ALEGN + d.ANT)
            assert _same_bits(clean.a[:, t0, d.ALEGN:], clean.a[:, tr, d.ALEGN:]) and _same_bits(clean.lt[:, t0, d.ALEGN:], clean.lt[:, tr, d.ALEGN:])
            assert _same_bits(clean.dinv[:, t0], clean.dinv[:, tr]), row
    aliased = DH.factor(kind, dims_name, mode, H, diag=diag, b=b, alias=1)
    for name, u, v in zip(clean._fields, clean, aliased):
        assert _same_bits(u[:, live], v[:, live]), (name, "alias")
    i, j = np.meshgrid(np.arange(d.NV), np.arange(d.NV), indexing="ij")
    never = (j > i) | ~in_block(kind, d)
    Hn = np.array(H)
    Hn[:, never] = np.nan
    pad = np.full((len(H), d.NV), np.nan, dtype=np.float32)
    for alias in (0, 1):
        poisoned = DH.factor(kind, dims_name, mode, Hn, diag=diag, b=b, alias=alias, pad=pad)
        for name, u, v in zip(clean._fields, clean, poisoned):
            assert np.isfinite(v[:, live]).all(), (name, alias, "NaN reached the output")
            assert _same_bits(u[:, live], v[:, live]), (name, alias, "never-read entries")


@pytest.mark.parametrize("dims_name", AIRBOT + GO2)
def test_device_lane_maps_equal_the_restatement(dims_name):
    d = DH.dims(dims_name)
    for kind in ["natural"] + (["rowchol"] if d.ROWCHOL else []) + (["rowtree"] if d.ROWTREE else []) + (["arrow"] if d.ARROW else []):
        dof_dev, lane_dev = DH.lane_map(kind, dims_name)
        dof, _, _ = lane_table(kind, d)
        assert (dof_dev == dof).all(), (kind, dof_dev)
        assert (lane_dev == [o[0] for o in lanes_of_dof(kind, d)]).all(), (kind, lane_dev)


@pytest.mark.parametrize("kind,dims_name", sorted({(c[0], c[1]) for c in CASES}))
def test_pivot_floor(kind, dims_name):
    """A zero row and column, and a trailing pivot that comes out slightly negative: that dof's dinv is 1 / RSR_MINVAL (within the
    reciprocal's ulp), everything stays finite, and the other dofs' factors follow the fp64 factorisation with the same floor as
    closely as the accuracy rule asks: at most 4 x the numpy-float32 reference's distance, floor NV * 2^-24 of the largest entry."""
    d = DH.dims(dims_name)
    sparsity = {"natural": SPARSITY_OF_DIMS[dims_name][-1], "rowchol": "coupled", "rowtree": "trees", "arrow": "arrow"}[kind]
    H0, b, _ = _synthetic(dims_name, sparsity)
    cond = np.linalg.cond(H0.astype(np.float64))
    sel = np.argsort(cond)[:32]                                     # the best conditioned: the floor is the subject here
    H0, b = np.array(H0[sel], dtype=np.float64), np.array(b[sel])
    order = elimination_order(kind, d)
    last, zero = order[-1], order[len(order) // 2]
    Hz = H0.copy()
    Hz[:, zero, :] = 0.0
    Hz[:, :, zero] = 0.0
    Hneg = H0.copy()                                                # last pivot = Schur complement of `last` = 1 / inv(H)[last, last]
    schur = 1.0 / np.linalg.inv(H0)[:, last, last]
    Hneg[:, last, last] -= schur * (1.0 + 1e-2)
    one_ulp = np.spacing(np.float32(1.0) / MINVAL)
    for what, Hc, t in (("zero row and column", Hz, zero), ("negative trailing pivot", Hneg, last)):
        Hc = Hc.astype(np.float32)
        L64, _, raw64 = ldlt(Hc.astype(np.float64), np.float64, order)
        L32, D32, raw32 = ldlt(Hc, np.float32, order)
        assert (raw64[:, t] <= 0).all() and (raw32[:, t] <= 0).all() and (np.delete(raw32, t, 1) > 0).all(), what
        f = DH.factor(kind, dims_name, 0, Hc, b=b)
        L, dinv, x = decode(kind, d, f)
        live = slice(0, d.NV) if kind == "natural" else slice(0, 64)
        assert all(np.isfinite(v[:, live]).all() for v in f), what
        err = np.abs(dinv[:, t].astype(np.float64) - 1.0 / np.float64(MINVAL)).max()
        print("FLOOR %s %s %s: dinv %.9e, 1/MINVAL %.9e" % (kind, dims_name, what, dinv[0, t], 1.0 / np.float64(MINVAL)))
        assert err <= one_ulp, (what, dinv[:, t])
        scale = np.abs(L64).max()
        e_ref, e_k = np.abs(L32 - L64).max(), np.abs(L.astype(np.float64) - L64).max()
        print("FLOOR %s %s %s: factor distance kernel %.3e ref %.3e scale %.3e" % (kind, dims_name, what, e_k, e_ref, scale))
        assert e_k <= max(4.0 * e_ref, d.NV * U32 * scale), (what, e_k, e_ref)
        keep = np.arange(d.NV) != t
        np.testing.assert_array_equal(dinv[:, keep] > 0, True)
        e_ref = np.abs(1.0 / D32[:, keep].astype(np.float64) * raw64[:, keep] - 1.0).max()
        e_k = np.abs(dinv[:, keep].astype(np.float64) * raw64[:, keep] - 1.0).max()
        assert e_k <= max(4.0 * e_ref, d.NV * U32), (what, "dinv", e_k, e_ref)


def _sum_inputs():
    rng = np.random.default_rng(11)
    v = [rng.normal(size=(64, 64)), 10.0 ** rng.uniform(-6, 6, size=(32, 64)) * rng.choice([-1, 1], size=(32, 64))]
    c = np.zeros((32, 64))                                          # heavy cancellation: +-1e6 pairs plus 1e-3 terms
    for r in range(32):
        p = rng.permutation(64)
        c[r, p[:16]], c[r, p[16:32]] = 1e6, -1e6
        c[r, p[32:]] = 1e-3 * rng.uniform(0.5, 1.5, 32)
    v.append(c)
    one = np.zeros((12, 64))                                        # one non-zero lane
    for r, lane in enumerate((0, 15, 16, 31, 32, 63)):
        one[r, lane], one[6 + r, lane] = 1.2345678, -3.0e-7
    v.append(one)
    v.append(np.repeat(np.array([[0.1], [1.0], [-7.3], [3.0e20], [1.0e-30]]), 64, axis=1))      # all-equal values
    v.append(np.arange(64, dtype=np.float64)[None] + 1.0)
    return np.concatenate(v).astype(np.float32)


def test_wave_sums():
    """wave_sum: every lane the same bits; wave_sum3 = three wave_sums, bit for bit, fed one vector three times and three
    different vectors; row_sum16 uniform within a row; all against the fp64 sum within gamma_6 sum|v| (six levels of pairwise
    addition; row_sum16: four levels, gamma_4)."""
    v = _sum_inputs()
    n = len(v)
    same = DH.sums(v)
    rng = np.random.default_rng(12)
    three = np.stack([v, v[rng.permutation(n)], v[rng.permutation(n)]], axis=1)
    diff = DH.sums(three)
    for s, vin in ((same, np.repeat(v[:, None], 3, axis=1)), (diff, three)):
        assert np.isfinite(s.wave_sum).all()
        assert (_bits(s.wave_sum) == _bits(s.wave_sum)[:, :, :1]).all(), "wave_sum differs between lanes"
        assert _same_bits(s.wave_sum3, s.wave_sum), "wave_sum3 != wave_sum"
        rows = _bits(s.row_sum16).reshape(n, 3, 4, 16)
        assert (rows == rows[..., :1]).all(), "row_sum16 differs within a row"
        v64 = vin.astype(np.float64)
        g6, g4 = 6 * U32 / (1 - 6 * U32), 4 * U32 / (1 - 4 * U32)
        err = np.abs(s.wave_sum[:, :, 0].astype(np.float64) - v64.sum(2))
        assert (err <= g6 * np.abs(v64).sum(2)).all(), (err / np.abs(v64).sum(2)).max()
        v16 = v64.reshape(n, 3, 4, 16)
        err = np.abs(s.row_sum16.reshape(n, 3, 4, 16)[..., 0].astype(np.float64) - v16.sum(3))
        assert (err <= g4 * np.abs(v16).sum(3)).all()
    assert _same_bits(same.wave_sum[:, 0], same.wave_sum[:, 1]) and _same_bits(same.wave_sum[:, 0], same.wave_sum[:, 2])
    assert _same_bits(same.wave_sum3[:, 0], same.wave_sum3[:, 1]) and _same_bits(same.wave_sum3[:, 0], same.wave_sum3[:, 2])
    # a single non-zero lane and exact small integers come back exactly
    one = slice(64 + 32 + 32, 64 + 32 + 32 + 12)
    assert _same_bits(same.wave_sum[one, 0, 0], v[one].sum(1, dtype=np.float64).astype(np.float32))
    assert same.wave_sum[-1, 0, 0] == 64 * 65 / 2


def _ulps(got, exact):
    """Distance in fp32 ulps between `got` and the correctly rounded value of `exact` (fp64).  Values below the normal range count
    as zero on both sides, as the header of frcp / frsq / fsqrt states (the hardware approximations flush them)."""
    tiny = np.finfo(np.float32).tiny
    flush = lambda f: np.where(np.abs(f) < tiny, np.float32(0), f).astype(np.float32)
    want = flush(exact.astype(np.float32))

    def key(f):                                                     # monotone integer image of the floats
        i = f.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(flush(np.ascontiguousarray(got, dtype=np.float32))) - key(want))
    return np.where(np.isfinite(got), d, np.iinfo(np.int64).max)


def _recip_arguments():
    p = 2.0 ** np.arange(-126, 127)
    p32 = p.astype(np.float32)
    pw = np.concatenate([p32, np.nextafter(p32, np.float32(0)), np.nextafter(p32, np.float32(np.inf))])
    rng = np.random.default_rng(13)
    logu = (2.0 ** rng.uniform(-126, 126, size=100000)).astype(np.float32)
    return pw, logu


def test_reciprocals_in_ulps():
    """frcp <= 1, fsqrt <= 1, frsq <= 2 ulp of the correctly rounded fp64 result.  frcp / frsq: every power of two in
    [2^-126, 2^126] with both neighbours and 1e5 log-uniform values per sign (frsq: the positive ones); frsq / fsqrt: positive normal
    floats.  Valid arguments are the header's: finite, non-zero, "values below the normal range count as zero" -- so the one
    subnormal among the neighbours (just below 2^-126, either sign) is no argument of frcp: what it returns is printed, not bounded
    (measured: NaN), and a reciprocal below the normal range (the neighbour above 2^126) is expected as zero (measured: zero)."""
    pw, logu = _recip_arguments()
    tiny = np.finfo(np.float32).tiny
    x_all = np.concatenate([pw, -pw, logu, -logu])
    valid = np.abs(x_all) >= tiny
    assert (~valid).sum() == 2                                      # +- the largest subnormal
    x_pos = np.concatenate([pw[pw >= tiny], logu, np.array([tiny, np.finfo(np.float32).max, 1.0, 2.0, 3.0, 4.0], dtype=np.float32)])
    rcp_all, _, _ = DH.recips(x_all)
    _, rsq, sq = DH.recips(x_pos)
    print("RECIPS frcp of the subnormal neighbours (not arguments):", [(float(a).hex(), float(r)) for a, r in zip(x_all[~valid], rcp_all[~valid])])
    x_rcp, rcp = x_all[valid], rcp_all[valid]
    u_rcp = _ulps(rcp, 1.0 / x_rcp.astype(np.float64))
    u_rsq = _ulps(rsq, 1.0 / np.sqrt(x_pos.astype(np.float64)))
    u_sq = _ulps(sq, np.sqrt(x_pos.astype(np.float64)))
    under = np.abs(1.0 / x_rcp.astype(np.float64)) < tiny
    print("RECIPS frcp max %d ulp over %d arguments (%d with a reciprocal below the normal range: results %s), frsq max %d ulp, fsqrt max %d ulp"
          % (u_rcp.max(), len(x_rcp), under.sum(), sorted(set(rcp[under].tolist())), u_rsq.max(), u_sq.max()))
    assert u_sq.max() <= 1, (u_sq.max(), x_pos[np.argmax(u_sq)])
    assert u_rsq.max() <= 2, (u_rsq.max(), x_pos[np.argmax(u_rsq)])
    assert u_rcp.max() <= 1, (u_rcp.max(), x_rcp[np.argmax(u_rcp)])
