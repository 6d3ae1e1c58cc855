"""The test-only HIP unit of the L D L^T layouts (tests/device/primitives.hip, tests/device_harness.py) on the CPU: it compiles for
gfx950 and exports its entry points (a signature drift in rsr_device.hpp fails here, without a GPU), and the Python restatement
of the layouts' lane <-> dof maps is consistent with the Dims constants the unit exports.

Also home of what tests/test_device_primitives_gpu.py shares: the restated maps, the decoding of raw lane registers into
natural-order factors, the plain numpy L D L^T that is the accuracy reference, and the input generators."""
import os

import numpy as np
import pytest

import device_harness as DH

ALL_DIMS = list(DH.DIMS)
MINVAL = np.float32(1e-15)             # RSR_MINVAL
U32 = 2.0 ** -24                       # unit roundoff of fp32


# ---------------------------------------------------------------- the layouts, restated from the Dims constants
def tree_ranges(d):
    """Kinematic trees of a Dims: dof ranges [0, TREE1), [TREE1, TREE2), [TREE2, NV)."""
    return [(0, d.TREE1), (d.TREE1, d.TREE2), (d.TREE2, d.NV)]


def lane_table(kind, d):
    """(dof_of_lane[64], cols[64][NREG], pos[64]): the dof whose row a lane holds (-1: idle), the dof of each column register
    (-1: none) and the lane's position in its 16-lane row's local matrix."""
    nreg = d.NV if kind == "natural" else d.NCH
    dof = np.full(64, -1, dtype=np.int64)
    cols = np.full((64, nreg), -1, dtype=np.int64)
    pos = np.arange(64) % 16
    if kind == "natural":
        pos = np.arange(64)
        for lane in range(d.NV):
            dof[lane] = lane
            cols[lane] = np.arange(d.NV)
    elif kind == "rowchol":
        niso = d.ISO1 - d.ISO0
        na = d.NV - niso
        col_a = [c if c < d.ISO0 else c + niso for c in range(na)]           # block A: the dofs outside [ISO0, ISO1), in order
        for r in range(na):
            dof[r] = col_a[r]
            cols[r, :na] = col_a
        for r in range(niso):                                                # block B: the isolated dofs, lanes 16..
            dof[16 + r] = d.ISO0 + r
            cols[16 + r, :niso] = d.ISO0 + np.arange(niso)
    elif kind == "rowtree":
        for t, (lo, hi) in enumerate(tree_ranges(d)):
            for p in range(hi - lo):
                dof[16 * t + p] = lo + p
                cols[16 * t + p, :hi - lo] = lo + np.arange(hi - lo)
    elif kind == "arrow":
        for row in range(d.ALEGS):
            leg = d.ANT + d.ALEGN * row + np.arange(d.ALEGN)
            for p in range(d.ALEGN + d.ANT):
                lane = 16 * row + p
                dof[lane] = leg[p] if p < d.ALEGN else p - d.ALEGN
                cols[lane, :d.ALEGN] = leg
                cols[lane, d.ALEGN:d.ALEGN + d.ANT] = np.arange(d.ANT)
    else:
        raise KeyError(kind)
    return dof, cols, pos


def lanes_of_dof(kind, d):
    """dof -> the lanes that hold its row (one, or four for an arrow trunk dof), in lane order."""
    dof, _, _ = lane_table(kind, d)
    return [np.nonzero(dof == i)[0] for i in range(d.NV)]


def in_block(kind, d, mass_only=False):
    """[NV, NV] bool: entries a layout works on; the rest are structural zeros it never loads.  (The natural order loads every
    entry of the lower triangle: its template arguments only fold updates.)"""
    i, j = np.meshgrid(np.arange(d.NV), np.arange(d.NV), indexing="ij")
    iso = lambda k: (k >= d.ISO0) & (k < d.ISO1)
    if kind == "natural":
        return np.ones((d.NV, d.NV), dtype=bool)
    if kind == "rowchol":
        return iso(i) == iso(j)
    if kind == "rowtree":
        tree = lambda k: (k >= d.TREE1).astype(int) + (k >= d.TREE2).astype(int)
        return tree(i) == tree(j)
    leg = lambda k: np.where(k < d.ANT, -1, (k - d.ANT) // d.ALEGN)
    return (leg(i) < 0) | (leg(j) < 0) | (leg(i) == leg(j))


def elimination_order(kind, d):
    """dofs in the order a layout eliminates them within its blocks (arrow: legs first, then the trunk)."""
    if kind == "arrow":
        return list(range(d.ANT, d.NV)) + list(range(d.ANT))
    return list(range(d.NV))


def decode(kind, d, f):
    """Raw registers -> (L[n, NV, NV] float32 with L[i, j] = the factor entry of dofs (i, j), unit diagonal; dinv[n, NV];
    x[n, NV]).  Registers are copied, never recomputed: bit patterns survive.  A trunk dof of the arrow layout is read from
    its copy in row 0 (its leg columns from the row of that leg)."""
    dof, cols, _ = lane_table(kind, d)
    n = f.a.shape[0]
    L = np.zeros((n, d.NV, d.NV), dtype=np.float32)
    dinv = np.zeros((n, d.NV), dtype=np.float32)
    for lane in range(63, -1, -1):                     # descending: the lowest lane of a dof (row 0) is written last
        i = dof[lane]
        if i < 0:
            continue
        for c, j in enumerate(cols[lane]):
            if j >= 0 and j != i:
                if kind == "arrow" and i < d.ANT and j < d.ANT and lane >= 16:
                    continue
                L[:, i, j] = f.a[:, lane, c]
        dinv[:, i] = f.dinv[:, lane]
    L[:, np.arange(d.NV), np.arange(d.NV)] = 1.0
    return L, dinv, f.x[:, :d.NV]


# ---------------------------------------------------------------- plain numpy L D L^T: the accuracy reference
def ldlt(H, dtype=np.float32, order=None):
    """Natural-order (or `order`) square-root-free Cholesky, one rounding per operation in `dtype`: exact division, separate
    multiply and subtract, the kernels' pivot floor.  Returns (L unit lower in dof indices, D, raw pivots before the floor)."""
    n, nv, _ = H.shape
    order = list(range(nv)) if order is None else list(order)
    A = np.ascontiguousarray(H[:, order][:, :, order], dtype=dtype).copy()
    L = np.zeros_like(A)
    D = np.zeros((n, nv), dtype=dtype)
    raw = np.zeros((n, nv), dtype=dtype)
    for k in range(nv):
        raw[:, k] = A[:, k, k]
        piv = np.where(raw[:, k] > 0, raw[:, k], dtype(MINVAL)).astype(dtype)
        D[:, k] = piv
        u = A[:, k + 1:, k].copy()
        l = (u / piv[:, None]).astype(dtype)
        L[:, k + 1:, k] = l
        prod = (l[:, :, None] * u[:, None, :]).astype(dtype)
        A[:, k + 1:, k + 1:] = (A[:, k + 1:, k + 1:] - prod).astype(dtype)
    L[:, np.arange(nv), np.arange(nv)] = 1
    inv = np.argsort(order)
    return L[:, inv][:, :, inv], D[:, inv], raw[:, inv]


def ldlt_solve(L, D, b, order=None):
    """x of L D L^T x = b by the kernels' substitutions (column sweeps), in the dtype of L."""
    dtype = L.dtype.type
    n, nv, _ = L.shape
    order = list(range(nv)) if order is None else list(order)
    Lp = L[:, order][:, :, order]
    x = np.ascontiguousarray(b[:, order], dtype=dtype).copy()
    for k in range(nv):
        x[:, k + 1:] = (x[:, k + 1:] - (Lp[:, k + 1:, k] * x[:, k:k + 1]).astype(dtype)).astype(dtype)
    x = (x / D[:, order]).astype(dtype)
    for k in range(nv - 1, -1, -1):
        x[:, :k] = (x[:, :k] - (Lp[:, k, :k] * x[:, k:k + 1]).astype(dtype)).astype(dtype)
    return x[:, np.argsort(order)]


def backward_error(H, x, b):
    """eta = |b - H x|_inf / (|H|_inf |x|_inf + |b|_inf) per problem, in fp64."""
    H, x, b = (np.asarray(v, dtype=np.float64) for v in (H, x, b))
    r = np.abs(b - np.einsum("nij,nj->ni", H, x)).max(1)
    return r / (np.abs(H).sum(2).max(1) * np.abs(x).max(1) + np.abs(b).max(1))


def rebuild_error(H, L, D):
    """|H - L D L^T|_inf / |H|_inf per problem, in fp64."""
    H, L, D = (np.asarray(v, dtype=np.float64) for v in (H, L, D))
    R = np.einsum("nik,nk,njk->nij", L, D, L)
    return np.abs(H - R).sum(2).max(1) / np.abs(H).sum(2).max(1)


# ---------------------------------------------------------------- inputs
def synthetic_spd(dims_name, sparsity, n=256, seed=0):
    """H = S (I + J^T D J) S rounded to fp32, with J's rows inside the sparsity a layout assumes:
         "coupled": block diagonal over {dofs outside [ISO0, ISO1)} and {the isolated dofs}   (Hessian of the Airbot models)
         "trees":   block diagonal over the kinematic trees                                   (mass matrix; Hessian, trees apart)
         "arrow":   every row touches the trunk and at most one leg                           (Go2)
    S = diag, log-uniform, so that condition numbers span 1e1 .. 1e5.  Kept: the first n candidates whose pivots are all
    positive in the fp32 reference ldlt().  Returns (H[n] float32, b[n] float32, diag[n] float32, dropped fraction, cond[n])."""
    d = DH.dims(dims_name)
    nv = d.NV
    rng = np.random.default_rng([seed, DH.DIMS[dims_name], {"coupled": 0, "trees": 1, "arrow": 2}[sparsity]])
    m = n + n // 8
    rows = 3 * nv
    if sparsity == "arrow":
        legs = rng.integers(-1, d.ALEGS, size=(m, rows))
        k = np.arange(nv)
        leg_of = np.where(k < d.ANT, -1, (k - d.ANT) // d.ALEGN)
        mask = (leg_of[None, None, :] < 0) | (leg_of[None, None, :] == legs[:, :, None])
    else:
        if sparsity == "coupled":
            iso = (np.arange(nv) >= d.ISO0) & (np.arange(nv) < d.ISO1)
            group = iso.astype(int)
        else:
            group = (np.arange(nv) >= d.TREE1).astype(int) + (np.arange(nv) >= d.TREE2).astype(int) if d.TREE1 > 0 else np.zeros(nv, int)
        present = np.unique(group)
        pick = present[rng.integers(0, len(present), size=(m, rows))]
        mask = group[None, None, :] == pick[:, :, None]
    J = rng.normal(size=(m, rows, nv)) * mask
    Dw = 10.0 ** rng.uniform(-2, 0, size=(m, rows))
    core = np.eye(nv)[None] + np.einsum("nri,nr,nrj->nij", J, Dw, J)
    spread = rng.uniform(0.0, 4.0, size=(m, 1))                       # decades between the smallest and the largest scale
    S = 10.0 ** (spread * rng.uniform(-0.5, 0.5, size=(m, nv)) / 2)
    H = (S[:, :, None] * core * S[:, None, :]).astype(np.float32)
    H = np.maximum(H, H.transpose(0, 2, 1))                          # symmetric bit for bit
    _, _, raw = ldlt(H)
    ok = (raw > 0).all(1)
    keep = np.nonzero(ok)[0][:n]
    examined = keep[-1] + 1 if len(keep) == n else m
    dropped = 1.0 - len(keep) / examined
    H = H[keep]
    xt = rng.normal(size=(m, nv))[keep]
    b = np.einsum("nij,nj->ni", H.astype(np.float64), xt).astype(np.float32)
    diag = (np.diagonal(H, axis1=1, axis2=2) * 10.0 ** rng.uniform(-3, -1, size=(m, nv))[keep]).astype(np.float32)
    cond = np.linalg.cond(H.astype(np.float64))
    return H, b, diag, dropped, cond


SPARSITY_OF_DIMS = {"CubeDims": ("coupled", "trees"), "TShapeDims": ("coupled", "trees"),
                    "Go2FlatDims": ("arrow",), "Go2Dims": ("arrow",), "HandDims": ("arrow",)}


# ---------------------------------------------------------------- CPU tests
def test_unit_compiles_and_exports_every_entry_point():
    path = DH.build()
    assert os.path.exists(path) and os.path.dirname(path) == DH.BUILD_DIR
    L = DH.lib()
    for sym in DH.SYMBOLS:
        getattr(L, sym)
    assert L.rsr_prim_dims(len(DH.DIMS), None) == -1 and not DH.supported("arrow", "CubeDims", 0)


def test_dims_constants_of_the_shipped_families():
    nv = {"CubeDims": 20, "TShapeDims": 14, "Go2FlatDims": 18, "Go2Dims": 18, "HandDims": 18}
    for name in ALL_DIMS:
        d = DH.dims(name)
        assert d.NV == nv[name] and d.LD == d.NV + 1 and d.NISO == d.ISO1 - d.ISO0 and d.NA == d.NV - d.NISO
        assert d.NCH == (d.NA if d.ROWCHOL else 9 if d.ARROW else d.NV)
        assert d.ROWCHOL + d.ARROW == 1, "every shipped family has a blocked layout"
        if d.ROWTREE:
            assert d.NCT == max(hi - lo for lo, hi in tree_ranges(d)) and 0 < d.TREE1 <= d.TREE2 <= d.NV
        if d.ARROW:
            assert (d.ANT, d.ALEGN, d.ALEGS) == (6, 3, 4) and d.NV == d.ANT + d.ALEGN * d.ALEGS
    # the combinations rsr_solver.hpp instantiates (hessian_factor, forward, integrate), and nothing else
    MO, HD = DH.MASS_ONLY, DH.HAS_DIAG
    want = {"natural": {0, MO, HD, MO | HD}, "rowchol": {0, MO, MO | HD}, "rowtree": {0, HD}, "arrow": {0, HD}}
    for name in ALL_DIMS:
        d = DH.dims(name)
        has = {"natural": True, "rowchol": d.ROWCHOL, "rowtree": d.ROWTREE, "arrow": d.ARROW}
        for kind in DH.KINDS:
            got = {m for m in range(4) if DH.supported(kind, name, m)}
            assert got == (want[kind] if has[kind] else set()), (name, kind, got)


@pytest.mark.parametrize("name", ALL_DIMS)
def test_lane_maps_restated_from_the_constants(name):
    d = DH.dims(name)
    kinds = ["natural"] + (["rowchol"] if d.ROWCHOL else []) + (["rowtree"] if d.ROWTREE else []) + (["arrow"] if d.ARROW else [])
    for kind in kinds:
        dof, cols, pos = lane_table(kind, d)
        owners = lanes_of_dof(kind, d)
        for i in range(d.NV):                              # every dof has exactly one owning lane; an arrow trunk dof one per row
            want = 4 if (kind == "arrow" and i < d.ANT) else 1
            assert len(owners[i]) == want, (kind, i, owners[i])
            if want == 4:
                assert (owners[i] // 16).tolist() == [0, 1, 2, 3] and len(set(owners[i] % 16)) == 1
        active = sum(len(o) for o in owners)
        assert (dof >= 0).sum() == active and (dof[dof < 0] == -1).all() and (dof < 0).sum() == 64 - active      # idle lanes: -1
        for lane in np.nonzero(dof >= 0)[0]:
            # a lane's own dof sits at its position among its columns (the diagonal), columns are distinct, all in its block
            assert cols[lane, pos[lane]] == dof[lane], (kind, lane)
            c = cols[lane][cols[lane] >= 0]
            assert len(set(c)) == len(c) and in_block(kind, d)[dof[lane], c].all()
            if kind != "natural":                          # one block per 16-lane row: same columns along the row
                first = 16 * (lane // 16)
                assert (cols[lane] == cols[first]).all()
        assert (cols[dof < 0] == -1).all()
        # every in-block entry of the lower triangle (in elimination order) is held by some lane
        rank = np.argsort(elimination_order(kind, d))
        held = np.zeros((d.NV, d.NV), dtype=bool)
        for lane in np.nonzero(dof >= 0)[0]:
            for c, j in enumerate(cols[lane]):
                if j >= 0 and c <= pos[lane]:
                    held[dof[lane], j] = True
                    assert rank[j] <= rank[dof[lane]], (kind, lane, c)
        i, j = np.meshgrid(np.arange(d.NV), np.arange(d.NV), indexing="ij")
        assert (held == (in_block(kind, d) & (rank[j] <= rank[i]))).all(), kind


@pytest.mark.parametrize("name", ALL_DIMS)
def test_synthetic_inputs_keep_their_pivots_and_span_the_conditioning(name):
    d = DH.dims(name)
    for sparsity in SPARSITY_OF_DIMS[name]:
        H, b, diag, dropped, cond = synthetic_spd(name, sparsity)
        assert H.shape == (256, d.NV, d.NV) and dropped <= 0.05, (sparsity, dropped)
        assert (H == H.transpose(0, 2, 1)).all() and np.isfinite(H).all() and (diag > 0).all()
        kind = {"coupled": "rowchol", "trees": "rowtree", "arrow": "arrow"}[sparsity]
        assert (H[:, ~in_block(kind, d)] == 0).all(), sparsity
        assert cond.min() < 1e2 and cond.max() > 1e4 and cond.max() < 1e6, (sparsity, cond.min(), cond.max())
        # the reference solves them: backward error within Higham's gamma_(3n+1) of a Cholesky solve
        L, D, _ = ldlt(H)
        eta = backward_error(H, ldlt_solve(L, D, b), b)
        assert eta.max() < (3 * d.NV + 1) * U32, (sparsity, eta.max())
