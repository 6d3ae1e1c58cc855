"""Plain fp64 statement of what the Newton solver's leaf functions (rsr_mjx_amd/csrc/rsr_solver.hpp: rows_cost, ls_prepare /
ls_point / ls_eval / ls_costs, jdot, jt_force) compute, the error bounds the device tests hold them to, and the seeded inputs.
numpy only; `d` is device_harness.sr_dims(name).  Per-lane arrays are [n, NCHUNK, 64] with row = lane + 64 * chunk, so
a.reshape(n, NCHUNK * 64) is indexed by row.

Rows.  Row r of a wave with nefc rows is an equality row for r < NEQ, a friction-loss row for r < NEQ + NF and a unilateral row
(limit, pyramid edge) for r < nefc, in the compact layout r_lim = NEQ + NF, r_con = r_lim + nl, nefc = r_con + NPYR ncon.  Its
cost at x is  equality: D x^2 / 2;  friction, rf = R floss: floss (-rf / 2 - x) for x <= -rf, floss (-rf / 2 + x) for x >= rf,
else D x^2 / 2;  unilateral: D x^2 / 2 for x < 0, else 0.  force = -dc/dx, weight = d2c/dx2.  (The friction row's pieces meet at
+-rf only where D R = 1, which make_constraint keeps; the functions take D and R as given and so does this reference.)  The 1-D model is
phi(a) = sum_r c_r(ja_r + a v_r) + g0 + a g1 + a^2 g2, evaluated as written; phi' and phi'' are the derivatives of that form.
Rows >= nefc are make_constraint's padding {D 0, R 1, floss -1, mu 0, bn = bk = NBASE} with jaref = jv = 0 and add nothing.

Bounds.  u = 2^-24.  A value the kernel forms as a sum of terms t_k, each rounded r_k times on its way and then added through at
most `depth` fp32 additions, differs from the exact sum by at most sum_k ((1 + u)^(r_k + depth) - 1) |t_k|, to first order
(r_k + depth) u |t_k|.  The bound used is  sum_k (r_k + depth + 2) u |t_k|  =  c u S:  two more roundings than counted (the fp64
reference's own error and the second-order terms, both below 1e-6 of the bound, are inside them).  |t_k| is the magnitude of the
term as the kernel forms it: for c0m = floss (-rf / 2 - ja) that is floss (rf / 2 + |ja|), whose roundings act on rf / 2 and |ja|
separately.  Fused multiply-adds only remove roundings, so one bound holds with and without contraction.
  depth of the row sums: NCHUNK - 1 serial adds of the lane's chunks (the first lands on a zero), six levels of wave_sum, and for
  the line search the add of g: DEPTH_ROWS = NCHUNK + 5, DEPTH_LS = NCHUNK + 6.
  roundings per term, r_k (products by 0.5, 2 and -1 are exact):
    rows_cost   D x^2 / 2: 2 (two products)                    floss (-rf / 2 -+ x): 3 (rf, the sum, the product)
    q1, q2      b1 = v ja D: 2;  b2 = v v D / 2: 2;  c1m = -floss v, c1p: 1;  g1, g2: 0 (their add is in the depth)
    d0()        = 2 a q2 + q1: the terms of q2 gain 2 (product, add), those of q1 gain 1
    2 q2        against phi'': nothing gained
    cost        = a a q2 + a q1 + (q0 + g0): the terms of q2 gain 4 (a a, its product with q2, two adds), those of q1 gain 3,
                those of q0 gain 1;  b0 = ja ja D / 2: 2;  c0m, c0p: 3
  jdot: a base row's product with v is NV / 2 fused multiply-adds per half (each term passes at most NV / 2 roundings) and the
  add of the halves: depth NV / 2 + 1; out = bval[bn] + mu bval[bk] gives the terms of row bn 1 more rounding and those of row
  bk 2 more.  S = sum_i (|B[bn, i]| + |mu| |B[bk, i]|) |v_i|.
  jt_force, per dof i: S_i = sum_r (|B[bn_r, i]| + |mu_r| |B[bk_r, i]|) |f_r|, which is also the sum of the magnitudes of the folded
  terms the kernel forms (normal: B[n, i] sum_e f_e; direction k: B[k, i] mu_k (f_k+ - f_k-)).  Roundings per term: the fold onto
  the base row (normal: one pair add and NPYR / 2 - 1 serial adds; direction: the difference and the product by mu: at most
  NPYR / 2 and at least 2, so max(NPYR / 2, 2)), the product with J (1).  Depth: a quartet walk of T trips adds 2 T times into each
  accumulator; one group (NBC NCON <= 16): T = ceil(NBC NCON / 4), the accumulators start from dgw and from the NEQ equality adds,
  and meet in one add: 2 T + NEQ + 1.  Several groups (G = 64 / NV): T = ceil(ceil(NBC NCON / 4) / G), the add of the
  accumulators, then dgw + NEQ equality terms + G partial sums: 2 T + 1 + NEQ + G.  A friction or limit row's term is one product
  and at most one add in dgw (two rows per dof) before it enters that chain: no more than a contact term.

Thresholds.  The bounds compare sums over the SAME pieces, so every random row keeps x(a) = ja + a v further from each of its
thresholds (+-rf, 0) than 8 u (|ja| + |a v|) at all three step sizes: the kernel's x has at most two roundings (1 with an fma)
and its rf one, each below u (|ja| + |a v|) when x is near +-rf.  The generators redraw ja of rows inside the margin
(threshold_violations is the census the CPU test asserts empty).  What happens AT a threshold is tested exactly, on dyadic
inputs (threshold_cases)."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
MINVAL = np.float32(1e-15)
EQ, FRIC, UNI, PAD = 0, 1, 2, 3                       # row kinds
QUAD, LOWER, UPPER, OFF = 0, 1, 2, 3                  # pieces: quadratic, lower / upper linear (friction), zero (unilateral, x >= 0)
NWAVE = 256
MARGIN = 8.0


def f64(a):
    """the fp32 values the kernel is given, as fp64"""
    return np.asarray(a, np.float32).astype(np.float64)


def by_row(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1)


def row_kinds(d, nefc):
    """[n, NCHUNK * 64]: EQ, FRIC, UNI by row index, PAD from nefc on"""
    r = np.arange(d.NCHUNK * 64)[None, :]
    k = np.where(r < d.NEQ, EQ, np.where(r < d.NEQ + d.NF, FRIC, UNI))
    return np.where(r < np.asarray(nefc)[:, None], k, PAD)


def pieces(kind, x, rf):
    p = np.full(x.shape, QUAD)
    p = np.where((kind == FRIC) & (x <= -rf), LOWER, p)
    p = np.where((kind == FRIC) & (x >= rf), UPPER, p)
    p = np.where((kind == UNI) & ~(x < 0), OFF, p)
    return np.where(kind == PAD, OFF, p)


def row_cost(kind, x, D, R, floss):
    """(cost, force, weight, piece) of rows at x, elementwise in fp64; padding rows: all zero"""
    rf = R * floss
    p = pieces(kind, x, rf)
    quad, lo, up = p == QUAD, p == LOWER, p == UPPER
    c = np.where(quad, 0.5 * D * x * x, np.where(lo, floss * (-0.5 * rf - x), np.where(up, floss * (-0.5 * rf + x), 0.0)))
    f = np.where(quad, -D * x, np.where(lo, floss, np.where(up, -floss, 0.0)))
    w = np.where(quad, D, 0.0)
    return c, f, w, p


def _rows(d, case):
    kind = row_kinds(d, case["nefc"])
    ja, D, R, fl = (by_row(f64(case[k])) for k in ("jaref", "D", "R", "floss"))
    return kind, ja, D, R, fl


def rows_cost_ref(d, case):
    """rows_cost at x = jaref: cost[n], force, hw, piece [n, rows], the magnitude sum S[n] and the bound[n] of the cost"""
    kind, ja, D, R, fl = _rows(d, case)
    c, f, w, p = row_cost(kind, ja, D, R, fl)
    lin = (p == LOWER) | (p == UPPER)
    mag = np.where(p == QUAD, 0.5 * D * ja * ja, np.where(lin, fl * (0.5 * R * fl + np.abs(ja)), 0.0))
    depth = d.NCHUNK + 5
    rk = np.where(lin, 3, 2)
    lanes = lambda a: a.reshape(len(a), d.NCHUNK, 64).sum(1)              # a lane's share: its rows, before the wave_sum
    return dict(cost=c.sum(1), force=f, hw=w, piece=p, S=mag.sum(1), bound=U * ((rk + depth + 2) * mag).sum(1),
                lane=lanes(c), lane_bound=U * lanes((rk + d.NCHUNK - 1 + 2) * mag))


def model_ref(d, case, alpha=None):
    """the 1-D model at alpha[n, 3] (the case's, or fp64 ones given): phi, dphi, ddphi [n, 3], their bounds b_cost, b_d0, b_q2, the
    pieces [n, 3, rows] and nquad [n, 3] (rows on the quadratic piece whose weight D v^2 is not zero)"""
    kind, ja, D, R, fl = _rows(d, case)
    v = by_row(f64(case["jv"]))
    g, al = f64(case["g"]), f64(case["alpha"]) if alpha is None else np.asarray(alpha, np.float64)
    a = al[:, :, None]
    K, JA, V, DD, RR, FL = (x[:, None, :] for x in (kind, ja, v, D, R, fl))
    x = JA + a * V
    c, f, w, p = row_cost(K, x, DD, RR, FL)
    phi = c.sum(2) + g[:, None, 0] + al * g[:, None, 1] + al * al * g[:, None, 2]
    dphi = (-f * V).sum(2) + g[:, None, 1] + 2 * al * g[:, None, 2]
    ddphi = (w * V * V).sum(2) + 2 * g[:, None, 2]
    # magnitudes of the terms as the kernel forms them
    quad, lin = p == QUAD, (p == LOWER) | (p == UPPER)
    b0, b1, b2 = np.abs(0.5 * JA * JA * DD), np.abs(V * JA * DD), np.abs(0.5 * V * V * DD)
    c0, c1 = FL * (0.5 * RR * FL + np.abs(JA)), np.abs(FL * V)
    depth = d.NCHUNK + 6
    A = np.abs(a)
    ag = np.abs(g)

    def total(rows, gs):
        """sum over the rows of (roundings, magnitude, mask) and over the g terms of (roundings, magnitude)"""
        s = sum((((r + depth + 2) * m) * k).sum(2) for r, m, k in rows)
        return U * (s + sum((r + depth + 2) * m for r, m in gs))

    b_q2 = total([(2, 2 * b2, quad)], [(0, 2 * ag[:, None, 2] + 0 * al)])
    b_d0 = total([(3, b1, quad), (4, 2 * A * b2, quad), (2, c1, lin)], [(1, ag[:, None, 1] + 0 * al), (2, 2 * np.abs(al) * ag[:, None, 2])])
    b_cost = total([(6, A * A * b2, quad), (5, A * b1, quad), (3, b0, quad), (4, A * c1, lin), (4, c0, lin)],
                   [(1, ag[:, None, 0] + 0 * al), (3, np.abs(al) * ag[:, None, 1]), (4, al * al * ag[:, None, 2])])
    nquad = (quad & (DD * V * V != 0)).sum(2)
    return dict(phi=phi, dphi=dphi, ddphi=ddphi, b_cost=b_cost, b_d0=b_d0, b_q2=b_q2, piece=p, nquad=nquad, x=x)


def threshold_violations(d, case, alphas=None):
    """[n, rows] bool: a live row whose x(a) is within MARGIN u (|ja| + |a v|) of one of its thresholds at some step size"""
    kind, ja, D, R, fl = _rows(d, case)
    v = by_row(f64(case["jv"])) if "jv" in case else np.zeros_like(ja)
    al = f64(case["alpha"]) if alphas is None else alphas
    bad = np.zeros(ja.shape, bool)
    rf = R * fl
    for k in range(al.shape[1]):
        a = al[:, k:k + 1]
        x, m = ja + a * v, MARGIN * U * (np.abs(ja) + np.abs(a * v))
        bad |= (kind == UNI) & (np.abs(x) <= m)
        bad |= (kind == FRIC) & ((np.abs(x + rf) <= m) | (np.abs(x - rf) <= m))
    return bad


# ---------------------------------------------------------------- inputs of the row model
def structures(d, seed=0):
    """(nl, ncon) of the NWAVE waves: 64 structures, each four times.  nl in {0, 1, NL} x ncon in {0 .. 5, NCON}; nefc at both ends
    of [NEQ + NF, NEFC], at every multiple of 64 in range and one row either side; random ones up to 64."""
    r_lim = d.NEQ + d.NF

    def of_nefc(t):
        ncon = min(d.NCON, (t - r_lim) // d.NPYR)
        return t - r_lim - d.NPYR * ncon, ncon

    s = [(nl, nc) for nl in (0, 1, d.NL) for nc in sorted({0, 1, 2, 3, 4, 5, d.NCON}) if nc <= d.NCON]
    s += [of_nefc(t) for m in range(64, d.NEFC + 2, 64) for t in (m - 1, m, m + 1) if r_lim <= t <= d.NEFC]
    rng = np.random.default_rng([seed, d.NEFC])
    while len(s) < 64:
        s.append((int(rng.integers(0, d.NL + 1)), int(rng.integers(0, d.NCON + 1))))
    assert len(s) == 64 and all(0 <= nl <= d.NL and 0 <= nc <= d.NCON for nl, nc in s)
    nl, nc = np.array([s[e % 64] for e in range(NWAVE)]).T
    return nl, nc


def model_cases(d, seed=1):
    """The NWAVE waves of the rows_cost and line-search tests (read-only arrays): nl, ncon, nefc [n]; jaref, jv, D, R, floss
    [n, NCHUNK, 64]; g [n, 3]; alpha [n, 3]; flat [n] (waves built to have no quadratic row and g2 = 0); redrawn (rows whose ja was
    redrawn for the threshold margin).
      D = 10^U(-2, 6), 6 % of the live rows D = 0; R = 1 / D; floss of friction row r of wave e: (0, 1e-3 U(.5, 2), 1e3 U(.5, 2))
      [(r + e) % 3]; friction rows with floss > 0 aim, at the wave's first step size, inside / below / above their thresholds
      [(r + e // 3) % 3]; ja, jv = N(0, 1) 10^U(-3, 1).
      step sizes by e // 64: (0, -a, b); (0, b, 1e6); (0, 1e15, b) with jv scaled by 1e-4 (the model stays inside fp32);
      e // 64 == 3: even waves flat with (0, b, 1e15) -- equality rows D = 0, friction rows saturated (all above or all below,
      by e // 2), unilateral rows positive, jv >= 0 (<= 0 on the friction rows saturated below) -- odd waves (-a, 1e6, 1e15) with jv
      scaled by 1e-4."""
    rng = np.random.default_rng([seed, d.NEFC])
    n, nr = NWAVE, d.NCHUNK * 64
    nl, ncon = structures(d)
    nefc = d.NEQ + d.NF + nl + d.NPYR * ncon
    kind = row_kinds(d, nefc)
    live = kind != PAD
    e, r = np.arange(n)[:, None], np.arange(nr)[None, :]
    variant = (e // 64) + 0 * r
    flat = ((variant == 3) & (e % 2 == 0))[:, 0]
    a_, b_ = rng.uniform(0.05, 2.0, n), rng.uniform(0.05, 2.0, n)
    z = np.zeros(n)
    alpha = np.select([variant[:, :1] == 0, variant[:, :1] == 1, variant[:, :1] == 2, flat[:, None]],
                      [np.stack([z, -a_, b_], 1), np.stack([z, b_, z + 1e6], 1), np.stack([z, z + 1e15, b_], 1), np.stack([z, b_, z + 1e15], 1)],
                      np.stack([-a_, z + 1e6, z + 1e15], 1)).astype(np.float32)
    small_v = (variant[:, 0] == 2) | ((variant[:, 0] == 3) & ~flat)
    D = (10.0 ** rng.uniform(-2, 6, (n, nr))).astype(np.float32)
    D[rng.uniform(size=(n, nr)) < 0.06] = 0.0
    D[flat[:, None] & (kind == EQ)] = 0.0
    R = np.where(D > 0, 1.0 / np.where(D > 0, D, 1.0), 10.0 ** rng.uniform(-3, 1, (n, nr))).astype(np.float32)
    fclass = (r + e) % 3
    floss = np.where(kind == FRIC, np.select([fclass == 0, fclass == 1], [0.0, 1e-3], 1e3) * rng.uniform(0.5, 2.0, (n, nr)), -1.0).astype(np.float32)
    jv = (rng.normal(size=(n, nr)) * 10.0 ** rng.uniform(-3, 1, (n, nr)) * np.where(small_v, 1e-4, 1.0)[:, None]).astype(np.float32)
    rf = f64(R) * f64(floss)
    down = (flat & ((np.arange(n) // 2) % 2 == 1))[:, None]                       # flat waves whose friction rows sit below -rf

    def draw():
        ja = rng.normal(size=(n, nr)) * 10.0 ** rng.uniform(-3, 1, (n, nr))
        aim = (r + e // 3) % 3
        t = np.select([aim == 0, aim == 1], [rng.uniform(-0.9, 0.9, (n, nr)), -(1.2 + rng.uniform(0, 3, (n, nr)))], 1.2 + rng.uniform(0, 3, (n, nr)))
        ja = np.where((kind == FRIC) & (floss > 0), t * rf - f64(alpha)[:, :1] * f64(jv), ja)
        up = np.abs(ja) + 1e-3
        ja = np.where(flat[:, None] & (kind == UNI), up, ja)
        ja = np.where(flat[:, None] & (kind == FRIC), np.where(down, -1.0, 1.0) * (1.5 * np.maximum(rf, 0.0) + up), ja)
        return ja.astype(np.float32)

    jv = np.where(flat[:, None], np.where(down & (kind == FRIC), -1.0, 1.0) * np.abs(jv), jv).astype(np.float32)
    jaref = draw()
    pad = lambda a, v: np.where(live, a, np.float32(v)).astype(np.float32)
    jv, D, R, floss = pad(jv, 0), pad(D, 0), pad(R, 1), pad(floss, -1)
    redrawn = np.zeros((n, nr), bool)
    for _ in range(64):
        jaref = pad(jaref, 0)
        c = dict(nefc=nefc, jaref=jaref, jv=jv, D=D, R=R, floss=floss, alpha=alpha)
        bad = threshold_violations(d, c)
        if not bad.any():
            break
        redrawn |= bad
        jaref = np.where(bad, draw(), jaref)
    g = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 3))
    g[:, 2] = np.abs(g[:, 2])
    g[flat] = [0.3, -0.7, 0.0]
    sh = (n, d.NCHUNK, 64)
    c = dict(nl=nl, ncon=ncon, nefc=nefc.astype(np.int32), jaref=jaref.reshape(sh), jv=jv.reshape(sh), D=D.reshape(sh), R=R.reshape(sh),
             floss=floss.reshape(sh), g=g.astype(np.float32), alpha=alpha, flat=flat, redrawn=redrawn)
    for a in c.values():
        a.setflags(write=False)
    return c


def model_census(d, case):
    """{name: count} of what the waves cover: row kind x piece x chunk over the three step sizes and at x = jaref, the floss
    classes by piece, D = 0 inside nefc, the structures"""
    m = model_ref(d, case)
    kind = row_kinds(d, case["nefc"])
    ch = (np.arange(d.NCHUNK * 64) // 64)[None, :]
    fl = by_row(f64(case["floss"]))
    x0 = rows_cost_ref(d, case)["piece"]
    out = {}
    names = {QUAD: "quadratic", LOWER: "lower", UPPER: "upper", OFF: "off"}
    for where, P, K, CH, FL in (("ls", m["piece"], kind[:, None, :], ch[:, None, :], fl[:, None, :]), ("rows_cost", x0, kind, ch, fl)):
        if d.NEQ:
            out[f"{where} equality quadratic"] = int(((K == EQ) & (P == QUAD)).sum())
        for cls, sel in (("floss 0", FL == 0), ("floss small", (FL > 0) & (FL < 1)), ("floss large", FL >= 1)):
            for p in (LOWER, UPPER) + (() if cls == "floss 0" else (QUAD,)):
                out[f"{where} friction {cls} {names[p]}"] = int(((K == FRIC) & sel & (P == p)).sum())
        for c in range(d.NCHUNK):
            for p in (QUAD, OFF):
                out[f"{where} unilateral chunk {c} {names[p]}"] = int(((K == UNI) & (CH == c) & (P == p)).sum())
    out["D = 0 inside nefc"] = int(((kind != PAD) & (by_row(case["D"]) == 0)).sum())
    out["flat waves"] = int(case["flat"].sum())
    out["ja redrawn for the margin"] = int(case["redrawn"].sum())
    out.update(structure_census(d, case["nl"], case["ncon"]))
    return out


def structure_census(d, nl, ncon):
    out = {}
    nefc = d.NEQ + d.NF + nl + d.NPYR * ncon
    for v in (0, 1, d.NL):
        out[f"nl {v}"] = int((nl == v).sum())
    for v in sorted({0, 1, 2, 3, 4, 5, d.NCON}):
        if v <= d.NCON:
            out[f"ncon {v}"] = int((ncon == v).sum())
    for t in sorted({d.NEQ + d.NF, d.NEFC} | {m + k for m in range(64, d.NEFC + 2, 64) for k in (-1, 0, 1) if d.NEQ + d.NF <= m + k <= d.NEFC}):
        out[f"nefc {t}"] = int((nefc == t).sum())
    G = 1 if d.NBC * d.NCON <= 16 else 64 // d.NV
    for q in sorted({(d.NBC * c) % (4 * G) for c in range(d.NCON + 1)}):
        out[f"contact base rows mod {4 * G} = {q}"] = int(((d.NBC * ncon) % (4 * G) == q).sum())
    return out


def threshold_cases(d):
    """Single-row problems on dyadic numbers (every product and sum exact in fp32, fused or not, or rounded once from an exact
    fp64 value): all rows but one have D = 0, floss = 0, ja = 1, v = 0; g = 0.  R = 1/2, floss = 1/4 (rf = 1/8), D = 4 (not 1 / R:
    the friction row's pieces then differ in value and slope at +-rf, so the piece taken shows in every output).
    Friction row NEQ: x = t through ja = 2 t, v = t, a = -1 for t = -rf, +rf, one fp32 step inside each, one outside each.
    Unilateral row, the first of chunk 0 (NEQ + NF) and, where NCHUNK > 1, row 67: x = 1/2 + 2 v with v = -1/4 (x = 0) and
    v one fp32 step either side (x = -2^-24, +2^-25).  Returns (case, want): want[n] = (row, piece, name)."""
    rf = np.float32(0.125)
    nxt = lambda a, b: np.nextafter(np.float32(a), np.float32(b))
    rows = []
    for name, t, p in (("x == -rf", -rf, LOWER), ("x == +rf", rf, UPPER), ("one step inside -rf", nxt(-rf, 0), QUAD),
                       ("one step inside +rf", nxt(rf, 0), QUAD), ("one step outside -rf", nxt(-rf, -1), LOWER),
                       ("one step outside +rf", nxt(rf, 1), UPPER)):
        rows.append((d.NEQ, np.float32(2) * t, t, -1.0, p, "friction " + name))
    for r in [d.NEQ + d.NF] + ([67] if d.NCHUNK > 1 else []):
        for name, v, p in (("x == 0", -0.25, OFF), ("one step below 0", nxt(-0.25, -1), QUAD), ("one step above 0", nxt(-0.25, 0), OFF)):
            rows.append((r, 0.5, v, 2.0, p, f"unilateral row {r} {name}"))
    n, nr = len(rows), d.NCHUNK * 64
    nefc = np.full(n, d.NEFC, np.int32)
    live = row_kinds(d, nefc) != PAD
    jaref, jv = np.where(live, 1.0, 0.0).astype(np.float32), np.zeros((n, nr), np.float32)
    D, R = np.zeros((n, nr), np.float32), np.full((n, nr), 0.5, np.float32)
    R[~live] = 1.0
    floss = np.where(row_kinds(d, nefc) == FRIC, 0.0, -1.0).astype(np.float32)
    alpha = np.zeros((n, 3), np.float32)
    for i, (r, ja, v, a, p, name) in enumerate(rows):
        jaref[i, r], jv[i, r], D[i, r] = ja, v, 4.0
        if r < d.NEQ + d.NF:
            floss[i, r] = 0.25
        alpha[i] = [a, 0.0, a]
    sh = (n, d.NCHUNK, 64)
    case = dict(nefc=nefc, jaref=jaref.reshape(sh), jv=jv.reshape(sh), D=D.reshape(sh), R=R.reshape(sh), floss=floss.reshape(sh),
                g=np.zeros((n, 3), np.float32), alpha=alpha)
    return case, [(r, p, name) for r, ja, v, a, p, name in rows]


# ---------------------------------------------------------------- the Jacobian products
def j_cases(d, seed=2):
    """The NWAVE waves of the jdot / jt_force tests (read-only): nl, ncon, nefc, nbase [n]; B [n, NBASE, NV] base rows (fp32: an
    equality row has two entries, friction rows a +1 and limit rows a +-1 on distinct dofs of their own kind, contact base rows
    dense N(0, 1) 10^U(-2, 1)); bmu [n, NBASE]: per contact direction 0, 1e-3 U(.5, 2) or U(1.2, 3); sdof [n, NSP]; mu, bn, bk
    [n, NCHUNK, 64] as make_constraint sets them (padding: 0, NBASE, NBASE); v [n, NV]; force [n, NCHUNK, 64] (a third of the live
    rows exactly zero, padding rows zero)."""
    rng = np.random.default_rng([seed, d.NEFC])
    n, nr, nsp = NWAVE, d.NCHUNK * 64, d.NEQ + d.NF + d.NL
    nl, ncon = structures(d)
    r_lim = d.NEQ + d.NF
    rcon = r_lim + nl
    nefc, nbase = rcon + d.NPYR * ncon, rcon + d.NBC * ncon
    B = np.zeros((n, d.NBASE, d.NV), np.float32)
    bmu = np.zeros((n, d.NBASE), np.float32)
    sdof = np.zeros((n, nsp), np.int32)
    mu = np.zeros((n, nr), np.float32)
    bn = np.full((n, nr), d.NBASE, np.int32)
    bk = np.full((n, nr), d.NBASE, np.int32)
    for e in range(n):
        for r in range(d.NEQ):
            i, j = rng.choice(d.NV, 2, replace=False)
            B[e, r, i], B[e, r, j] = 1.0, -rng.normal()
        fd = rng.permutation(d.NV)[:d.NF]
        ld = rng.permutation(d.NV)[:nl[e]]
        B[e, d.NEQ + np.arange(d.NF), fd] = 1.0
        B[e, r_lim + np.arange(nl[e]), ld] = rng.choice([-1.0, 1.0], nl[e])
        sdof[e, d.NEQ:r_lim] = fd
        sdof[e, r_lim:rcon[e]] = ld
        nb = d.NBC * ncon[e]
        B[e, rcon[e]:nbase[e]] = rng.normal(size=(nb, d.NV)) * 10.0 ** rng.uniform(-2, 1, (nb, 1))
        cls = rng.integers(0, 3, nb)
        m = np.select([cls == 0, cls == 1], [0.0, 1e-3 * rng.uniform(0.5, 2, nb)], rng.uniform(1.2, 3, nb))
        m[::d.NBC] = 0.0                                   # (normal rows: unused)
        bmu[e, rcon[e]:nbase[e]] = m
        bn[e, :rcon[e]] = bk[e, :rcon[e]] = np.arange(rcon[e])
        for c in range(ncon[e]):
            for ed in range(d.NPYR):
                r = rcon[e] + d.NPYR * c + ed
                bn[e, r] = rcon[e] + d.NBC * c
                bk[e, r] = bn[e, r] + 1 + (ed >> 1)
                mu[e, r] = -bmu[e, bk[e, r]] if ed & 1 else bmu[e, bk[e, r]]
    live = np.arange(nr)[None, :] < nefc[:, None]
    force = rng.normal(size=(n, nr)) * 10.0 ** rng.uniform(-2, 3, (n, nr))
    force[rng.uniform(size=(n, nr)) < 1 / 3] = 0.0
    force = np.where(live, force, 0.0).astype(np.float32)
    v = (rng.normal(size=(n, d.NV)) * 10.0 ** rng.uniform(-2, 2, (n, d.NV))).astype(np.float32)
    sh = (n, d.NCHUNK, 64)
    c = dict(nl=nl.astype(np.int32), ncon=ncon.astype(np.int32), nefc=nefc, nbase=nbase, B=B, bmu=bmu, sdof=sdof, mu=mu.reshape(sh),
             bn=bn.reshape(sh), bk=bk.reshape(sh), v=v, force=force.reshape(sh))
    for a in c.values():
        a.setflags(write=False)
    return c


def j_pyramid(d, case):
    """(J [n, rows, NV], |J|): row r = B[bn_r] + mu_r B[bk_r] of the rows below nefc, zero rows from there on; |J| the same with
    magnitudes (|B[bn]| + |mu| |B[bk]|)"""
    n = len(case["nefc"])
    B = np.concatenate([f64(case["B"]), np.zeros((n, 1, d.NV))], 1)
    bn, bk, mu = by_row(case["bn"]), by_row(case["bk"]), by_row(f64(case["mu"]))
    live = (np.arange(d.NCHUNK * 64)[None, :] < case["nefc"][:, None])[:, :, None]
    e = np.arange(n)[:, None]
    J = np.where(live, B[e, bn] + mu[:, :, None] * B[e, bk], 0.0)
    Ja = np.where(live, np.abs(B[e, bn]) + np.abs(mu[:, :, None] * B[e, bk]), 0.0)
    return J, Ja


def j_ref(d, case):
    """jv = J v [n, rows] and qfc = J^T f [n, NV] with their bounds b_jv, b_qfc"""
    n = len(case["nefc"])
    J, _ = j_pyramid(d, case)
    B = np.concatenate([np.abs(f64(case["B"])), np.zeros((n, 1, d.NV))], 1)
    bn, bk, mu = by_row(case["bn"]), by_row(case["bk"]), np.abs(by_row(f64(case["mu"])))
    v, f = f64(case["v"]), by_row(f64(case["force"]))
    e = np.arange(n)[:, None]
    live = np.arange(d.NCHUNK * 64)[None, :] < case["nefc"][:, None]
    depth = d.NV // 2 + 1
    sn, sk = B[e, bn] @ np.abs(v)[:, :, None], mu[:, :, None] * (B[e, bk] @ np.abs(v)[:, :, None])
    b_jv = np.where(live, U * ((1 + depth + 2) * sn[..., 0] + (2 + depth + 2) * sk[..., 0]), 0.0)
    _, Ja = j_pyramid(d, case)
    quart = -(-d.NBC * d.NCON // 4)
    if d.NBC * d.NCON <= 16:
        jdepth = 2 * quart + d.NEQ + 1
    else:
        G = 64 // d.NV
        jdepth = 2 * -(-quart // G) + 1 + d.NEQ + G
    cj = max(d.NPYR // 2, 2) + 1 + jdepth + 2
    b_qfc = cj * U * np.einsum("nri,nr->ni", Ja, np.abs(f))
    return dict(jv=np.einsum("nri,ni->nr", J, v), qfc=np.einsum("nri,nr->ni", J, f), b_jv=b_jv, b_qfc=b_qfc, c_qfc=cj)
