"""Plain numpy fp64 restatement of the box-box and plane-box contact manifolds (the operation of box_box_sat, plane_box_sat and the
clip / manifold block of collision<C>), written from the definition and sharing nothing with the oracle's C: overlap on the 15 axes
from support functions, reference and incident face, Sutherland-Hodgman clipping of the incident face to the reference rectangle,
vertex depths, and the selection rule (first candidate; farthest from it; farthest from their line; farthest on the other side).

It also returns what a test needs to decide, reference-side only, whether a pose is clear of the operation's thresholds
(`margin`) and which picks are within a tolerance of the winning value (`selection_outcomes`).

Frames are 3x3 matrices whose COLUMNS are the box axes (geom_xmat reshaped to 3x3).  tests/test_boxbox_manifold.py tests this
module against the f64 oracle; tests/boxbox_cases.py holds what the tests build around it (pairs of a model, labels, census)."""
import numpy as np

PAD = 1e-6          # added to |cos| between axes of different boxes
PREF = 0.95         # an edge axis wins only if best_edge > PREF * best_face + PAD
BAND = 1e-3         # plane-box: vertices within 1 mm of the deepest one are candidates
PARALLEL = 1e-6     # edge axes with 1 - cos^2 below this are skipped


def selection(x, y, mask):
    """(a, b, c, d) of the selection rule over the candidates mask[i] of the points (x[i], y[i]); d is None if no candidate lies
    strictly on the other side of line ab from c.  First maximum wins."""
    x, y, mask = np.asarray(x, float), np.asarray(y, float), np.asarray(mask, bool)
    cand = np.nonzero(mask)[0]
    a = int(cand[0])
    d2 = (x[a] - x) ** 2 + (y[a] - y) ** 2
    b = int(cand[np.argmax(d2[cand])])
    cr = (x[a] - x) * -(y[a] - y[b]) + (y[a] - y) * (x[a] - x[b])
    c = int(cand[np.argmax(np.abs(cr[cand]))])
    other = -np.sign(cr[c]) * cr if cr[c] != 0 else -cr
    d = int(cand[np.argmax(other[cand])])
    if not other[d] > 0:
        d = None
    return a, b, c, d


def _dedupe(idx):
    out = []
    for i in idx:
        if i is not None and i not in out:
            out.append(i)
    return out


def selection_outcomes(x, y, mask, tol=0.0, rel=0.0):
    """Every index set the selection rule can produce when a pick within `tol` (a length: distances, and cross products divided by
    |ab|) or within `rel` of the winning value may replace the winner.  One set = the selection is clear at that tolerance."""
    x, y, mask = np.asarray(x, float), np.asarray(y, float), np.asarray(mask, bool)
    cand = np.nonzero(mask)[0]
    a = int(cand[0])
    out = set()
    dist = np.sqrt((x[a] - x) ** 2 + (y[a] - y) ** 2)
    near = lambda v, best: v >= best - tol - rel * abs(best)
    for b in cand[near(dist[cand], dist[cand].max())]:
        lab = max(dist[b], 1e-300)
        cr = ((x[a] - x) * -(y[a] - y[b]) + (y[a] - y) * (x[a] - x[b])) / lab
        ac = np.abs(cr)
        for c in cand[near(ac[cand], ac[cand].max())]:
            sides = (1.0, -1.0) if ac[c] <= tol else (np.sign(cr[c]),)
            for sg in sides:
                other = -sg * cr
                best = other[cand].max()
                if best > tol:
                    for d in cand[near(other[cand], best)]:
                        out.add(frozenset(_dedupe([a, int(b), int(c), int(d)])))
                else:
                    out.add(frozenset(_dedupe([a, int(b), int(c)])))
                    if best > 0:
                        out.add(frozenset(_dedupe([a, int(b), int(c), int(cand[np.argmax(other[cand])])])))
    return out


def box_vertices(pos, R, size):
    """the eight vertices, index bits (4, 2, 1) = +x, +y, +z"""
    sg = np.array([[(v >> 2) & 1, (v >> 1) & 1, v & 1] for v in range(8)], float) * 2 - 1
    return (sg * size) @ np.asarray(R, float).reshape(3, 3).T + pos


def plane_box(pp, Rp, bp, Rb, size):
    """Plane (normal = third column of Rp) against a box.  Returns a dict: kind 'none' / 'plane'; support[8] (> 0: below the
    plane), smax, mask[8] (the band), vertices[8, 3], x / y (in-plane coordinates), sel (vertex indices in the order a, b, c, d),
    dist[k], pos[k, 3], normal, margin (smallest distance of smax from 0 and of a support from the band edge)."""
    pp, bp, size = (np.asarray(v, float) for v in (pp, bp, size))
    Rp = np.asarray(Rp, float).reshape(3, 3)
    n = Rp[:, 2]
    V = box_vertices(bp, Rb, size)
    sup = (pp - V) @ n
    smax = sup.max()
    r = dict(kind="none", normal=n, support=sup, smax=smax, vertices=V, margin=abs(smax))
    if not smax > 0:
        return r
    thr = max(smax - BAND, 0.0)
    mask = sup > thr
    x, y = V @ Rp[:, 0], V @ Rp[:, 1]
    sel = _dedupe(selection(x, y, mask))
    dist = -sup[sel]
    r.update(kind="plane", mask=mask, x=x, y=y, sel=sel, dist=dist, pos=V[sel] - 0.5 * dist[:, None] * n, thr=thr,
             margin=min(abs(smax), np.abs(sup - thr).min()))
    return r


def sat(pa, Ra, sa, pb, Rb, sb):
    """The 15 separating values (negative = overlap; 6 face axes A0 A1 A2 B0 B1 B2, then 9 edge axes A_i x B_j, nan where the
    two edges are parallel) from the boxes' supports along each axis, with PAD on the cross-box cosines."""
    A, B = np.asarray(Ra, float).reshape(3, 3).T, np.asarray(Rb, float).reshape(3, 3).T      # rows = axes
    sa, sb = np.asarray(sa, float), np.asarray(sb, float)
    dp = np.asarray(pb, float) - np.asarray(pa, float)
    C = A @ B.T
    AC = np.abs(C) + PAD
    t = A @ dp
    face = np.concatenate([np.abs(t) - (sa + AC @ sb), np.abs(B @ dp) - (sb + AC.T @ sa)])
    edge = np.full((3, 3), np.nan)
    for i in range(3):
        for j in range(3):
            l2 = 1.0 - C[i, j] ** 2
            if l2 < PARALLEL:
                continue
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            # L = A_i x B_j = C[i1, j] A_i2 - C[i2, j] A_i1; support of each box along L: |L . A_i1| = |C[i2, j]| and so on, padded
            L_dp = t[i2] * C[i1, j] - t[i1] * C[i2, j]
            ra = sa[i1] * AC[i2, j] + sa[i2] * AC[i1, j]
            rb = sb[j1] * AC[i, j2] + sb[j2] * AC[i, j1]
            edge[i, j] = (abs(L_dp) - (ra + rb)) / np.sqrt(l2)
    return face, edge, A, B, dp


def clip_polygon(px, py, pd, hu, hv):
    """Sutherland-Hodgman against x <= hu, x >= -hu, y <= hv, y >= -hv in that order; a kept vertex is written before its edge's
    intersection.  Returns the final (x, y, depth) lists and the vertex count after each pass."""
    P = list(zip(px, py, pd))
    counts = []
    for side in range(4):
        h, sg, ax = (hu if side < 2 else hv), (-1.0 if side & 1 else 1.0), (0 if side < 2 else 1)
        Q = []
        for i, p in enumerate(P):
            q = P[(i + 1) % len(P)]
            d1, d2 = h - sg * p[ax], h - sg * q[ax]
            if d1 >= 0:
                Q.append(p)
            if (d1 >= 0) != (d2 >= 0):
                t = d1 / (d1 - d2)
                Q.append(tuple(p[k] + t * (q[k] - p[k]) for k in range(3)))
        P = Q
        counts.append(len(P))
        if not P:
            break
    return (np.array([p[k] for p in P]) for k in range(3)), counts


def box_box(pa, Ra, sa, pb, Rb, sb, force=None):
    """force: None, or ("face", code) / ("edge", i, j) to build the contact on that axis whatever the SAT prefers (a test uses it
    to rate a result that took another axis whose separating value is within its tolerance of the winning one).

    Returns a dict: kind 'sep' / 'none' (overlapping on all axes, no penetrating point) / 'edge' / 'face'; sep_face[6],
    sep_edge[3, 3], best_face, face_code, best_edge, margin (smallest distance of any threshold quantity from its threshold);
    edge: wi, wj, qa, qb; face: nref, nref_sign, flip, mq, o, axu, axv, hu, hv, poly_x / poly_y / poly_d (final polygon),
    pass_counts, mask; and for both the contact itself: normal, dist[k], pos[k, 3], sel."""
    pa, pb, sa, sb = (np.asarray(v, float) for v in (pa, pb, sa, sb))
    face, edge, A, B, dp = sat(pa, Ra, sa, pb, Rb, sb)
    r = dict(kind="sep", sep_face=face, sep_edge=edge)
    allsep = np.concatenate([face, edge.ravel()[~np.isnan(edge.ravel())]])
    r["margin"] = abs(allsep.max())          # separated: the largest value decides; overlapping: the one nearest to 0 does
    if (allsep > 0).any():
        return r
    face_code = int(np.argmax(face)) if force is None or force[0] != "face" else force[1]
    best_face = face[face_code]
    r.update(kind="none", face_code=face_code, best_face=best_face)
    if not np.isnan(edge).all() and (force is None or force[0] == "edge"):
        flat = np.where(np.isnan(edge), -np.inf, edge).ravel()
        wi, wj = divmod(int(np.argmax(flat)), 3) if force is None else force[1:]
        best_edge = flat[3 * wi + wj]
        r["best_edge"], r["edge_ij"] = best_edge, (wi, wj)
        if force is None:
            r["margin"] = min(r["margin"], abs(best_edge - (PREF * best_face + PAD)))
        if force is not None or best_edge > PREF * best_face + PAD:
            L = np.cross(A[wi], B[wj])
            L = L / np.linalg.norm(L)
            if L @ dp < 0:
                L = -L
            # the supporting edges: A's farthest along +L, B's farthest along -L
            ea, eb = pa.copy(), pb.copy()
            for k in range(3):
                if k != wi:
                    ea += (1.0 if L @ A[k] > 0 else -1.0) * sa[k] * A[k]
                if k != wj:
                    eb -= (1.0 if L @ B[k] > 0 else -1.0) * sb[k] * B[k]
            # closest points of the two lines, each clamped to its edge
            w = eb - ea
            u = A[wi] @ B[wj]
            M = np.array([[1.0, -u], [u, -1.0]])
            s, t = np.linalg.solve(M, [A[wi] @ w, B[wj] @ w])
            s, t = np.clip(s, -sa[wi], sa[wi]), np.clip(t, -sb[wj], sb[wj])
            qa, qb = ea + s * A[wi], eb + t * B[wj]
            dist = (qb - qa) @ L
            r.update(wi=wi, wj=wj, best_edge=best_edge, qa=qa, qb=qb, normal=L)
            r["margin"] = min(r["margin"], abs(dist))
            if dist < 0:
                r.update(kind="edge", dist=np.array([dist]), pos=0.5 * (qa + qb)[None], sel=[0])
            return r
    ref_is_a = face_code < 3
    k = face_code % 3
    (pr, Rr, sr), (pq, Rq, sq) = ((pa, A, sa), (pb, B, sb)) if ref_is_a else ((pb, B, sb), (pa, A, sa))
    nref = Rr[k].copy()
    nref_sign = 1
    if nref @ (pq - pr) < 0:
        nref, nref_sign = -nref, -1
    dots = Rq @ nref
    mq = int(np.argmax(np.abs(dots)))
    sgn_q = -1.0 if dots[mq] > 0 else 1.0
    uq, vq, ur, vr = (mq + 1) % 3, (mq + 2) % 3, (k + 1) % 3, (k + 2) % 3
    axu, axv, hu, hv = Rr[ur], Rr[vr], sr[ur], sr[vr]
    o = pr + nref * sr[k]
    centre = pq + sgn_q * sq[mq] * Rq[mq]
    W = np.array([centre + su * sq[uq] * Rq[uq] + sv * sq[vq] * Rq[vq] - o for su, sv in ((1, 1), (-1, 1), (-1, -1), (1, -1))])
    (x, y, dep), counts = clip_polygon(W @ axu, W @ axv, -(W @ nref), hu, hv)
    normal = nref if ref_is_a else -nref
    r.update(nref=nref, nref_sign=nref_sign, flip=not ref_is_a, mq=mq, o=o, axu=axu, axv=axv, hu=hu, hv=hv, normal=normal,
             poly_x=x, poly_y=y, poly_d=dep, pass_counts=counts, incident=(W @ axu, W @ axv, -(W @ nref)))
    if len(dep):
        r["margin"] = min(r["margin"], np.abs(dep).min())
    mask = dep > 0
    r["mask"] = mask
    if not mask.any():
        return r
    sel = _dedupe(selection(x, y, mask))
    r.update(kind="face", sel=sel, dist=-dep[sel],
             pos=o + np.outer(x[sel], axu) + np.outer(y[sel], axv) - 0.5 * np.outer(dep[sel], nref))
    return r
