"""Plane-sphere, plane-capsule and plane-cylinder contacts in plain numpy fp64, written from the geometry: the lowest point of a
sphere, the two end spheres of a capsule, and points of the rim circle of the cylinder's disk that faces the plane.  It shares no
code with the oracle (oracle/rsr_oracle.c) and does not follow its order of operations; tests/test_planeprim.py holds it against
the f64 oracle to 1e-9.

Every function takes the plane's pose and the primitive's pose as the model's geom poses (position [3], matrix [9] or [3, 3], row
major, the plane's normal and the primitive's axis in the third column) and returns a dict:

    kind      "sphere" / "capsule" / "cylinder"
    point     [3]      a point of the plane (its geom's position)
    normal    [3]      the plane's normal
    dist      [k]      height of each contact's surface point above the plane (k = 1, 2, 3: every point, penetrating or not)
    pos       [k, 3]   surface point - normal * dist / 2
    surface   [k, 3]   the surface points themselves
    frame     [3, 3]   capsules only: rows (n, b, n x b), b the first tangent
    margins   {name: distance of a threshold quantity from its threshold}, see below
    margin    the least of them

and the quantities the classes are made of (capsule: bn, na, theta; cylinder: prj, len, theta, flat, facing).

Threshold quantities: `bn - 0.5` (capsule: the length of the axis' projection into the plane against the tangent fallback),
`|prjaxis| hl - 1e-3` (cylinder: lying flat), `len` (cylinder: the axis against the normal, where the rim direction is lost),
`len - 1e-2` (cylinder: where the rim direction is made orthogonal to the axis), `|prjaxis|` (cylinder: which disk faces the plane) and `dist - includemargin` of every point (in contact or not)."""
import numpy as np

HALF = 0.5            # a capsule axis whose projection into the plane is shorter than this gets a fixed tangent
FLAT = 1e-3           # |axis . n| * half length below which a cylinder counts as lying flat
NEAR = 1e-2           # |n - (n . a) a| below which the rim direction is made orthogonal to the axis explicitly
ALIGNED = 1e-12       # |n - (n . a) a| below which the rim direction is taken from the cylinder's x axis


def _plane(ppos, pmat):
    return np.asarray(ppos, float), np.asarray(pmat, float).reshape(3, 3)[:, 2]


def _finish(r, includemargin):
    r["pos"] = r["surface"] - 0.5 * np.outer(r["dist"], r["normal"])
    for i, d in enumerate(r["dist"]):
        r["margins"][f"dist {i}"] = abs(d - includemargin)
    r["touching"] = r["dist"] < includemargin
    r["margin"] = min(r["margins"].values())
    return r


def plane_sphere(ppos, pmat, cpos, radius, includemargin=0.0):
    """one point under the centre: dist = (c - p) . n - r, pos = c - n (r + dist / 2)"""
    p, n = _plane(ppos, pmat)
    low = np.asarray(cpos, float) - n * radius                    # the sphere's lowest point
    r = dict(kind="sphere", point=p, normal=n, surface=low[None], dist=np.array([(low - p) @ n]), margins={})
    return _finish(r, includemargin)


def plane_capsule(ppos, pmat, cpos, cmat, radius, halflen, includemargin=0.0):
    """the end spheres, +axis end first; frame (n, b, n x b) with b the axis projected into the plane and normalised, or, where
    that projection is shorter than 0.5, (0, 1, 0) for |n_y| < 0.5 and (0, 0, 1) otherwise"""
    p, n = _plane(ppos, pmat)
    c, a = np.asarray(cpos, float), np.asarray(cmat, float).reshape(3, 3)[:, 2]
    ends = np.stack([c + a * halflen, c - a * halflen])
    low = ends - n * radius
    na = float(a @ n)
    inplane = a - n * na
    bn = float(np.linalg.norm(inplane))
    if bn < HALF:
        b = np.array([0.0, 1.0, 0.0]) if abs(n[1]) < 0.5 else np.array([0.0, 0.0, 1.0])
    else:
        b = inplane / bn
    r = dict(kind="capsule", point=p, normal=n, surface=low, dist=(low - p) @ n, frame=np.stack([n, b, np.cross(n, b)]),
             bn=bn, na=na, theta=float(np.arctan2(bn, na)), fallback=bn < HALF, margins={"bn": abs(bn - HALF)})
    return _finish(r, includemargin)


def plane_cylinder(ppos, pmat, cpos, cmat, radius, halflen, includemargin=0.0):
    """three points: the rim point of least height on the disk that faces the plane, and the rim points 120 degrees to either
    side of it on the same disk; for a cylinder lying flat (|a . n| hl < 1e-3) the second point is instead the least-height rim
    point of the other disk.  With the axis along the normal (every rim point as low as the others) the first point is the one
    on the cylinder's own x axis."""
    p, n = _plane(ppos, pmat)
    c, R = np.asarray(cpos, float), np.asarray(cmat, float).reshape(3, 3)
    a = R[:, 2]
    prj = float(a @ n)
    down = -a if prj >= 0.0 else a                                 # the axis, pointing at the plane
    facing, other = c + down * halflen, c - down * halflen
    # steepest descent on a disk: -n projected into the disks' plane.  The columns of geom_xmat are unit to 1e-8 only, so
    # down (down . n) - n keeps (|down|^2 - 1) (down . n) along the axis; within NEAR of alignment, where that would count, it is removed
    slope = down * (down @ n) - n
    near = float(np.linalg.norm(slope))
    if near < NEAR:
        slope = slope - down * ((slope @ down) / (down @ down))
    ln = float(np.linalg.norm(slope))
    u = R[:, 0] if ln < ALIGNED else slope / ln
    side = np.cross(u, down)                                       # along the rim at u, a third of a turn's sine away
    side = side / np.linalg.norm(side) * np.sin(2.0 * np.pi / 3.0)
    rim = [facing + radius * u, facing + radius * (np.cos(2.0 * np.pi / 3.0) * u + side), facing + radius * (np.cos(2.0 * np.pi / 3.0) * u - side)]
    flat = abs(prj) * halflen < FLAT
    if flat:
        rim[1] = other + radius * u
    rim = np.stack(rim)
    r = dict(kind="cylinder", point=p, normal=n, surface=rim, dist=(rim - p) @ n, prj=prj, len=ln, theta=float(np.arctan2(ln, abs(prj))),
             flat=bool(flat), facing=facing, other=other, axis=a, radius=radius, halflen=halflen,
             margins={"flat": abs(abs(prj) * halflen - FLAT), "len": ln, "near": abs(near - NEAR), "sign": abs(prj)})
    return _finish(r, includemargin)
