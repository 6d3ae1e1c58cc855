"""What the physics-layer GPU tests (tests/test_*_gpu.py on rsr_mjx_amd/physics.py) share: batches and states (with the seeded default
randomisation, the replica batch and the applied forces of the rollout tests; tools/rates_support.py takes them from here), bitwise comparison,
the error rule, the CPU oracle's reference pass, the row-count exclusion, contact wrenches from the oracle's rows, and snapshots of
everything a Physics handle owns.  Plain functions; torch is imported inside them, so collection works without a GPU.

The error of a field is per env and relative: rel(hip, ref) = |hip - ref|_inf / max(1, |ref|_inf of that env's field).
The rule (rule) bounds it against the f64 oracle with the f32 oracle's own distance from the f64 oracle as the spread:
    p99 <= 1e-5, or p99 <= 3 x the spread's p99; and every env within max(1e-4, 20 x the spread's largest value).
The exclusion (keep): an env whose row counts (ne, nf, nl, ncon) differ between the kernel and the f64 oracle, or between the f32 and
the f64 oracle, is a contact or limit mode flip and is left out of the comparison; at most 2 % of the envs may be."""
import hashlib

import numpy as np

from rsr_mjx_amd import prng
from rsr_mjx_amd.envs.families import FAMILIES

PIPE = ("qpos", "qvel", "ctrl", "qacc_warmstart", "time", "xpos", "site_xpos")
GO2 = ("go2flat", "go2rough", "footstand")
IMPLICIT = ("cube", "tshape")
ALL = ("qpos", "qvel", "time", "actuator_force", "ncon", "sensordata")          # every field a rollout can record

# every supported sensor type on the Airbot endpoint (and on the T-shape's tail sites, framepos with a ref site)
AIRBOT_SPEC = [("pos", "framepos", "endpoint"), ("linvel", "framelinvel", "endpoint"), ("angvel", "frameangvel", "endpoint"),
               ("gyro", "gyro", "endpoint"), ("vel", "velocimeter", "endpoint"), ("quat", "framequat", "endpoint"),
               ("xaxis", "framexaxis", "endpoint"), ("zaxis", "framezaxis", "endpoint")]
TSHAPE_SPEC = AIRBOT_SPEC + [("tail_in_ee", "framepos", "T_tail", "endpoint")]
GO2_EXTRA = [("FR_vel", "velocimeter", "FR"), ("FR_quat", "framequat", "FR")]          # (55 + 7 floats: within the 64 cap)


def sensor_spec(kind, envdef):
    """the rollout tests' sensor table of a family"""
    if kind == "cube":
        return AIRBOT_SPEC
    if kind == "tshape":
        return TSHAPE_SPEC
    return envdef.sensors + GO2_EXTRA


# ---- batches and states

def action_scale(kind):
    """the scale of the random actions that move a family's batch off its reset state"""
    return 1.0 if kind in IMPLICIT else 0.5


def default_dr(kind, envdef, n):
    """the seeded randomisation of n envs that make(kind, n, True) applies, or None for the T-shape (the Airbot randomisation of
    domain_randomize.py is the cube scene's)"""
    from rsr_mjx_amd.envs import airbot, go2
    if kind == "tshape":
        return None
    if kind == "cube":
        return airbot.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(5), n))
    return go2.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(12), n))


def make(kind, n, dr_on, variant=None):
    """(envdef, batched env, dr dict or None, action scale); no Episode / AutoReset wrappers, no Go2 kicks.  variant: a name of
    tests/model_variants.py, applied to envdef.sys.arrays before the batch (and its blob) is built."""
    from model_variants import envdef_of
    envdef = envdef_of(kind, variant)
    dr = default_dr(kind, envdef, n) if dr_on else None
    return envdef, envdef.batched(n, randomization=dr), dr, action_scale(kind)


def pair(kind, n, seed=3, steps=3):
    """Two batches in the same state (records equal bit for bit) after a few env steps, same DR: (envdef, A, B, scale, rng)."""
    import torch
    dr_on = kind != "tshape"                 # (the Airbot randomisation of domain_randomize.py is the cube scene's)
    envdef, A, _, scale = make(kind, n, dr_on)
    _, B, _, _ = make(kind, n, dr_on)
    rng = np.random.default_rng(seed)
    A.reset(prng.split(prng.PRNGKey(7), n))
    B.reset(prng.split(prng.PRNGKey(7), n))
    for _ in range(steps):
        A.step(None, np.clip(rng.normal(size=(n, A.dims.nu)) * scale, -1, 1).astype(np.float32))
    B.record.copy_(A.record)
    torch.cuda.synchronize()
    return envdef, A, B, scale, rng


def replica(kind, envdef, A, k, dr="default"):
    """A.num_envs * k envs: env e * k + j holds env e's record row and per-env leaves.  dr: the randomisation A was built with
    (the family's default_dr unless given; None: the replica gets no per-env leaves)"""
    import torch
    if dr == "default":
        dr = default_dr(kind, envdef, A.num_envs)
    R = envdef.batched(A.num_envs * k, randomization=None if dr is None else {f: np.repeat(np.asarray(v), k, 0) for f, v in dr.items()})
    R.reset(prng.split(prng.PRNGKey(7), A.num_envs * k))
    R.record.copy_(A.record.repeat_interleave(k, 0))
    torch.cuda.synchronize()
    return R


def applied_forces(envdef, n, nv, rng):
    """xfrc of the order of a third of each body's weight on every body, and a qfrc"""
    m = np.maximum(envdef.sys.arrays["body_mass"], 0.05)[None, :, None]
    x = rng.normal(size=(n, m.shape[1], 6))
    x[:, :, :3] *= 9.81 * m * 0.3
    x[:, :, 3:] *= 0.981 * m * 0.3
    return x.astype(np.float32), (rng.normal(size=(n, nv)) * 0.5).astype(np.float32)


_STATES = {}


def perturb(A, qpos, qvel, seed):
    """(qpos, qvel, ctrl) in fp32: the given reset states [n, nq] / [n, nv] with hinge and slide angles moved by N(0, 0.05), qvel by
    N(0, 0.2), and a ctrl drawn uniformly inside the control range, from default_rng(seed); A: the model's arrays"""
    n = len(qpos)
    rng = np.random.default_rng(seed)
    qpos, qvel = np.asarray(qpos).astype(np.float64), np.asarray(qvel).astype(np.float64)
    jt, qa = A["jnt_type"], A["jnt_qposadr"]
    for j in range(len(jt)):
        if jt[j] in (2, 3):                               # hinge / slide: perturb the angle
            qpos[:, qa[j]] += rng.normal(scale=0.05, size=n)
    qvel += rng.normal(scale=0.2, size=qvel.shape)
    lo, hi = A["actuator_ctrlrange"][:, 0], A["actuator_ctrlrange"][:, 1]
    ctrl = lo + (hi - lo) * rng.uniform(size=(n, len(lo)))
    return qpos.astype(np.float32), qvel.astype(np.float32), ctrl.astype(np.float32)


def random_states(envdef, kind, n, seed):
    """Reset distribution of the shipped env plus perturb(): a perturbation of qpos / qvel, and a random ctrl inside the control
    range.  Computed once per (kind, n, seed); every call gets copies of its own."""
    if (kind, n, seed) not in _STATES:
        import torch
        _, E, _, _ = make(kind, n, False)
        E.reset(prng.split(prng.PRNGKey(seed), n))
        torch.cuda.synchronize()
        _STATES[(kind, n, seed)] = perturb(envdef.sys.arrays, E.view("qpos").cpu().numpy(), E.view("qvel").cpu().numpy(), seed)
    return tuple(a.copy() for a in _STATES[(kind, n, seed)])


def free_states(envdef, kind, n, seed, zero_vel=False):
    """random_states moved clear of every contact and joint limit: free bodies (the Airbot's cube / target / T block) parked
    apart in the air or the Go2 trunk lifted to 1 m, limited joints kept 0.02 inside their range (the middle of a range narrower
    than 0.1: the Airbot's link4 and fingers).  The Airbot's shoulder (its second joint) is raised by 0.3 rad: the reset pose
    holds the fingers a centimetre above the table, and the perturbation of random_states puts them into it in 12 of 256
    T-shape envs (CPU oracle)."""
    qpos, qvel, ctrl = random_states(envdef, kind, n, seed)
    A = envdef.sys.arrays
    if kind in ("cube", "tshape"):
        qpos[:, int(A["jnt_qposadr"][1])] += 0.3
    for j in range(len(A["jnt_type"])):
        jt, qa = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j])
        if jt == 0:
            qpos[:, qa:qa + 3] = [0.0, 0.0, 1.0] if kind not in ("cube", "tshape") else [3.0 + j, 3.0, 2.0]
        elif A["jnt_limited"][j]:
            lo, hi = float(A["jnt_range"][j, 0]), float(A["jnt_range"][j, 1])
            qpos[:, qa] = 0.5 * (lo + hi) if hi - lo < 0.1 else np.clip(qpos[:, qa], lo + 0.02, hi - 0.02)
    if zero_vel:
        qvel[:] = 0.0
    return qpos, qvel, ctrl


def setup(kind, n=256, seed=11, sensors=None, zero_floss=False, variant=None):
    """(envdef, E, Physics(E, sensors), qpos, qvel, ctrl): a DR-off batch after reset(PRNGKey(1)) and random_states(kind, n, seed),
    not yet written into it; zero_floss: dof friction loss zeroed through the batch's per-env leaf; variant: see make (the states
    stay those of the shipped model)."""
    from rsr_mjx_amd.physics import Physics
    envdef, E, _, _ = make(kind, n, False, variant)
    if zero_floss:
        E.set_randomization({"dof_frictionloss": np.zeros((n, E.dims.nv), np.float32)})
    E.reset(prng.split(prng.PRNGKey(1), n))
    return (envdef, E, Physics(E, sensors=sensors)) + random_states(envdef, kind, n, seed)


# ---- comparison

def bits(t):
    """bitwise view: Go2 records hold PRNG key words, some of them NaN patterns"""
    import torch
    return t.contiguous().view(torch.int32)


def assert_bitwise(name, a, b):
    import torch
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if not torch.equal(bits(a), bits(b)):
        d = (a.double() - b.double()).abs()
        raise AssertionError(f"{name}: {int((bits(a) != bits(b)).sum())} elements differ, max |d| {float(d.max()):.3e}")


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    return (np.abs(a - b) / np.maximum(1.0, np.abs(b).max(1, keepdims=True))).max(1)


def rule(kind, what, err, spread, fails):
    """The project's bound on a dynamic field (see the module docstring); prints p99 / max, appends to `fails`."""
    p99, mx = float(np.quantile(err, 0.99)), float(err.max())
    sp99, smx = float(np.quantile(spread, 0.99)), float(spread.max())
    print(kind, what, "p99 %.2e max %.2e f32-f64 p99 %.2e max %.2e" % (p99, mx, sp99, smx))
    if not (p99 <= 1e-5 or p99 <= 3.0 * sp99):
        fails.append(f"{kind} {what}: p99 {p99:.2e}")
    cap = max(1e-4, 20.0 * smx)
    if not (err <= cap).all():
        fails.append(f"{kind} {what}: {(err > cap).sum()} envs beyond the cap {cap:.2e}, max {mx:.2e}")


# ---- the CPU oracle's reference pass

_PASSES = {}
_PER_DOF = ("qfrc_constraint", "qfrc_smooth", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qacc")
_PER_ROW = ("efc_aref", "efc_D", "efc_R", "efc_floss")


def oracle_pass(oracle_mod, blob, dims, qpos, qvel, ctrl, warm=None, ncon_cap=None, precisions=("f32", "f64")):
    """{precision: per-env list of dicts} of Oracle.forward(qpos, qvel, ctrl, warm or zeros) on `blob` with the contact cap set to
    `ncon_cap` (default dims.ncon_max): efc_force (padded to dims.nefc_max), efc_J [nefc, nv], efc_aref, efc_D, efc_R, efc_floss,
    qfrc_constraint, qfrc_smooth, qfrc_bias, qfrc_passive, qfrc_actuator, qacc, M [nv, nv], contacts [ncon, 10], xpos [nbody, 3],
    xmat [nbody, 3, 3] and the counts nefc, ne, nf, ncon.  Meant to run at the oracle's default switches (tests/conftest.py resets
    them before every test).  Cached under a hash of the blob, the inputs, the cap and the precisions; every module that asks for
    the same pass shares the result, so its arrays are read-only."""
    nv = int(dims.nv)
    cap = int(dims.ncon_max if ncon_cap is None else ncon_cap)
    h = hashlib.sha1(blob)
    for a in (qpos, qvel, ctrl, warm):
        a = None if a is None else np.ascontiguousarray(a)
        h.update(repr(None if a is None else (a.dtype.str, a.shape)).encode())
        h.update(b"" if a is None else a.tobytes())
    h.update(repr((cap, int(dims.nefc_max), tuple(precisions))).encode())
    key = h.hexdigest()
    if key in _PASSES:
        return _PASSES[key]
    out, nbody = {}, int(dims.nbody)
    for p in precisions:
        o = oracle_mod.Oracle(blob, p)
        o.set_ncon_cap(cap)
        get = lambda k, *shape: o.get(k, max(1, int(np.prod(shape)))).reshape(shape)     # (Oracle.get zeroes `cap` doubles per call)
        rows = []
        for e in range(len(qpos)):
            w = np.zeros(nv) if warm is None else warm[e].astype(np.float64)
            o.forward(qpos[e].astype(np.float64), qvel[e].astype(np.float64), ctrl[e], w, step=False)
            nefc, ne, nf, ncon = (int(x) for x in get("counts", 6)[:4])
            r = {k: get(k, nv) for k in _PER_DOF}
            r.update({k: get(k, nefc) for k in _PER_ROW})
            f = np.zeros(int(dims.nefc_max))
            f[:nefc] = get("efc_force", nefc)
            r.update(efc_force=f, efc_J=get("efc_J", nefc, nv), M=get("M", nv, nv), contacts=get("contacts", ncon, 10),
                     xpos=get("xpos", nbody, 3), xmat=get("xmat", nbody, 3, 3))
            for a in r.values():
                a.flags.writeable = False
            r.update(nefc=nefc, ne=ne, nf=nf, ncon=ncon)
            rows.append(r)
        out[p] = rows
    _PASSES[key] = out
    return out


def stacked(rows, names):
    """{name: [n, w]} of one precision's per-env list (M flattened row by row, a count as one column)"""
    return {k: np.stack([np.asarray(r[k], np.float64).reshape(-1) for r in rows]) for k in names}


# ---- the row law at a given acceleration (what Physics.inverse evaluates), on the oracle's rows

def row_forces(r, a, dt):
    """efc_force at acceleration a in arithmetic dt: x = J a - aref; equality rows -D x; friction-loss rows -D x, clamped to
    +-floss outside |x| < R floss; limit and contact rows -D min(x, 0)"""
    J, aref, D, R, fl = (r[k].astype(dt) for k in ("efc_J", "efc_aref", "efc_D", "efc_R", "efc_floss"))
    x = (J @ a.astype(dt) - aref).astype(dt)
    f = (-D * x).astype(dt)
    ne, nf = r["ne"], r["nf"]
    fr = slice(ne, ne + nf)
    rf = (R[fr] * fl[fr]).astype(dt)
    f[fr] = np.where(x[fr] <= -rf, fl[fr], np.where(x[fr] >= rf, -fl[fr], f[fr]))
    f[ne + nf:] = (-D[ne + nf:] * np.minimum(x[ne + nf:], 0)).astype(dt)
    return f


def inverse_ref(r, a, dt, nefc_max):
    """the four checked outputs at acceleration a from oracle env r, in arithmetic dt"""
    f = row_forces(r, a, dt)
    qfc = (r["efc_J"].astype(dt).T @ f).astype(dt)
    a = a.astype(dt)
    qfi = ((r["M"].astype(dt) @ a).astype(dt) + r["qfrc_bias"].astype(dt) - r["qfrc_passive"].astype(dt) - qfc).astype(dt)
    pad = np.zeros(nefc_max, dt)
    pad[:len(f)] = f
    return dict(efc_force=pad, qfrc_constraint=qfc, qfrc_actuator=r["qfrc_actuator"].astype(dt), qfrc_inverse=qfi)


def inverse_inputs(ref64, seed):
    """the three accelerations of the inverse parity tests, fp32 [n, nv]: the f64 oracle's own qacc, that plus seeded noise of scale
    0.3 max(1, |qacc|_inf), zeros"""
    own = np.stack([r["qacc"] for r in ref64]).astype(np.float32)
    rng = np.random.default_rng(seed)
    scale = 0.3 * np.maximum(1.0, np.abs(own).max(1, keepdims=True))
    noisy = (own + scale * rng.normal(size=own.shape)).astype(np.float32)
    return dict(own=own, noisy=noisy, zeros=np.zeros_like(own))


# ---- row counts, the exclusion, contact wrenches from the oracle's rows

def npyr(env):
    """pyramid edges per contact: 2 (condim - 1), one condim per model"""
    condim = np.unique(env.sys.arrays["pair_condim"])
    assert len(condim) == 1
    return 2 * (int(condim[0]) - 1)


def counts_of(rows, npyr):
    """[n, 4] (ne, nf, nl, ncon) of oracle_pass's per-env list"""
    return np.array([[r["ne"], r["nf"], r["nefc"] - r["ne"] - r["nf"] - npyr * r["ncon"], r["ncon"]] for r in rows])


def keep(kind, hip_counts, ref, npyr):
    """envs whose (ne, nf, nl, ncon) agree between the kernel (hip_counts [n, 4]), the f64 oracle and the f32 oracle; asserts the
    2 % condition"""
    hip = np.asarray(hip_counts)
    c64, c32 = counts_of(ref["f64"], npyr), counts_of(ref["f32"], npyr)
    flips = (hip != c64).any(1) | (c32 != c64).any(1)
    print(kind, "excluded envs: %d of %d (kernel vs f64 %d, f32 vs f64 %d)"
          % (flips.sum(), len(hip), (hip != c64).any(1).sum(), (c32 != c64).any(1).sum()))
    assert flips.mean() <= 0.02, f"{kind}: row counts differ in {flips.sum()} of {len(hip)} envs"
    return ~flips


def keep_inverse(kind, phys, ref, npyr):
    """keep on the counts of the last inverse()"""
    hc = phys.inverse_efc_counts.cpu().numpy().astype(int)
    ncon = hc[:, 0] - hc[:, 1] - hc[:, 2] - hc[:, 3]
    assert (ncon % npyr == 0).all() and (ncon >= 0).all()
    return keep(kind, np.stack([hc[:, 1], hc[:, 2], hc[:, 3], ncon // npyr], 1), ref, npyr)


def contact_order_check(kind, A, geom1, geom2, ref, kept):
    """the kept envs list their contacts (geom1 / geom2 [n, K] of the kernel) in the order of both oracles"""
    for e in np.nonzero(kept)[0]:
        for p in ("f32", "f64"):
            pr = ref[p][e]["contacts"][:, 9].astype(int)
            nc = len(pr)
            assert (geom1[e, :nc] == A["pair_geom1"][pr]).all() and (geom2[e, :nc] == A["pair_geom2"][pr]).all(), (kind, e, "contact order")


def keep_constraint(kind, phys, ref, npyr):
    """keep and contact_order_check on the counts and contacts of the last constraint_forces()"""
    hc = phys.efc_counts.cpu().numpy().astype(int)
    cf = phys.contact_forces()
    hip = np.stack([hc[:, 1], hc[:, 2], hc[:, 3], cf["ncon"].cpu().numpy()], 1)
    assert (hc[:, 0] == hip[:, 0] + hip[:, 1] + hip[:, 2] + npyr * hip[:, 3]).all()
    kept = keep(kind, hip, ref, npyr)
    contact_order_check(kind, phys.env.sys.arrays, cf["geom1"].cpu().numpy(), cf["geom2"].cpu().numpy(), ref, kept)
    return kept


def free_trees(A):
    """{root body: first dof} of the kinematic trees that hang on a free joint"""
    return {int(A["jnt_bodyid"][j]): int(A["jnt_dofadr"][j]) for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) == 0}


def ref_wrench(r, A, npyr, ncon_max):
    """The force and torque (about the root body's origin, in its frame) that each contact of oracle env `r` puts on a free-jointed
    tree, from the oracle's own rows: sum over the contact's pyramid rows of efc_J[row, d:d+3] f and efc_J[row, d+3:d+6] f (d: the
    tree's free joint).  Returns force [ncon_max, 2, 3], torque [ncon_max, 2, 3] (index 1: the side, 0 = body1's tree,
    1 = body2's), on [ncon_max, 2] (the side's tree is free-jointed) and root [ncon_max, 2]."""
    free = free_trees(A)
    F, T = np.zeros((ncon_max, 2, 3)), np.zeros((ncon_max, 2, 3))
    on, root = np.zeros((ncon_max, 2), bool), np.zeros((ncon_max, 2), int)
    rcon = r["nefc"] - npyr * r["ncon"]
    for c in range(r["ncon"]):
        rows = slice(rcon + npyr * c, rcon + npyr * (c + 1))
        f = r["efc_force"][rows]
        for side in (0, 1):
            rb = int(A["body_rootid"][int(r["contacts"][c, 7 + side])])
            if rb in free:
                d = free[rb]
                # a tree on both sides of one contact would put both sides' columns in the same dofs
                other = int(A["body_rootid"][int(r["contacts"][c, 8 - side])])
                assert other != rb
                on[c, side], root[c, side] = True, rb
                F[c, side] = f @ r["efc_J"][rows, d:d + 3]
                T[c, side] = f @ r["efc_J"][rows, d + 3:d + 6]
    return F, T, on, root


def wrench_on_root(pos, force, torque, r, root, sign):
    """R_root^T [(pos - xpos_root) x F + tau] with F = sign * force, tau = sign * torque: the generalised force a wrench at `pos`
    puts on a free joint's rotational dofs (they are expressed in the body frame)"""
    Fw, tw = sign * np.asarray(force, np.float64), sign * np.asarray(torque, np.float64)
    return r["xmat"][root].T @ (np.cross(np.asarray(pos, np.float64) - r["xpos"][root], Fw) + tw)


def closure_residual(F_sum, qfc_lin):
    """per env: |sum of the contact forces on the tree - qfrc_constraint[d:d+3]| / max(1, |qfrc_constraint[d:d+3]|_inf)"""
    return rel(F_sum, qfc_lin)


# ---- everything a Physics handle owns and shares

ALL_BUFFERS = ("record", "side", "applied", "dynamics", "constraint", "transition", "inverse")


def handle_views(phys, buffer):
    """{field: live view} of one of ALL_BUFFERS: the env's record; the side buffer (sensordata included); xfrc / qfrc while applied
    forces are on; the dynamics, constraint and inverse buffers; the transition buffer's columns and, once fd_x / fd_y were read (the
    keep_states tests), the two halves of its states buffer.  Fetching a view makes the library allocate its buffer, zeroed, on first use.  The one
    place in tests/ that names Physics's private view accessors."""
    if buffer == "record":
        return {"": phys.env.record}
    if buffer == "side":
        return dict(phys._side)
    if buffer == "applied":
        return {} if phys.xfrc_applied is None else dict(xfrc=phys.xfrc_applied, qfrc=phys.qfrc_applied)
    if buffer == "dynamics":
        return dict(phys._dyn_views())
    if buffer == "constraint":
        return dict(phys._con_views())
    if buffer == "transition":
        return {name: phys._fd_view(name) for name in ["columns"] + [s for s in ("states_x", "states_y") if s in phys._fd]}
    assert buffer == "inverse", buffer
    return dict(phys._inv_views())


_PREFIX = dict(record="record", side="side_", applied="applied_", dynamics="dyn_", constraint="con_", transition="fd_", inverse="inv_")


def all_but(*own):
    """ALL_BUFFERS but an op's own outputs"""
    assert set(own) <= set(ALL_BUFFERS)
    return tuple(b for b in ALL_BUFFERS if b not in own)


def handle_snapshot(phys, buffers=ALL_BUFFERS):
    """{name: clone} of every field of `buffers`: "record", "side_qacc", "dyn_qM", "con_efc_force", "fd_columns", "inv_qacc", ..."""
    import torch
    torch.cuda.synchronize()
    return {_PREFIX[b] + k: v.clone() for b in buffers for k, v in handle_views(phys, b).items()}


def assert_unchanged(before, after, except_=()):
    """every field of `before` is in `after`, bit for bit, but those whose name starts with one of `except_`"""
    for k, v in before.items():
        if not any(k.startswith(x) for x in except_):
            assert_bitwise(k, after[k], v)
