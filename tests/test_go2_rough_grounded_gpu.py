"""The physics layer on rough-terrain Go2 states that STAND ON THE TERRAIN (tests/golden/go2_rough_grounded_states.npz, written by
tests/golden/make_go2_rough_grounded.py with the fp64 oracle): the states the other physics-layer modules draw for this family come
from the reset distribution, where the robots spawn clear of the ground (59 of 256 envs with any contact), and those modules lower
their bars for it.  Here every env has contacts with the height field, and the bars are the other families'.

On the CPU the f64 oracle lists >= 3 contacts in 256 of the 256 envs (815 contacts in all), and the f32 and f64 oracles disagree on
(ne, nf, nl, ncon) in 0 of them; every one of the 815 contacts carries a normal force > 0 in the f64 oracle (the generator sees to
that; on the device the smallest force along its normal is 2.29 N).

Errors, rule and exclusion: tests/physics_support.py, as in test_constraint_gpu."""
import os

import numpy as np
import pytest

from physics_support import closure_residual, keep_constraint, make, npyr, oracle_pass, ref_wrench, rel, rule, wrench_on_root
from rsr_mjx_amd import prng

pytestmark = pytest.mark.gpu

KIND = "go2rough"
N = 256


def _states():
    a = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "go2_rough_grounded_states.npz"))
    assert a["qpos"].shape[0] == N and a["qpos"].dtype == np.float32
    return a["qpos"], a["qvel"], a["ctrl"]


def _setup():
    from rsr_mjx_amd.physics import Physics
    envdef, E, _, _ = make(KIND, N, False)
    E.reset(prng.split(prng.PRNGKey(1), N))
    return (envdef, E, Physics(E)) + _states()


def _ref(oracle_mod, E, qpos, qvel, ctrl):
    return oracle_pass(oracle_mod, E.blob, E.dims, qpos, qvel, ctrl)


def test_contacts_on_grounded_states(oracle_mod):
    """phys.contacts() after set_state: ncon, the geom ids in the oracle's order, and dist, pos, normal per slot against the f64
    oracle on the kept envs, f32 oracle as spread; more than 3 N 0.8 contacts in all."""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = _setup()
    A = envdef.sys.arrays
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    torch.cuda.synchronize()
    c = {k: v.cpu().numpy() for k, v in phys.contacts().items()}
    phys.qacc_warmstart.zero_()
    phys.constraint_forces()                                   # (for keep_constraint: the row counts; it leaves the contacts of the pass alone)
    torch.cuda.synchronize()
    ref = _ref(oracle_mod, E, qpos, qvel, ctrl)
    keep = keep_constraint(KIND, phys, ref, npyr(E))
    K = E.dims.ncon_max
    pad = {p: {f: np.zeros((N, K, w)) for f, w in (("dist", 1), ("pos", 3), ("normal", 3))} for p in ("f32", "f64")}
    for e in np.nonzero(keep)[0]:
        r = ref["f64"][e]
        nc = r["ncon"]
        pair = r["contacts"][:, 9].astype(int)
        assert c["ncon"][e] == nc and (c["geom1"][e, :nc] == A["pair_geom1"][pair]).all() and (c["geom2"][e, :nc] == A["pair_geom2"][pair]).all(), e
        assert (c["geom1"][e, nc:] == -1).all()
        for p in ("f32", "f64"):
            rc = ref[p][e]["contacts"]
            pad[p]["dist"][e, :nc, 0], pad[p]["pos"][e, :nc], pad[p]["normal"][e, :nc] = rc[:, 0], rc[:, 1:4], rc[:, 4:7]
    total = int(c["ncon"][keep].sum())
    print(KIND, "grounded: contacts on the kept envs:", total, "envs with >= 3:", int((c["ncon"] >= 3).sum()))
    assert total > 3 * N * 0.8
    fails = []
    for f in ("dist", "pos", "normal"):
        rule(KIND, "contact " + f, rel(c[f].reshape(N, -1), pad["f64"][f])[keep], rel(pad["f32"][f], pad["f64"][f])[keep], fails)
    assert not fails, fails


def test_forces_on_grounded_states(oracle_mod):
    """constraint_forces() / contact_forces(): efc_force, qfrc_constraint, constraint_qacc against the f64 oracle; the contact wrench
    on the trunk's free joint against the oracle's rows; closure on dofs 0..2 (bound: the f32 oracle's residual of the same identity,
    as test_constraint_gpu); every contact force has a positive component along its own contact normal.  The checks of
    test_constraint_gpu, with seen > N."""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = _setup()
    A = envdef.sys.arrays
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.qacc_warmstart.zero_()
    phys.constraint_forces()
    torch.cuda.synchronize()
    ref = _ref(oracle_mod, E, qpos, qvel, ctrl)
    edges, K = npyr(E), E.dims.ncon_max
    keep = keep_constraint(KIND, phys, ref, edges)
    fails = []
    for f, t in dict(efc_force=phys.efc_force, qfrc_constraint=phys.qfrc_constraint, qacc=phys.constraint_qacc).items():
        h = t.cpu().numpy().astype(np.float64)
        r64, r32 = (np.stack([r[f] for r in ref[p]]) for p in ("f64", "f32"))
        rule(KIND, f, rel(h, r64)[keep], rel(r32, r64)[keep], fails)
    cf = {k: v.cpu().numpy() for k, v in phys.contact_forces().items()}
    refF, refT = ({p: np.zeros((N, K, 2, 3)) for p in ("f32", "f64")} for _ in range(2))
    hipF, hipT = np.zeros((N, K, 2, 3)), np.zeros((N, K, 2, 3))
    seen = 0
    for e in np.nonzero(keep)[0]:
        for p in ("f32", "f64"):
            refF[p][e], refT[p][e], on, root = ref_wrench(ref[p][e], A, edges, K)
        for cc, side in zip(*np.nonzero(on)):
            sign = 1.0 if side == 1 else -1.0
            hipF[e, cc, side] = sign * cf["force"][e, cc]
            hipT[e, cc, side] = wrench_on_root(cf["pos"][e, cc], cf["force"][e, cc], cf["torque"][e, cc], ref["f64"][e], root[cc, side], sign)
            seen += 1
    print(KIND, "grounded: contacts on the trunk's tree:", seen)
    assert seen > N
    rule(KIND, "contact force", rel(hipF, refF["f64"])[keep], rel(refF["f32"], refF["f64"])[keep], fails)
    rule(KIND, "contact torque on the root", rel(hipT, refT["f64"])[keep], rel(refT["f32"], refT["f64"])[keep], fails)
    # closure on dofs 0..2: the field is geom1 of every pair, so the sum of the contact forces is qfrc_constraint[0:3]
    live = np.arange(K)[None, :] < cf["ncon"][:, None]
    assert (A["geom_bodyid"][cf["geom1"][live]] == 0).all()
    Fsum = (live[:, :, None] * cf["force"]).astype(np.float32).sum(1, dtype=np.float32)
    qfc = phys.qfrc_constraint.cpu().numpy()
    spread = np.zeros(N)
    for e in range(N):
        F, _, on, _ = ref_wrench(ref["f32"][e], A, edges, K)
        per = (F[:, 1] * on[:, 1][:, None]).astype(np.float32)
        spread[e] = closure_residual(per.sum(0, dtype=np.float32)[None], ref["f32"][e]["qfrc_constraint"][None, 0:3].astype(np.float32))[0]
    rule(KIND, "closure on dofs 0..2", closure_residual(Fsum, qfc[:, 0:3]), spread, fails)
    along = np.einsum("nkc,nkc->nk", cf["force"], cf["normal"])
    print(KIND, "grounded: smallest contact force along its normal %.3e" % along[live].min())
    assert (along[live] > 0).all(), f"{(along[live] <= 0).sum()} contacts without a force along their normal"
    assert (cf["normal_force"][live] > 0).all()
    assert not fails, fails


def test_step_from_grounded_states(oracle_mod):
    """phys.step(None, n_substeps) from these states: qpos, qvel, qacc against the oracle's substeps (each warm-started from the
    previous pass's qacc, as test_physics_oracle_parity does), under that test's rule; contact-mode flips counted, at most 2 %."""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = _setup()
    nf = phys.n_substeps
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.step(None, nf)
    torch.cuda.synchronize()
    fields = ("qpos", "qvel", "qacc")
    hip = {f: getattr(phys, f).cpu().numpy().reshape(N, -1) for f in fields}
    ref = {p: {f: np.zeros_like(hip[f], dtype=np.float64) for f in fields} for p in ("f32", "f64")}
    ncon = {p: np.zeros(N, int) for p in ("f32", "f64")}
    for p in ("f32", "f64"):
        o = oracle_mod.Oracle(E.blob, p)
        o.set_ncon_cap(E.dims.ncon_max)
        for e in range(N):
            q, v = qpos[e].astype(np.float64), qvel[e].astype(np.float64)
            o.forward(q, v, ctrl[e], np.zeros(E.dims.nv), step=False)
            for _ in range(nf):
                o.forward(q, v, ctrl[e], o.get("qacc"), step=True)
                q, v = o.get("qpos"), o.get("qvel")
            for f in fields:
                ref[p][f][e] = o.get(f)
            ncon[p][e] = int(o.get("counts")[3])
    flips = (phys.contacts()["ncon"].cpu().numpy() != ncon["f64"]) | (ncon["f32"] != ncon["f64"])
    print(KIND, "grounded step: contact-mode flips in %d of %d envs" % (flips.sum(), N))
    assert flips.mean() <= 0.02
    fails = []
    for f in fields:
        rule(KIND, "stepN " + f, rel(hip[f], ref["f64"][f])[~flips], rel(ref["f32"][f], ref["f64"][f])[~flips], fails)
    assert not fails, fails
