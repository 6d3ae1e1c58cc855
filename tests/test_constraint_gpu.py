"""Physics.constraint_forces / Physics.contact_forces (rsr_physics_constraint, csrc/physics/rsr_constraint.hpp) on every built
family: efc_force, qfrc_constraint and qacc against the CPU oracle, the contact wrench against the oracle's Jacobian rows, sign and
closure on the device alone, consistency with dynamics(), bit identity with forward(), no side effects, the Go2 warm start.

States: random_states(envdef, kind, 256, 11), the states of test_physics_gpu's forward test, DR off.  Errors, the rule and the
exclusion of envs whose row counts flip: tests/physics_support.py.  On the CPU, with the oracle's own reset states for seed 11 and
the same perturbation, the fp32-vs-fp64 part of that excludes 0 (cube), 0 (tshape), 0 (go2flat), 0 (go2rough) and 0 (footstand) of
256 envs, so seed 11 stays.

Contact slots: the kernel and the oracle list the contacts of an env in the same order (geom pair by geom pair); the tests check
that on the geom ids of every kept env rather than assume it."""
import numpy as np
import pytest

from physics_support import (FAMILIES, GO2, PIPE, all_but, assert_unchanged, bits, closure_residual, free_trees, handle_snapshot,
                             handle_views, keep_constraint, make, oracle_pass, ref_wrench, rel, rule, setup, wrench_on_root)
from physics_support import npyr as npyr_of
from rsr_mjx_amd import prng

N = 256


def _ref(oracle_mod, E, qpos, qvel, ctrl, blob=None):
    return oracle_pass(oracle_mod, blob or E.blob, E.dims, qpos, qvel, ctrl)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_constraint_forces_match_the_oracle(oracle_mod, kind):
    """efc_force, qfrc_constraint and constraint_qacc after set_state + constraint_forces() against Oracle.forward(q, v, ctrl,
    zeros) in f64, under the module's rule and exclusion.  set_state's forward pass leaves its qacc in qacc_warmstart; the oracle
    is given zeros, so the record's warm start is zeroed before the call (the Go2 solve is one Newton iteration: the start
    matters, and the two sides must start alike)."""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = setup(kind)
    assert float(phys.efc_force.abs().max()) == 0.0 and float(phys.contact_forces()["force"].abs().max()) == 0.0      # zeros until the first call
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.qacc_warmstart.zero_()                                    # (set_state leaves the forward pass's qacc there)
    phys.constraint_forces()
    torch.cuda.synchronize()
    d = E.dims
    assert phys.efc_force.shape == (N, d.nefc_max) and phys.qfrc_constraint.shape == (N, d.nv)
    assert phys.efc_counts.shape == (N, 4) and phys.constraint_qacc.shape == (N, d.nv)
    ref = _ref(oracle_mod, E, qpos, qvel, ctrl)
    npyr = npyr_of(E)
    keep = keep_constraint(kind, phys, ref, npyr)
    hip = dict(efc_force=phys.efc_force, qfrc_constraint=phys.qfrc_constraint, qacc=phys.constraint_qacc)
    fails = []
    for f, t in hip.items():
        h = t.cpu().numpy().astype(np.float64)
        r64, r32 = (np.stack([r[f] for r in ref[p]]) for p in ("f64", "f32"))
        rule(kind, f, rel(h, r64)[keep], rel(r32, r64)[keep], fails)
    # rows >= nefc are zero
    nefc = phys.efc_counts[:, 0].cpu().numpy().astype(int)
    ef = phys.efc_force.cpu().numpy()
    assert all((ef[e, nefc[e]:] == 0).all() for e in range(N))
    assert np.abs(ef).max() > 1.0, "no constraint force anywhere: the test shows nothing"
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_contact_wrench_matches_the_oracle_rows(oracle_mod, kind):
    """Every contact on a free-jointed tree (the Go2; the Airbot's cube / T block): the force on the tree from the f64 oracle's
    rows, sum_e efc_J[r_e, d:d+3] efc_force[r_e] (d: the tree's free joint, r_e: the contact's pyramid rows), against +-force by
    the side the tree is on; and sum_e efc_J[r_e, d+3:d+6] efc_force[r_e] against R_root^T [(pos - xpos_root) x force + torque]
    (free-joint rotational dofs are expressed in the body frame; root: the body of the free joint, xpos / xmat the f64 oracle's).
    On the f64 oracle's own rows that torque form holds to rounding (CPU, these states: the part of R J_rot - (pos - xpos) x J_lin
    across the normal is <= 4e-16 on every pyramid row of all five families, and the whole of it on the rows without torsion), so
    the form stands as given.  Both under the module's rule per env, the f32 oracle's wrench formed the same way as the spread.
    (The rough-terrain Go2 spawns clear of the ground: a handful of contacts in 256 envs, all of them checked.)  normal_force >= 0 and equal to the sum of the contact's edge forces (summed in pairs, as the kernel folds
    them) to 1 ulp; slots >= ncon are zero."""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = setup(kind)
    A = envdef.sys.arrays
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.qacc_warmstart.zero_()
    phys.constraint_forces()
    torch.cuda.synchronize()
    ref = _ref(oracle_mod, E, qpos, qvel, ctrl)
    npyr, K = npyr_of(E), E.dims.ncon_max
    keep = keep_constraint(kind, phys, ref, npyr)
    cf = {k: v.cpu().numpy() for k, v in phys.contact_forces().items()}
    assert cf["force"].shape == (N, K, 3) and cf["torque"].shape == (N, K, 3) and cf["normal_force"].shape == (N, K)
    refF, refT = ({p: np.zeros((N, K, 2, 3)) for p in ("f32", "f64")} for _ in range(2))
    hipF, hipT = np.zeros((N, K, 2, 3)), np.zeros((N, K, 2, 3))
    seen = 0
    for e in np.nonzero(keep)[0]:
        for p in ("f32", "f64"):
            refF[p][e], refT[p][e], on, root = ref_wrench(ref[p][e], A, npyr, K)
        for c, side in zip(*np.nonzero(on)):                  # (the f64 oracle's)
            sign = 1.0 if side == 1 else -1.0
            hipF[e, c, side] = sign * cf["force"][e, c]
            hipT[e, c, side] = wrench_on_root(cf["pos"][e, c], cf["force"][e, c], cf["torque"][e, c], ref["f64"][e], root[c, side], sign)
            seen += 1
    print(kind, "contacts on free-jointed trees:", seen)
    assert seen > (0 if kind == "go2rough" else N // 4), f"{kind}: only {seen} contacts on free-jointed trees"
    fails = []
    rule(kind, "contact force", rel(hipF, refF["f64"])[keep], rel(refF["f32"], refF["f64"])[keep], fails)
    rule(kind, "contact torque on the root", rel(hipT, refT["f64"])[keep], rel(refT["f32"], refT["f64"])[keep], fails)
    # the normal force: non-negative, the sum of the edges; empty slots zero
    ncon = cf["ncon"]
    hc = phys.efc_counts.cpu().numpy().astype(int)
    ef = phys.efc_force.cpu().numpy()
    assert (cf["normal_force"] >= 0).all()
    for e in range(N):
        rcon = hc[e, 0] - npyr * ncon[e]
        edges = ef[e, rcon:rcon + npyr * ncon[e]].reshape(ncon[e], npyr)
        s = np.zeros(ncon[e], np.float32)
        for k in range(0, npyr, 2):
            s = (s + (edges[:, k] + edges[:, k + 1]).astype(np.float32)).astype(np.float32)
        assert (np.abs(cf["normal_force"][e, :ncon[e]] - s) <= np.spacing(s)).all(), (kind, e)
        for f in ("normal_force", "force", "torque", "dist", "pos", "normal"):
            assert (cf[f][e, ncon[e]:] == 0).all(), (kind, e, f)
        assert (cf["geom1"][e, ncon[e]:] == -1).all()
    if npyr == 4:
        assert (cf["torque"] == 0).all()                     # condim 3: no torsional row
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_contact_forces_close_on_the_free_joint(oracle_mod, kind):
    """Device alone: the translation dofs of a free joint are in the world frame and no row but the contacts of its tree touches
    them, so qfrc_constraint[d:d+3] must equal the sum over the tree's contacts of +-force (the side sign).  Go2: dofs 0..2, every
    contact, sign + where the ground is geom1.  Airbot: the dofs of the cube / T block.  The bound is the residual of the same
    identity on the f32 oracle for these states -- sum over rows of efc_J[r, d:d+3] efc_force[r] summed per contact and then over
    contacts in fp32, against its fp32 qfrc_constraint[d:d+3] -- times 3 on the p99 (the project's margin), 20 on every env, floors
    1e-5 / 1e-4 as in the module's rule.  Measured on the CPU (oracle reset states): the f32 oracle's residual is p99 <= 2.2e-7,
    max <= 2.4e-7 on all five families, so the floors decide: p99 <= 1e-5, every env <= 1e-4.  No env is excluded: both sides are the
    kernel's.  And on a standing pose of the Go2 models whose ground is a plane (geom1 of every pair), every contact force points
    up.  The standing pose is the env's reset state at rest: the home keyframe at the reset's random place and heading, qvel zero,
    position targets equal to the joint angles, so that the actuators hold the pose and every foot bears load.  (The random states
    above do not stand: their ctrl is drawn over the whole control range, the legs are pulled off the ground, and the oracle
    itself, f32 and f64, leaves 361 of 994 (flat) and 673 of 1252 (footstand) listed contacts without force there.  On the
    standing pose the f64 and f32 oracles load all 4 x 256 contacts, CPU, set_state's pass and then this one.)"""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = setup(kind)
    A = envdef.sys.arrays
    free = free_trees(A)
    stand_qpos, stand_ctrl = phys.qpos.clone(), phys.ctrl.clone()   # the reset state, before the random states overwrite it
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.constraint_forces()
    torch.cuda.synchronize()
    cf = {k: v.cpu().numpy() for k, v in phys.contact_forces().items()}
    qfc = phys.qfrc_constraint.cpu().numpy()
    ref32 = _ref(oracle_mod, E, qpos, qvel, ctrl)["f32"]
    npyr, K = npyr_of(E), E.dims.ncon_max
    geom_root = A["body_rootid"][A["geom_bodyid"]]
    fails, total = [], 0
    for rb, d in sorted(free.items()):
        s1 = (cf["geom1"] >= 0) & (geom_root[np.maximum(cf["geom1"], 0)] == rb)
        s2 = (cf["geom2"] >= 0) & (geom_root[np.maximum(cf["geom2"], 0)] == rb)
        assert not (s1 & s2).any()
        sign = s2.astype(np.float32) - s1.astype(np.float32)
        total += int((sign != 0).sum())
        Fsum = (sign[:, :, None] * cf["force"]).astype(np.float32).sum(1, dtype=np.float32)
        err = closure_residual(Fsum, qfc[:, d:d + 3])
        # the f32 oracle's residual of the same identity, in fp32
        spread = np.zeros(N)
        for e in range(N):
            F, _, on, root = ref_wrench(ref32[e], A, npyr, K)
            per = (F[:, 1] * (on[:, 1] & (root[:, 1] == rb))[:, None] + F[:, 0] * (on[:, 0] & (root[:, 0] == rb))[:, None]).astype(np.float32)
            spread[e] = closure_residual(per.sum(0, dtype=np.float32)[None], ref32[e]["qfrc_constraint"][None, d:d + 3].astype(np.float32))[0]
        rule(kind, f"closure on dofs {d}..{d + 2}", err, spread, fails)
    print(kind, "contacts on free-jointed trees:", total)
    assert total > (0 if kind == "go2rough" else N // 4), f"{kind}: only {total} contacts on free-jointed trees"
    assert not fails, fails
    if kind in ("go2flat", "footstand"):
        # a standing pose: the reset state (home keyframe, position targets = that pose) at rest
        assert float((stand_ctrl - stand_qpos[:, 7:]).abs().max()) < 1e-6
        phys.set_state(qpos=stand_qpos, qvel=np.zeros_like(qvel), ctrl=stand_ctrl)
        phys.constraint_forces()
        torch.cuda.synchronize()
        c2 = {k: v.cpu().numpy() for k, v in phys.contact_forces().items()}
        live = np.arange(K)[None, :] < c2["ncon"][:, None]
        plane1 = live & (A["geom_bodyid"][np.maximum(c2["geom1"], 0)] == 0)
        assert (A["geom_type"][c2["geom1"][live]] == 0).all()         # mjGEOM_PLANE
        assert plane1.sum() > N and (plane1 == live).all()
        assert (c2["force"][..., 2][plane1] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_qacc_follows_from_the_dynamics_terms_and_qfrc_constraint(oracle_mod, kind):
    """Dof friction loss zeroed through the per-env leaf (as test_dynamics_gpu's qacc test does): qM @ constraint_qacc against
    qfrc_passive - qfrc_bias + qfrc_actuator + qfrc_constraint (product in fp64 on the host), both from the kernels.  Rule of the
    module, with the f32 oracle's own residual of the same identity on the same states and model, M qacc against qfrc_smooth +
    qfrc_constraint, as the spread.  No env is excluded: both sides are the kernels'.  The identity holds to the solver's
    convergence, in the oracle as in the kernel.  Measured on the CPU (oracle reset states), the f32 oracle's residual is p99
    2.1e-4 (cube) and 1.9e-2 (T-shape), and 5.8 / 1.1 / 12 on go2flat / go2rough / footstand: the Go2 models run one Newton
    iteration from a zero warm start, which leaves qacc far from the minimiser, so on them the rule bounds little; the bit
    identity with forward() and the oracle parity of qacc and qfrc_constraint are what hold the Go2 kernels."""
    import torch
    from rsr_mjx_amd.model import pack_blob, unpack_blob
    envdef, E, phys, qpos, qvel, ctrl = setup(kind, zero_floss=True)
    nv = E.dims.nv
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.qacc_warmstart.zero_()
    phys.dynamics()
    phys.constraint_forces()
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy().astype(np.float64)
    lhs = np.einsum("nij,nj->ni", g(phys.qM), g(phys.constraint_qacc))
    rhs = g(phys.qfrc_passive) - g(phys.qfrc_bias) + g(phys.qfrc_actuator) + g(phys.qfrc_constraint)
    fields = dict(unpack_blob(E.blob))
    fields["dof_frictionloss"] = np.zeros_like(fields["dof_frictionloss"])
    ref32 = _ref(oracle_mod, E, qpos, qvel, ctrl, blob=pack_blob(fields))["f32"]
    o_lhs = np.stack([r["M"] @ r["qacc"] for r in ref32])
    o_rhs = np.stack([r["qfrc_smooth"] + r["qfrc_constraint"] for r in ref32])
    fails = []
    rule(kind, "M qacc = qfrc_smooth + qfrc_constraint", rel(lhs, rhs), rel(o_lhs, o_rhs), fails)
    assert np.abs(g(phys.qfrc_constraint)).max() > 1.0
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("applied", [False, True])
def test_it_is_the_forward_pass(kind, applied):
    """constraint_forces() then forward() on the same record: constraint_qacc is phys.qacc and the RSR_C_CONTACT / RSR_C_NCON
    views are phys.contacts(), bit for bit; plain, and with applied forces on (non-zero qfrc and xfrc), where qfrc_constraint also
    differs from the plain run."""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = setup(kind)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.step(None, 2)                                             # a warm start that is neither zero nor this pass's qacc
    phys.constraint_forces()
    torch.cuda.synchronize()
    plain = phys.qfrc_constraint.clone()
    if applied:
        g = torch.Generator(device="cpu").manual_seed(3)
        mass = torch.as_tensor(envdef.sys.arrays["body_mass"], dtype=torch.float32)
        x = torch.randn((N, E.dims.nbody, 6), generator=g) * 0.5 * 9.81 * mass[None, :, None].clamp(min=0.05)
        q = torch.randn((N, E.dims.nv), generator=g) * 0.5
        phys.set_applied(x, q)
        phys.constraint_forces()
        torch.cuda.synchronize()
        assert not torch.equal(bits(phys.qfrc_constraint), bits(plain))
        assert float((phys.qfrc_constraint - plain).abs().max()) > 1e-3
    cq = phys.constraint_qacc.clone()
    cv = handle_snapshot(phys, ("constraint",))
    phys.forward()
    torch.cuda.synchronize()
    bad = (bits(cq) != bits(phys.qacc)).any(1)
    assert not bool(bad.any()), f"{kind}: qacc differs in {int(bad.sum())} envs, max |d| {float((cq - phys.qacc).abs().max()):.3e}"
    side = handle_views(phys, "side")
    assert torch.equal(bits(cv["con_contact"]), bits(side["contact"]))
    assert torch.equal(bits(cv["con_ncon"]), bits(side["ncon"]))
    assert float(cv["con_ncon"].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_constraint_forces_has_no_side_effects(kind):
    import torch
    from rsr_mjx_amd.physics import Physics
    envdef, E, _, scale = make(kind, N, kind != "tshape")
    _, F, _, _ = make(kind, N, kind != "tshape")
    E.reset(prng.split(prng.PRNGKey(4), N))
    F.reset(prng.split(prng.PRNGKey(4), N))
    rng = np.random.default_rng(0)
    act = lambda: np.clip(rng.normal(size=(N, E.dims.nu)) * scale, -1, 1).astype(np.float32)
    a0 = act()
    E.step(None, a0)
    F.step(None, a0)
    phys = Physics(E, sensors=[("lin", "framelinvel", "endpoint" if kind in ("cube", "tshape") else "imu")])
    phys.step(None, 1)
    phys.dynamics()
    torch.cuda.synchronize()
    before = handle_snapshot(phys, all_but("constraint"))
    rec0 = before["record"]
    phys.constraint_forces()
    # the record (the warm start included), the side buffer, sensordata, the dynamics buffer and every other buffer of the handle
    # are bitwise as before
    assert_unchanged(before, handle_snapshot(phys, all_but("constraint")))
    views = handle_views(phys, "constraint")
    first = {k: v.clone() for k, v in views.items()}
    assert all(float(first[k].abs().max()) > 0 for k in ("qfrc_constraint", "qacc", "efc_counts", "efc_force"))
    # env_ids: the other envs' rows keep a sentinel, the listed rows get the full call's values
    for v in views.values():
        v.fill_(7.25)
    ids = np.array([3, 17, 64, 100, N - 1])
    phys.constraint_forces(env_ids=ids)
    torch.cuda.synchronize()
    others = np.setdiff1d(np.arange(N), ids)
    for k, v in views.items():
        assert bool((v[others] == 7.25).all()), k
        assert torch.equal(bits(v[ids]), bits(first[k][ids])), k
    with pytest.raises(ValueError):
        phys.constraint_forces(env_ids=[N])
    with pytest.raises(ValueError):
        phys.constraint_forces(env_ids=[1, 1])
    from rsr_mjx_amd import _lib
    bad = np.ones(2, np.int32)
    assert _lib.lib().rsr_physics_constraint(phys._h, bad.ctypes.data, 0, None) == -1          # env_ids with count < 1
    import ctypes as C
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    for fid in (-1, len(_lib.CONSTRAINT_FIELDS)):
        assert _lib.lib().rsr_physics_constraint_view(phys._h, fid, C.byref(ptr), shape, stride) == -1
    assert torch.equal(bits(E.record), bits(rec0))
    # an env.step after constraint_forces() equals the same step without it (F: the same history, no physics handle)
    F.record.copy_(rec0)
    a1 = act()
    E.step(None, a1)
    F.step(None, a1)
    torch.cuda.synchronize()
    for k in PIPE + ("obs", "reward", "done"):
        assert torch.equal(bits(E.view(k)), bits(F.view(k))), k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", GO2)
def test_go2_constraint_forces_read_the_warm_start_and_leave_it(kind):
    """The Go2 solve is one Newton iteration from the cheaper of qacc_warmstart and qacc_smooth, so the warm start decides the
    result: after phys.step the call must read the record's qacc_warmstart (constraint_qacc differs from a run on the same state
    with the warm start zeroed), leave it as it was, and give identical outputs when called twice.  The start can matter only
    where a foot touches: an env without a contact has the friction-loss rows alone, and there the oracle, f32 and f64, returns
    the same qacc from either start.  So the count is taken over the envs with a contact, and more than half of those must
    differ.  On the CPU oracle, these states after two steps: 255 of 256 (flat), 251 of 256 (footstand) and 58 of the 59 envs
    with a contact (rough terrain, where the robots spawn clear of the ground; none of the other 197 differs)."""
    import torch
    envdef, E, phys, qpos, qvel, ctrl = setup(kind)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.step(None, 2)
    torch.cuda.synchronize()
    warm0 = phys.qacc_warmstart.clone()
    assert float(warm0.abs().max()) > 0
    phys.constraint_forces()
    torch.cuda.synchronize()
    first = handle_snapshot(phys, ("constraint",))
    assert torch.equal(bits(phys.qacc_warmstart), bits(warm0))
    phys.constraint_forces()
    assert_unchanged(first, handle_snapshot(phys, ("constraint",)))
    phys.qacc_warmstart.zero_()
    phys.constraint_forces()
    torch.cuda.synchronize()
    differ = (bits(phys.constraint_qacc) != bits(first["con_qacc"])).any(1)
    touching = first["con_ncon"].reshape(N) > 0
    print(kind, "constraint_qacc depends on the warm start in %d of %d envs, %d of the %d with a contact"
          % (int(differ.sum()), N, int((differ & touching).sum()), int(touching.sum())))
    assert int(touching.sum()) > 0
    assert int((differ & touching).sum()) > int(touching.sum()) // 2
    assert float(phys.qacc_warmstart.abs().max()) == 0.0
