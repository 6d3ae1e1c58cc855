"""Model variants for the constraint-row tests (tests/test_model_variants.py on the CPU, tests/test_model_variants_gpu.py on the
device): edits of envdef.sys.arrays that move the constants every shipped asset agrees on -- solimp power and midpoint, contact
and limit margins, impratio, the friction rule, direct and under-damped solref, refsafe, the equality polynomial -- so that the
branches of kbi / make_constraint / collision (csrc/rsr_device.hpp) and of model.lane_records that no shipped model takes run on
the device and are compared with the CPU oracle, which reads the raw arrays of the blob and never the lane records.

VARIANTS maps a name to (families, edit); apply(envdef, name) edits envdef.sys.arrays before envdef.batched(n) builds the blob
(BatchedEnv.__init__ goes through model_fields, which recomputes lane_rec and pair_incl); blob_of(envdef) builds that blob on the
CPU.  Every edit replaces arrays (never writes into one), keeps their dtype and shape, and changes no dimension: the kernels are
templated on the dimensions and on pair_condim.

States: physics_support.random_states (device) or oracle_states (CPU) of the shipped model, seed 11, then offsets(kind, ...): the
reset states alone leave whole regimes of the impedance curve and the margin band empty (see offsets).  Plain functions; torch is
imported inside them.

SMOOTH_VARIANTS is a second table of the same shape for the smooth side (tests/test_smooth_variants.py on the CPU,
tests/test_smooth_variants_gpu.py on the device): the integrator and eulerdamp, actuator gear, biasprm 0 and 2, the ctrl, force and
joint actuator-force clamps, gravity and armature, which decide branches of smooth_forces, com_crb_mass, integrate and solve
(csrc/rsr_device.hpp, csrc/rsr_solver.hpp) and of discrete_acc (csrc/physics/rsr_inverse.hpp) that no shipped model takes.  Its
states are those above plus smooth_offsets (ctrl outside the control range); per_env_blobs gives the oracle the per-env leaves a
case sets on the device (the zero damping of euler_damped's odd envs, the Go2 randomisation of actuators_dr)."""
import numpy as np

N = 256
SEED = 11

# solimp rows (d0, d_width, width, midpoint, power): a non-integer power with the midpoint off centre, and power 1 (powf(mid, 0)
# = 1, y = x on both sides of the midpoint); the width is set per table below
IMP_A = (0.7, 0.97, None, 0.3, 2.5)
IMP_B = (0.6, 0.95, None, 0.65, 1.0)
PAIR_WIDTH = {4: 0.004, 3: 0.020}      # by the model's condim: the Airbot scenes (box contacts, millimetres deep), the Go2 models
JNT_WIDTH = 0.06            # the limit rows' |pos| comes from the 0.05 rad perturbation of random_states
EQ_WIDTH = 0.05
MARGIN = dict(pair_margin=0.010, pair_gap=0.004, jnt_margin=0.05)
IMPRATIO = 1.5              # the value tests/golden/compiler_pusher.xml uses
DIRECT = (-800.0, -40.0)    # direct solref (stiffness, damping) on limit, friction-loss and equality rows
PAIR_SOLREF = ((0.004, 0.5), (0.03, 2.0))      # 0.004 < 2 dt on every family (dt 0.0025 Airbot, 0.004 Go2): the refsafe clamp decides
EQ_DATA = (0.002, -0.8, 0.3, -0.2, 0.1)


def _set(A, key, value):
    old = np.asarray(A[key])
    new = np.broadcast_to(np.asarray(value, dtype=old.dtype), old.shape).copy()
    A[key] = new


def _alternate(A, key, row_a, row_b):
    """even rows of the table get row_a, odd rows row_b"""
    old = np.asarray(A[key])
    new = old.copy()
    new[0::2] = np.asarray(row_a, dtype=old.dtype)
    new[1::2] = np.asarray(row_b, dtype=old.dtype)
    A[key] = new


def _imp(row, width):
    return [row[0], row[1], width, row[3], row[4]]


def impedance(A, pair_width=None):
    width = pair_width or PAIR_WIDTH[int(np.asarray(A["pair_condim"])[0])]
    _alternate(A, "pair_solimp", _imp(IMP_A, width), _imp(IMP_B, width))
    _alternate(A, "jnt_solimp", _imp(IMP_A, JNT_WIDTH), _imp(IMP_B, JNT_WIDTH))
    _alternate(A, "dof_solimp", _imp(IMP_A, JNT_WIDTH), _imp(IMP_B, JNT_WIDTH))
    _alternate(A, "eq_solimp", _imp(IMP_A, EQ_WIDTH), _imp(IMP_B, EQ_WIDTH))


def margin(A):
    for k, v in MARGIN.items():
        _set(A, k, v)


def impratio(A):
    _set(A, "opt_impratio", IMPRATIO)


def friction_rule(A):
    """geom_friction distinct per geom (sliding in 0.3 .. 1.2, torsional in 0.002 .. 0.05; rolling stays: no model here has a
    rolling row).  geom_priority 1 everywhere but on the geoms that are only ever the second geom of a pair, which cycle through
    0, 2, 1: rule 1 (geom1 wins), 2 (geom2 wins) and 0 (equal: the maximum).  Airbot cube: table - target rule 1, table - cube
    rule 2, finger - table rule 0.  Footstand: the floor against the robot's geoms, a third each."""
    rng = np.random.default_rng(SEED)
    fr = np.asarray(A["geom_friction"]).copy()
    ng = len(fr)
    fr[:, 0] = rng.uniform(0.3, 1.2, ng)
    fr[:, 1] = rng.uniform(0.002, 0.05, ng)
    A["geom_friction"] = fr
    pr = np.ones(ng, dtype=np.asarray(A["geom_priority"]).dtype)
    firsts = set(int(g) for g in A["pair_geom1"])
    for i, g in enumerate(sorted(set(int(g) for g in A["pair_geom2"]) - firsts)):
        pr[g] = (0, 2, 1)[i % 3]
    A["geom_priority"] = pr


def solref(A):
    for k in ("jnt_solref", "dof_solref", "eq_solref"):
        _set(A, k, DIRECT)
    _alternate(A, "pair_solref", PAIR_SOLREF[0], PAIR_SOLREF[1])


def solref_refsafe_off(A):
    solref(A)
    _set(A, "opt_disable_refsafe", 1)


def eq_poly(A):
    _set(A, "eq_data", EQ_DATA)


def combined(A):
    """all of the above (refsafe on); the Airbot pairs' width grows by twice margin - gap: a box contact is kept at dist < 0 only,
    so with a margin every contact row has |pos| > margin - gap, and the narrow width would leave them all at x >= 1"""
    airbot = int(np.asarray(A["pair_condim"])[0]) == 4
    impedance(A, PAIR_WIDTH[4] + 2.0 * (MARGIN["pair_margin"] - MARGIN["pair_gap"]) if airbot else None)
    for edit in (margin, impratio, friction_rule, solref, eq_poly):
        edit(A)


VARIANTS = {
    "impedance": (("cube", "go2flat", "footstand"), impedance),
    "margin": (("cube", "go2flat", "footstand"), margin),
    "impratio": (("cube", "go2flat"), impratio),
    "friction_rule": (("cube", "footstand"), friction_rule),
    "solref": (("cube", "go2flat"), solref),
    "solref_refsafe_off": (("cube", "go2flat"), solref_refsafe_off),
    "eq_poly": (("cube", "tshape"), eq_poly),
    "combined": (("cube", "footstand"), combined),
}
CASES = [(name, kind) for name, (kinds, _) in VARIANTS.items() for kind in kinds]

# ---- the smooth side: constants chosen (the shipped values are in the table of tests/test_smooth_variants.py)
INT_EULER, INT_IMPLICITFAST = 0, 3
GEAR = (1.25, -0.6)         # by actuator in the pattern - + + -: each clamp setting below (which go by u % 2) meets both signs.  The
                            # servo's stiffness on the joint is gear^2 kp, 1.56 and 0.36 times the shipped one.  The Airbot's last
                            # actuator (wrist inertia 8e-5, kp 100, timestep 0.0025: a semi-implicit step is linearly stable for
                            # gear^2 < 0.51, the shipped model leans on its clamps) gets the -0.6
BIAS0 = 0.03                # biasprm[:, 0] = BIAS0 x gainprm[:, 0]: the force of a 0.03 rad servo error (30 N Airbot arm, 1.8 N Go2)
BIAS2 = -0.25               # biasprm[u, 2] = BIAS2 / (timestep x dof_invweight0[dof of u]).  Euler takes the actuator force explicitly
                            # (in MuJoCo too; implicitfast would not, and model_fields refuses a velocity term there, so every case with
                            # bias2 runs Euler), so the feedback stays at 0.25 (x gear^2) of the joint's inertia / timestep, where an
                            # explicit step is stable: 3.9 .. 0.008 on the Airbot, 1.7 .. 0.44 on the Go2; the velocity term is then
                            # 0.1 .. 5 % of the force at the test's qvel (N(0, 0.2)), a hundred times the comparison's bound and more
ACTFRC = 10.0               # jnt_actfrcrange (-10, 10) on the Go2's actuated joints: gear x forcerange reaches 1.25 x 24 there
ACTFRC_SCALE = (0.75, 0.875)  # the Airbot's jnt_actfrcrange (-24, 24) -> (-18, 21), (-8, 8) -> (-6, 7): see actuators
GRAVITY = (1.5, -2.0, -9.0)
ARMATURE = (0.02, 0.005)    # dof_armature[i] = 0.02 + 0.005 i: distinct per dof, free-joint dofs (cube, T block, Go2 trunk) included
CTRL_OUT = 0.25             # smooth_offsets: ctrl this fraction of the range width beyond its end


def euler_damped(A):
    """Euler with eulerdamp on: implicit in the damping wherever any dof is damped (the per-env zero damping of the odd envs is
    not a model constant: smooth_dr)"""
    _set(A, "opt_integrator", INT_EULER)
    _set(A, "opt_disable_eulerdamp", 0)


def euler_plain(A):
    _set(A, "opt_integrator", INT_EULER)
    _set(A, "opt_disable_eulerdamp", 1)


def implicitfast(A):
    _set(A, "opt_integrator", INT_IMPLICITFAST)


def actuators(A, lift=False):
    """gear - + + - of GEAR; biasprm 0 as a fraction of the gain, biasprm 2 by the joint's inertia (see BIAS2); ctrllimited 0 on odd
    actuators, forcelimited 0 on even ones; jnt_actfrclimited of the actuated joints: the Go2's become limited to +-ACTFRC.
    An implicitfast model (the Airbot) becomes Euler with eulerdamp on: the same solve (M + h D) while every env is damped, and the
    integrator under which a velocity term in the actuator force is taken explicitly by definition.
    The Airbot's joint clamp stays on unless `lift`, with the range at ACTFRC_SCALE times the shipped one: without that clamp the
    position servos (kp 1000 against a wrist inertia of 8e-5) amplify a one-ulp change of qvel to 2.7e-3 of qpos (p99, f32 oracle)
    over the env step's four substeps, 20 times what the shipped model does (1.2e-4; 1.8e-4 with the clamp at the new range), and
    the f32 oracle's distance from the f64 one then measures that amplification, not rounding.  smooth_combined lifts it: the
    armature there holds the amplification at the shipped model's."""
    if int(np.asarray(A["opt_integrator"])[0]) == INT_IMPLICITFAST:
        euler_damped(A)
    nu = len(np.asarray(A["actuator_gear"]))
    u = np.arange(nu)
    _set(A, "actuator_gear", np.where((u % 4 == 1) | (u % 4 == 2), GEAR[0], GEAR[1]))
    kp = np.asarray(A["actuator_gainprm"])[:, 0]
    bias = np.asarray(A["actuator_biasprm"]).copy()
    dof = np.asarray(A["jnt_dofadr"])[np.asarray(A["actuator_trnid"]).astype(int)]
    bias[:, 0] = BIAS0 * kp
    bias[:, 2] = BIAS2 / (float(np.asarray(A["opt_timestep"])[0]) * np.asarray(A["dof_invweight0"])[dof])
    A["actuator_biasprm"] = bias
    _set(A, "actuator_ctrllimited", np.where(u % 2 == 1, 0, np.asarray(A["actuator_ctrllimited"])))
    _set(A, "actuator_forcelimited", np.where(u % 2 == 0, 0, np.asarray(A["actuator_forcelimited"])))
    lim, rng = np.asarray(A["jnt_actfrclimited"]).copy(), np.asarray(A["jnt_actfrcrange"]).copy()
    for j in np.asarray(A["actuator_trnid"]).astype(int):
        if not lim[j]:
            lim[j], rng[j] = 1, (-ACTFRC, ACTFRC)
        elif lift:
            lim[j] = 0
        else:
            rng[j] = rng[j] * np.asarray(ACTFRC_SCALE)
    A["jnt_actfrclimited"], A["jnt_actfrcrange"] = lim, rng


def gravity(A):
    _set(A, "opt_gravity", GRAVITY)


def armature(A):
    _set(A, "dof_armature", ARMATURE[0] + ARMATURE[1] * np.arange(len(np.asarray(A["dof_armature"]))))


def smooth_combined(A):
    """all of the above under Euler with eulerdamp on (implicit in the damping on both families; on the Go2 that is the flipped
    eulerdamp, and implicitfast is left to its own variant: it excludes bias2); the Airbot's joint clamp on the actuator force is
    lifted here (see actuators)"""
    actuators(A, lift=True)
    gravity(A)
    armature(A)
    euler_damped(A)


SMOOTH_VARIANTS = {
    "euler_damped": (("cube", "tshape", "go2flat", "footstand"), euler_damped),
    "euler_plain": (("cube", "tshape"), euler_plain),
    "implicitfast": (("go2flat", "go2rough", "footstand"), implicitfast),
    "actuators": (("cube", "go2flat"), actuators),
    "actuators_dr": (("go2flat",), actuators),         # with the Go2 domain randomisation on: per-env gainprm / biasprm leaves
    "gravity": (("cube", "go2flat", "footstand"), gravity),
    "armature": (("cube", "tshape", "go2flat"), armature),
    "smooth_combined": (("cube", "go2flat"), smooth_combined),
}
SMOOTH_CASES = [(name, kind) for name, (kinds, _) in SMOOTH_VARIANTS.items() for kind in kinds]
INTEGRATOR_CASES = [(name, kind) for name, kind in SMOOTH_CASES if name in ("euler_damped", "euler_plain", "implicitfast", "smooth_combined")]


def table_of(name):
    """the table (VARIANTS or SMOOTH_VARIANTS) that holds a variant"""
    assert (name in VARIANTS) != (name in SMOOTH_VARIANTS), name
    return VARIANTS if name in VARIANTS else SMOOTH_VARIANTS


def apply(envdef, name):
    """edits envdef.sys.arrays in place (the dict; its arrays are replaced), before envdef.batched(n)"""
    table_of(name)[name][1](envdef.sys.arrays)
    return envdef


def envdef_of(kind, variant=None):
    """the env definition of a family (no batch, no device), with a variant applied"""
    from rsr_mjx_amd.envs import families
    envdef = families.envdef(kind)
    if variant is not None:
        assert kind in table_of(variant)[variant][0], (variant, kind)
        apply(envdef, variant)
    return envdef


def blob_of(envdef):
    """the blob BatchedEnv.__init__ packs for envdef.batched(n) (episode_length 0, no auto reset), built on the CPU"""
    from rsr_mjx_amd.model import model_fields, pack_blob
    f = model_fields(envdef.sys)
    f.update(envdef._fields_fn(envdef.sys, episode_length=0, auto_reset=False, **envdef._kwargs))
    return pack_blob(f)


def dims_of(blob):
    """the library's Dims of a blob (rsr_model_create runs on the host: no device needed)"""
    import ctypes as C
    from rsr_mjx_amd import _lib
    h, dims = C.c_void_p(), _lib.Dims()
    _lib.check(_lib.lib().rsr_model_create(C.create_string_buffer(blob, len(blob)), len(blob), C.byref(h)))
    _lib.check(_lib.lib().rsr_model_dims(h, C.byref(dims)))
    _lib.lib().rsr_model_destroy(h)
    return dims


def cube_z(A, names):
    """qpos address of the z of the pushed cube's free joint (Airbot cube scene)"""
    body = int(names["body"]["cube_for_push"])
    j = int(A["body_jntadr"][body])
    assert int(A["jnt_type"][j]) == 0
    return int(A["jnt_qposadr"][j]) + 2


def positive_limits(A, qpos):
    """limited hinge / slide joints of one state whose limit distance is positive and inside jnt_margin: active through the margin
    alone"""
    out = []
    for j in range(len(A["jnt_type"])):
        if A["jnt_limited"][j] and int(A["jnt_type"][j]) in (2, 3):
            q = float(qpos[int(A["jnt_qposadr"][j])])
            dist = min(q - float(A["jnt_range"][j][0]), float(A["jnt_range"][j][1]) - q)
            if 0.0 < dist < float(A["jnt_margin"][j]):
                out.append(j)
    return out


ELBOW, WRIST = 2, 5          # Airbot joints: the elbow hinge, and the last arm hinge (the gripper's roll, range +-3.14)


def offsets(envdef, kind, qpos):
    """Per-env offsets on top of random_states, in place, the same for every variant of a family:
      cube      : the cube's free-joint z lowered by U(0, 0.005): the reset puts its four table contacts at one depth, and the contact
                  depth has to span the impedance curve; in every third env the elbow bent by a further 0.2 rad, which puts the
                  fingers into the table (the reset states touch on two geom pairs only, table - cube and table - target: too few
                  for three friction rules); in every other third the gripper's roll within U(0, 0.05) of its upper limit: a limit
                  distance inside the margin band (the other limits that are ever active are the three joints whose range is
                  2e-4 wide, always violated);
      go2flat   : the trunk height moved by U(-0.03, 0.03): the feet's sphere contacts keep positive distances, which is where
                  the margin band 0 < dist < margin - gap comes from (no box contact is kept at dist > 0);
      footstand : the trunk height swept over 0.06 .. 0.2 (the sweep of test_handstand.py): capsule and cylinder contacts.
    The T-shape and the rough-terrain Go2 states stay as they are."""
    n = len(qpos)
    rng = np.random.default_rng(SEED + 1)
    if kind == "cube":
        A = envdef.sys.arrays
        qpos[:, cube_z(A, envdef.sys.names)] -= rng.uniform(0.0, 0.005, n).astype(qpos.dtype)
        qpos[0::3, int(A["jnt_qposadr"][ELBOW])] -= 0.2
        third = qpos[1::3]
        qpos[1::3, int(A["jnt_qposadr"][WRIST])] = (float(A["jnt_range"][WRIST][1]) - rng.uniform(0.0, 0.05, len(third))).astype(qpos.dtype)
    elif kind == "go2flat":
        qpos[:, 2] += rng.uniform(-0.03, 0.03, n).astype(qpos.dtype)
    elif kind == "footstand":
        qpos[:, 2] = np.linspace(0.06, 0.2, n).astype(qpos.dtype)[rng.permutation(n)]
    return qpos


def oracle_states(oracle_mod, kind, n=N, seed=SEED):
    """random_states on the CPU: the f32 oracle's reset of the shipped model for PRNGKey(seed), the same perturbation (the same
    generator, draw for draw), then offsets()."""
    from physics_support import perturb
    from rsr_mjx_amd import prng
    envdef = envdef_of(kind)
    o = oracle_mod.Oracle(blob_of(envdef), "f32")
    st = o.new_state(n)
    o.reset(st, prng.split(prng.PRNGKey(seed), n))
    qpos, qvel, ctrl = perturb(envdef.sys.arrays, st["qpos"], st["qvel"], seed)
    return offsets(envdef, kind, qpos), qvel, ctrl


def device_states(envdef, kind, n=N, seed=SEED):
    """random_states (the device's reset of the shipped model) plus offsets()"""
    from physics_support import random_states
    qpos, qvel, ctrl = random_states(envdef, kind, n, seed)
    return offsets(envdef, kind, qpos), qvel, ctrl


# ---- the smooth side: states and per-env leaves

def smooth_offsets(kind, qpos, qvel, ctrl):
    """On top of the states above, in place: in every third env ctrl is put CTRL_OUT of the range width outside
    actuator_ctrlrange, above it on the actuators with (u + env) even and below it on the others, so that both ends of the ctrl
    clamp engage (physics_support.perturb draws ctrl inside the range) and, where ctrllimited is 0, the unclamped ctrl shows."""
    R = np.asarray(envdef_of(kind).sys.arrays["actuator_ctrlrange"], np.float64)
    lo, hi = R[:, 0], R[:, 1]
    envs = np.arange(0, len(ctrl), 3)
    up = (np.arange(len(lo))[None, :] + envs[:, None]) % 2 == 0
    ctrl[envs] = np.where(up, hi + CTRL_OUT * (hi - lo), lo - CTRL_OUT * (hi - lo)).astype(ctrl.dtype)
    return qpos, qvel, ctrl


def smooth_oracle_states(oracle_mod, kind, n=N, seed=SEED):
    return smooth_offsets(kind, *oracle_states(oracle_mod, kind, n, seed))


def smooth_device_states(envdef, kind, n=N, seed=SEED):
    return smooth_offsets(kind, *device_states(envdef, kind, n, seed))


def smooth_dr(variant, envdef, n=N):
    """The per-env leaves of a smooth case, {field: [n, ...]} as BatchedEnv.set_randomization takes them, or None: euler_damped
    zeroes dof_damping in the odd envs (the even ones keep the model's), so that one batch holds both sides of the eulerdamp
    decision; actuators_dr is the Go2 randomisation of physics_support.make(dr_on=True) on the edited model."""
    A = envdef.sys.arrays
    if variant == "euler_damped":
        damp = np.tile(np.asarray(A["dof_damping"], np.float32)[None], (n, 1))
        damp[1::2] = 0.0
        return dict(dof_damping=damp)
    if variant == "actuators_dr":
        from rsr_mjx_amd import prng
        from rsr_mjx_amd.envs import go2
        return go2.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(12), n))
    return None


def per_env_blobs(blob, dr, n=N):
    """(blobs, which): the distinct model blobs the oracle needs and which[e], the one of env e: `blob` with env e's leaves of
    `dr` in place of the model's (the oracle's debug forward reads the model's own values)"""
    if dr is None:
        return [blob], np.zeros(n, int)
    from rsr_mjx_amd.model import pack_blob, unpack_blob
    fields = unpack_blob(blob)
    blobs, which, seen = [], np.zeros(n, int), {}
    for e in range(n):
        g = dict(fields)
        for k, v in dr.items():
            g[k] = np.asarray(v[e], dtype=fields[k].dtype).reshape(fields[k].shape)
        b = pack_blob(g)
        if b not in seen:
            seen[b] = len(blobs)
            blobs.append(b)
        which[e] = seen[b]
    return blobs, which


def per_env_pass(oracle_mod, blobs, which, dims, qpos, qvel, ctrl, warm=None, precisions=("f32", "f64")):
    """physics_support.oracle_pass with env e on blobs[which[e]]: {precision: per-env list}, the envs in their own order"""
    from physics_support import oracle_pass
    out = {p: [None] * len(qpos) for p in precisions}
    for k, blob in enumerate(blobs):
        idx = np.nonzero(which == k)[0]
        r = oracle_pass(oracle_mod, blob, dims, qpos[idx], qvel[idx], ctrl[idx], None if warm is None else warm[idx], precisions=precisions)
        for p in precisions:
            for i, e in enumerate(idx):
                out[p][e] = r[p][i]
    return out


def per_env_steps(oracle_mod, blobs, which, dims, qpos, qvel, ctrl, nsteps, fields, precisions=("f32", "f64")):
    """The loop of test_physics_gpu.test_physics_oracle_parity with env e on blobs[which[e]]: a forward pass from a zero warm
    start (what set_state does), then nsteps substeps, each warm-started from the previous pass's qacc.  Returns {precision:
    {field: [n, w]}} with the counts (ne, nf, nl, ncon) of the last pass as "counts" [n, 4]; npyr from pair_condim."""
    from rsr_mjx_amd.model import unpack_blob
    npyr = 2 * (int(unpack_blob(blobs[0])["pair_condim"][0]) - 1)
    n, out = len(qpos), {}
    for p in precisions:
        oracles = []
        for blob in blobs:
            o = oracle_mod.Oracle(blob, p)
            o.set_ncon_cap(int(dims.ncon_max))
            oracles.append(o)
        res = {f: [] for f in fields}
        counts = np.zeros((n, 4), int)
        for e in range(n):
            o = oracles[which[e]]
            q, v = qpos[e].astype(np.float64), qvel[e].astype(np.float64)
            o.forward(q, v, ctrl[e], np.zeros(int(dims.nv)), step=False)
            for _ in range(nsteps):
                w = o.get("qacc")
                o.forward(q, v, ctrl[e], w, step=True)
                q, v = o.get("qpos"), o.get("qvel")
            for f in fields:
                res[f].append(o.get(f))
            nefc, ne, nf, ncon = (int(x) for x in o.get("counts", 6)[:4])
            counts[e] = [ne, nf, nefc - ne - nf - npyr * ncon, ncon]
        out[p] = {f: np.stack(a) for f, a in res.items()}
        out[p]["counts"] = counts
    return out
