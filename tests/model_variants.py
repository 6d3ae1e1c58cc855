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
imported inside them."""
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


def apply(envdef, name):
    """edits envdef.sys.arrays in place (the dict; its arrays are replaced), before envdef.batched(n)"""
    VARIANTS[name][1](envdef.sys.arrays)
    return envdef


def envdef_of(kind, variant=None):
    """the env definition of a family (no batch, no device), with a variant applied"""
    from rsr_mjx_amd.envs import airbot, go2
    if kind in ("cube", "tshape"):
        envdef = airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
    else:
        envdef = go2.load({"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain", "footstand": "Go2Footstand"}[kind])
    if variant is not None:
        assert kind in VARIANTS[variant][0], (variant, kind)
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
