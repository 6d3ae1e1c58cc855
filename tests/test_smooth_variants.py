"""The reference of tests/test_smooth_variants_gpu.py, pinned on the CPU before the kernels are judged against it: for every
(variant, family) of model_variants.SMOOTH_CASES the f64 oracle's actuator_force, qfrc_actuator, qfrc_bias at rest, M and one
integration step against closed forms written in numpy fp64 from the raw arrays of the blob, none of which goes through the
oracle's recursions (RNE, CRB, its Cholesky): gain / bias / gear / clamps from MuJoCo's definitions (mj_fwdActuation), gravity as
-sum_b m_b J_b(xipos_b)^T g and M as sum_b J^T m J + J^T I J + armature through mjcf.body_jacobian and mjcf.mass_matrix, and the
integrator's decision, solve and semi-implicit update from the oracle's own M, qfrc_smooth, qfrc_constraint and the env's damping.
Then the conditions under which the device tests show anything.

The integrator's solve is (M + h diag(D)) qacc = qfrc_smooth + qfrc_constraint.  That is mj_Euler with eulerdamp on.  It is
MuJoCo's implicitfast only while no actuator has a velocity term: implicitfast solves (M - h qDeriv) with qDeriv = -diag(D) +
moment^T diag(biasprm[:, 2] + gainprm[:, 2] ctrl) moment, and the oracle, the kernels and this closed form all leave the second
part out ("actuator velocity gains, zero here").  Finding of this work: the bias2 variants are the first models with
such a term, and rsr_model_create accepted one under implicitfast and would have simulated it differently from MuJoCo.
model.model_fields (and set_randomization for the per-env leaves) now refuses biasprm[:, 2] or gainprm[:, 2] != 0 under
implicitfast, and every variant with bias2 runs Euler, where MuJoCo takes the actuator force explicitly as well: actuators turns
the Airbot to Euler with eulerdamp on, smooth_combined runs that on both families, and implicitfast on the Go2 has no bias2.

What the shipped assets agree on, and the variant that moves it:
  opt_integrator / opt_disable_eulerdamp   Airbot implicitfast (3) / 0, Go2 Euler (0) / 1      euler_damped, euler_plain, implicitfast (and
                                                                                               Euler with eulerdamp in every bias2 case)
  actuator_gear                            1                                                   actuators (1.25, -0.6 in the pattern - + + -)
  actuator_biasprm[:, 0], [:, 2]           0                                                   actuators (0.03 x the gain; -0.25 inertia / timestep)
  actuator_ctrllimited, _forcelimited      1                                                   actuators (0 on odd / on even actuators)
  jnt_actfrclimited                        0 on the Go2, 1 on the Airbot's arm                 actuators (Go2 limited to +-10; Airbot range x (0.75, 0.875), lifted in smooth_combined)
  opt_gravity                              (0, 0, -9.81)                                       gravity (1.5, -2, -9)
  dof_armature                             0 on the Airbot and the Go2 trunk                   armature (0.02 + 0.005 i)
and smooth_combined sets all of them.  euler_damped also zeroes dof_damping in the odd envs (a per-env leaf on the device, a second
blob here), so both sides of the eulerdamp decision are in one batch; actuators_dr is actuators under the Go2 randomisation, every
env on a blob of its own.

States: model_variants.smooth_oracle_states: the constraint variants' states (the f32 oracle's reset of the shipped model for
PRNGKey(11), physics_support.perturb with seed 11, model_variants.offsets) with ctrl a quarter of the range width outside
actuator_ctrlrange in every third env.  256 envs.

Kinematics.  The closed forms need fp64 frames.  mjcf.forward_kinematics renormalises every body quaternion and joint axis; the
oracle, like MuJoCo's mj_kinematics, does not, and the blob carries the model's unit quaternions rounded to fp32, so the two
differ by the fp32 rounding of the constants (measured 1.6e-8 on the Airbot's xpos, 3e-16 on the Go2's, whose body quaternions are
exact in fp32), above the closed forms' bound.  frames() therefore restates mj_kinematics in numpy without the renormalisation and
is itself held to the oracle's xpos / xmat at the closed forms' bound and to mjcf.forward_kinematics within 2e-6 (24-bit constants
along a chain of at most nine bodies); everything downstream is mjcf.body_jacobian and mjcf.mass_matrix on those frames.

Bound of the closed forms: 1e-9 of the field's largest magnitude in the env (both sides are double precision).  The integrator
needs no more: cond(M + h D) is at most 1.5e3 over all cases (16 with the armature), cond x 2^-52 = 3e-13; the test asserts that.
Measured, worst env per case (actuator_force / qfrc_actuator / gravity / M / qvel / qpos after the step; cond: 1 where every env
integrates explicitly):
  euler_damped     cube       0 / 0 / 3.6e-16 / 1.9e-16 / 6.0e-16 / 1.5e-16; cond 1.5e3; frames vs mjcf.forward_kinematics 1.6e-8
  euler_damped     tshape     0 / 0 / 2.2e-16 / 1.3e-16 / 5.7e-16 / 7.8e-17; cond 9.0e2; frames vs mjcf.forward_kinematics 1.6e-8
  euler_damped     go2flat    0 / 0 / 4.4e-17 / 6.6e-17 / 8.7e-16 / 1.2e-16; cond 7.7e2; frames vs mjcf.forward_kinematics 2.2e-16
  euler_damped     footstand  0 / 0 / 3.4e-17 / 5.7e-17 / 1.0e-15 / 4.3e-16; cond 1.3e3; frames vs mjcf.forward_kinematics 2.2e-16
  euler_plain      cube       0 / 0 / 3.6e-16 / 1.9e-16 / 0 / 7.7e-17; cond 1.0e0; frames vs mjcf.forward_kinematics 1.6e-8
  euler_plain      tshape     0 / 0 / 2.2e-16 / 1.3e-16 / 0 / 7.8e-17; cond 1.0e0; frames vs mjcf.forward_kinematics 1.6e-8
  implicitfast     go2flat    0 / 0 / 4.4e-17 / 6.6e-17 / 1.1e-15 / 2.1e-16; cond 7.8e2; frames vs mjcf.forward_kinematics 2.2e-16
  implicitfast     go2rough   0 / 0 / 4.4e-17 / 6.6e-17 / 8.5e-16 / 1.2e-16; cond 7.8e2; frames vs mjcf.forward_kinematics 2.2e-16
  implicitfast     footstand  0 / 0 / 3.4e-17 / 5.7e-17 / 1.0e-15 / 4.3e-16; cond 1.3e3; frames vs mjcf.forward_kinematics 2.2e-16
  actuators        cube       0 / 0 / 3.6e-16 / 1.9e-16 / 7.9e-16 / 1.5e-16; cond 1.5e3; frames vs mjcf.forward_kinematics 1.6e-8
  actuators        go2flat    0 / 0 / 4.4e-17 / 6.6e-17 / 0 / 1.2e-16; cond 1.0e0; frames vs mjcf.forward_kinematics 2.2e-16
  actuators_dr     go2flat    0 / 0 / 3.8e-16 / 9.3e-17 / 0 / 1.2e-16; cond 1.0e0; frames vs mjcf.forward_kinematics 3.3e-16
  gravity          cube       0 / 0 / 3.0e-16 / 1.9e-16 / 8.1e-16 / 1.4e-16; cond 1.5e3; frames vs mjcf.forward_kinematics 1.6e-8
  gravity          go2flat    0 / 0 / 3.1e-17 / 6.6e-17 / 0 / 1.2e-16; cond 1.0e0; frames vs mjcf.forward_kinematics 2.2e-16
  gravity          footstand  0 / 0 / 4.6e-17 / 5.7e-17 / 0 / 1.2e-16; cond 1.0e0; frames vs mjcf.forward_kinematics 2.2e-16
  armature         cube       0 / 0 / 3.6e-16 / 1.6e-16 / 5.9e-16 / 7.7e-17; cond 1.6e1; frames vs mjcf.forward_kinematics 1.6e-8
  armature         tshape     0 / 0 / 2.2e-16 / 1.6e-16 / 2.7e-16 / 7.8e-17; cond 1.7e1; frames vs mjcf.forward_kinematics 1.6e-8
  armature         go2flat    0 / 0 / 4.4e-17 / 6.6e-17 / 0 / 1.2e-16; cond 1.0e0; frames vs mjcf.forward_kinematics 2.2e-16
  smooth_combined  cube       0 / 0 / 3.0e-16 / 1.6e-16 / 6.6e-16 / 1.6e-16; cond 1.6e1; frames vs mjcf.forward_kinematics 1.6e-8
  smooth_combined  go2flat    0 / 0 / 3.1e-17 / 6.6e-17 / 1.1e-15 / 1.2e-16; cond 2.1e2; frames vs mjcf.forward_kinematics 2.2e-16

Branch counts, these states, f64 oracle: actuators with the ctrl clamp engaged at its lower / upper end and with ctrl outside an
unlimited range; with the force clamp engaged and with |force| beyond the range of an unlimited actuator; dofs with the joint's
actuator-force clamp engaged; envs on the implicit / explicit side of the integrator's decision; envs whose qfrc_smooth or
post-step qvel moved by more than 1e-3 against the shipped model; envs left out by the f32-vs-f64 part of the exclusion:
  euler_damped     cube       ctrl 215 / 215, outside 0; force 942, beyond 0; actfrc 1272; implicit 128 / 128; moved 128; excluded 0
  euler_damped     tshape     ctrl 215 / 215, outside 0; force 912, beyond 0; actfrc 1270; implicit 128 / 128; moved 128; excluded 0
  euler_damped     go2flat    ctrl 516 / 516, outside 0; force 2308, beyond 0; actfrc 0; implicit 128 / 128; moved 256; excluded 0
  euler_damped     footstand  ctrl 516 / 516, outside 0; force 1434, beyond 0; actfrc 0; implicit 128 / 128; moved 256; excluded 0
  euler_plain      cube       ctrl 215 / 215, outside 0; force 942, beyond 0; actfrc 1272; implicit 0 / 256; moved 256; excluded 0
  euler_plain      tshape     ctrl 215 / 215, outside 0; force 912, beyond 0; actfrc 1270; implicit 0 / 256; moved 256; excluded 0
  implicitfast     go2flat    ctrl 516 / 516, outside 0; force 2308, beyond 0; actfrc 0; implicit 256 / 0; moved 256; excluded 0
  implicitfast     go2rough   ctrl 516 / 516, outside 0; force 2308, beyond 0; actfrc 0; implicit 256 / 0; moved 256; excluded 0
  implicitfast     footstand  ctrl 516 / 516, outside 0; force 1434, beyond 0; actfrc 0; implicit 256 / 0; moved 256; excluded 0
  actuators        cube       ctrl 129 / 129, outside 172; force 406, beyond 535; actfrc 1270; implicit 256 / 0; moved 256; excluded 0
  actuators        go2flat    ctrl 258 / 258, outside 516; force 1289, beyond 1221; actfrc 2868; implicit 0 / 256; moved 256; excluded 0
  actuators_dr     go2flat    ctrl 258 / 258, outside 516; force 1290, beyond 1218; actfrc 2867; implicit 0 / 256; moved 256; excluded 0
  gravity          cube       ctrl 215 / 215, outside 0; force 942, beyond 0; actfrc 1272; implicit 256 / 0; moved 256; excluded 0
  gravity          go2flat    ctrl 516 / 516, outside 0; force 2308, beyond 0; actfrc 0; implicit 0 / 256; moved 256; excluded 0
  gravity          footstand  ctrl 516 / 516, outside 0; force 1434, beyond 0; actfrc 0; implicit 0 / 256; moved 256; excluded 0
  armature         cube       ctrl 215 / 215, outside 0; force 942, beyond 0; actfrc 1272; implicit 256 / 0; moved 256; excluded 0
  armature         tshape     ctrl 215 / 215, outside 0; force 912, beyond 0; actfrc 1270; implicit 256 / 0; moved 256; excluded 0
  armature         go2flat    ctrl 516 / 516, outside 0; force 2308, beyond 0; actfrc 0; implicit 0 / 256; moved 256; excluded 0
  smooth_combined  cube       ctrl 129 / 129, outside 172; force 406, beyond 535; actfrc 0; implicit 256 / 0; moved 256; excluded 0
  smooth_combined  go2flat    ctrl 258 / 258, outside 516; force 1289, beyond 1221; actfrc 2868; implicit 256 / 0; moved 256; excluded 0
The bias2 term's median share of the force, as physics_support.rel would see its loss: 1.4e-3 on the cube, 3.0e-3 on the Go2.
(euler_damped on the Airbot: the even envs keep their damping, and Euler with eulerdamp is then the same solve as the shipped
implicitfast, so only the odd envs move, through the damping they lose; that case is there for the wave-uniform decision.)"""
import copy

import numpy as np
import pytest

import model_variants as V
import physics_support as S
from rsr_mjx_amd import mjcf

BOUND = 1e-9
_CASES = {}
_LEAVES = ("geom_friction", "body_ipos", "body_mass", "qpos0", "dof_frictionloss", "dof_armature", "actuator_gainprm", "actuator_biasprm",
           "dof_damping")


def _f32(v):
    v = np.asarray(v)
    return v.astype(np.float32).astype(np.float64) if v.dtype.kind == "f" else v


def case(oracle_mod, variant, kind):
    """dict of one (variant or None, family): envdef, A (its arrays as the blob carries them: fp32, widened), the per-env leaves dr,
    the blobs and which[e], dims, the CPU states, the forward pass on them (ref) and the same at qvel = 0 (rest); built once"""
    if (variant, kind) not in _CASES:
        envdef = V.envdef_of(kind, variant)
        blob = V.blob_of(envdef)
        dims = V.dims_of(blob)
        dr = V.smooth_dr(variant, envdef) if variant else None
        blobs, which = V.per_env_blobs(blob, dr)
        qpos, qvel, ctrl = V.smooth_oracle_states(oracle_mod, kind)
        ref = V.per_env_pass(oracle_mod, blobs, which, dims, qpos, qvel, ctrl)
        rest = V.per_env_pass(oracle_mod, blobs, which, dims, qpos, np.zeros_like(qvel), ctrl, precisions=("f64",))["f64"]
        A = {k: _f32(v) for k, v in envdef.sys.arrays.items()}
        _CASES[(variant, kind)] = dict(envdef=envdef, A=A, dr=dr, blobs=blobs, which=which, dims=dims, qpos=qpos, qvel=qvel, ctrl=ctrl,
                                       ref=ref, rest=rest, npyr=S.npyr(envdef))
    return _CASES[(variant, kind)]


def arrays_of(c, e):
    """the model arrays of env e: A with the env's leaves in place of the model's"""
    if c["dr"] is None:
        return c["A"]
    A = dict(c["A"])
    for k, v in c["dr"].items():
        assert k in _LEAVES and k in A, k
        A[k] = _f32(np.asarray(v[e], np.float32)).reshape(A[k].shape)
    return A


def model_of(c, e):
    m = copy.copy(c["envdef"].sys)
    m.arrays = arrays_of(c, e)
    return m


def err(mine, his):
    """|mine - his|_inf over the field's largest magnitude"""
    mine, his = np.asarray(mine, np.float64), np.asarray(his, np.float64)
    return float(np.abs(mine - his).max() / max(np.abs(his).max(), 1e-300)) if his.size else 0.0


# ---- the closed forms, fp64

def frames(m, qpos):
    """mj_kinematics as mjcf.forward_kinematics states it, without renormalising body quaternions and joint axes (see the module
    docstring): dict(xpos, xquat, xmat, xipos, ximat, xanchor, xaxis, qpos with the free joints' quaternions normalised)"""
    A, nb = m.arrays, m.nbody
    q = np.array(qpos, np.float64)
    xpos, xquat = np.zeros((nb, 3)), np.tile(np.array([1.0, 0, 0, 0]), (nb, 1))
    xanchor, xaxis = np.zeros((m.njnt, 3)), np.zeros((m.njnt, 3))
    for b in range(1, nb):
        p = int(A["body_parentid"][b])
        pos = xpos[p] + mjcf.rotate(A["body_pos"][b], xquat[p])
        quat = mjcf.quat_mul(xquat[p], A["body_quat"][b])
        for j in range(int(A["body_jntadr"][b]), int(A["body_jntadr"][b]) + int(A["body_jntnum"][b])):
            jt, qa = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j])
            if jt == 0:
                q[qa + 3:qa + 7] /= np.linalg.norm(q[qa + 3:qa + 7])
                xanchor[j], xaxis[j], pos, quat = q[qa:qa + 3], [0, 0, 1.0], q[qa:qa + 3].copy(), q[qa + 3:qa + 7].copy()
            else:
                assert jt in (2, 3)
                xanchor[j], xaxis[j] = mjcf.rotate(A["jnt_pos"][j], quat) + pos, mjcf.rotate(A["jnt_axis"][j], quat)
                dq = q[qa] - A["qpos0"][qa]
                if jt == 3:
                    quat = mjcf.quat_mul(quat, np.concatenate([[np.cos(0.5 * dq)], np.sin(0.5 * dq) * A["jnt_axis"][j]]))
                    pos = xanchor[j] - mjcf.rotate(A["jnt_pos"][j], quat)
                else:
                    pos = pos + xaxis[j] * dq
        xpos[b], xquat[b] = pos, quat
    xmat = np.stack([mjcf.quat_to_mat(x) for x in xquat])
    xipos = np.stack([xpos[b] + xmat[b] @ A["body_ipos"][b] for b in range(nb)])
    ximat = np.stack([mjcf.quat_to_mat(mjcf.quat_mul(xquat[b], A["body_iquat"][b])) for b in range(nb)])
    return dict(xpos=xpos, xquat=xquat, xmat=xmat, xipos=xipos, ximat=ximat, xanchor=xanchor, xaxis=xaxis, qpos=q)


def actuation(A, qpos, qvel, ctrl):
    """(actuator_force [nu], qfrc_actuator [nv], flags) of mj_fwdActuation for joint transmissions with affine gain and bias:
    length = gear q, velocity = gear v; ctrl clamped to ctrlrange where ctrllimited; force = gain0 ctrl + bias0 + bias1 length +
    bias2 velocity, clamped to forcerange where forcelimited; qfrc_actuator = gear force on the joint's dof, clamped to the
    joint's actfrcrange where actfrclimited.  flags: what engaged, for the branch counts."""
    nu, nv = len(A["actuator_gear"]), len(A["dof_jntid"])
    force, qfrc = np.zeros(nu), np.zeros(nv)
    n = dict(ctrl_lo=0, ctrl_hi=0, ctrl_free_outside=0, force_clamped=0, force_free_outside=0, actfrc_clamped=0, bias2_share=[])
    for u in range(nu):
        j = int(A["actuator_trnid"][u])
        qa, da, gear = int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j]), float(A["actuator_gear"][u])
        c, (lo, hi) = float(ctrl[u]), A["actuator_ctrlrange"][u]
        if A["actuator_ctrllimited"][u]:
            n["ctrl_lo"] += c < lo
            n["ctrl_hi"] += c > hi
            c = min(max(c, lo), hi)
        else:
            n["ctrl_free_outside"] += c < lo or c > hi
        g, b = A["actuator_gainprm"][u], A["actuator_biasprm"][u]
        vel = b[2] * (gear * float(qvel[da]))
        f = g[0] * c + b[0] + b[1] * (gear * float(qpos[qa])) + vel
        n["bias2_share"].append(abs(vel))
        lo, hi = A["actuator_forcerange"][u]
        if A["actuator_forcelimited"][u]:
            n["force_clamped"] += f < lo or f > hi
            f = min(max(f, lo), hi)
        else:
            n["force_free_outside"] += f < lo or f > hi
        force[u] = f
        qfrc[da] += gear * f
    for i in range(nv):
        j = int(A["dof_jntid"][i])
        if A["jnt_actfrclimited"][j]:
            lo, hi = A["jnt_actfrcrange"][j]
            n["actfrc_clamped"] += qfrc[i] < lo or qfrc[i] > hi
            qfrc[i] = min(max(qfrc[i], lo), hi)
    return force, qfrc, n


def gravity_force(m, kin):
    """qfrc_bias at qvel = 0: -sum_b m_b J_b(xipos_b)^T g"""
    g = m.arrays["opt_gravity"]
    out = np.zeros(m.nv)
    for b in range(1, m.nbody):
        jacp, _ = mjcf.body_jacobian(m, kin, kin["xipos"][b], b)
        out -= float(m.arrays["body_mass"][b]) * (jacp.T @ g)
    return out


def implicit_decision(A):
    """implicitfast, or Euler with eulerdamp on and any damped dof"""
    integrator = int(A["opt_integrator"][0])
    assert integrator in (V.INT_EULER, V.INT_IMPLICITFAST)
    return integrator == V.INT_IMPLICITFAST or (int(A["opt_disable_eulerdamp"][0]) == 0 and bool(np.any(A["dof_damping"] != 0)))


def integrate(A, qpos, qvel, M, fs, fc, qacc):
    """(qpos, qvel, implicit, cond) one step on: qacc = (M + h diag(D))^-1 (qfrc_smooth + qfrc_constraint) where implicit_decision,
    the solver's qacc otherwise; qvel += h qacc; qpos += h qvel, a free joint's quaternion q <- normalise(q * (cos(h |w| / 2),
    sin(h |w| / 2) w / |w|)) with w its (body-frame) angular velocity"""
    h, D = float(A["opt_timestep"][0]), A["dof_damping"]
    implicit = implicit_decision(A)
    cond = 1.0
    if implicit:
        Ah = M + h * np.diag(D)
        qacc, cond = np.linalg.solve(Ah, fs + fc), float(np.linalg.cond(Ah))
    v = np.asarray(qvel, np.float64) + h * qacc
    q = np.array(qpos, np.float64)
    for j in range(len(A["jnt_type"])):
        qa, da = int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
        if int(A["jnt_type"][j]) == 0:
            q[qa:qa + 3] += h * v[da:da + 3]
            w = v[da + 3:da + 6]
            n = np.linalg.norm(w)
            ax = w / n if n > 1e-15 else np.zeros(3)
            q2 = mjcf.quat_mul(q[qa + 3:qa + 7], np.concatenate([[np.cos(0.5 * h * n)], np.sin(0.5 * h * n) * ax]))
            q[qa + 3:qa + 7] = q2 / np.linalg.norm(q2)
        else:
            q[qa] += h * v[da]
    return q, v, implicit, cond


def closed(oracle_mod, c):
    """the closed forms of every env of a case against the oracle: dict of worst errors and branch counts; cached on the case"""
    if "closed" in c:
        return c["closed"]
    n = V.N
    worst = dict(actuator_force=0.0, qfrc_actuator=0.0, gravity=0.0, M=0.0, qvel=0.0, qpos=0.0, kin=0.0, cond=0.0)
    counts = dict(ctrl_lo=0, ctrl_hi=0, ctrl_free_outside=0, force_clamped=0, force_free_outside=0, actfrc_clamped=0, implicit=0, explicit=0)
    share, gmag = [], []
    oracles = [oracle_mod.Oracle(b, "f64") for b in c["blobs"]]
    for o in oracles:
        o.set_ncon_cap(int(c["dims"].ncon_max))
    step = dict(qvel=np.zeros((n, c["dims"].nv)), implicit=np.zeros(n, bool))
    for e in range(n):
        A, m = arrays_of(c, e), model_of(c, e)
        r, rest = c["ref"]["f64"][e], c["rest"][e]
        q, v, u = (c[k][e].astype(np.float64) for k in ("qpos", "qvel", "ctrl"))
        kin = frames(m, q)
        worst["kin"] = max(worst["kin"], float(np.abs(kin["xpos"] - mjcf.forward_kinematics(m, q)["xpos"]).max()))
        assert err(kin["xpos"], r["xpos"]) <= BOUND and err(kin["xmat"], r["xmat"]) <= BOUND, (e, "frames")
        force, qfrc, flags = actuation(A, kin["qpos"], v, u)
        for k in counts:
            counts[k] += int(flags.get(k, 0))
        share.append(max(flags["bias2_share"]) / max(1.0, np.abs(force).max()))          # what dropping bias2 would show as under rel()
        worst["qfrc_actuator"] = max(worst["qfrc_actuator"], err(qfrc, r["qfrc_actuator"]))
        g = gravity_force(m, kin)
        gmag.append(np.abs(g).max())
        worst["gravity"] = max(worst["gravity"], err(g, rest["qfrc_bias"]))
        worst["M"] = max(worst["M"], err(mjcf.mass_matrix(m, q, kin), r["M"]))
        o = oracles[c["which"][e]]
        o.forward(q, v, c["ctrl"][e], np.zeros(len(v)), step=True)
        worst["actuator_force"] = max(worst["actuator_force"], err(force, o.get("actuator_force")))
        M, fs, fc, qa = o.get("M").reshape(len(v), len(v)), o.get("qfrc_smooth"), o.get("qfrc_constraint"), o.get("qacc")
        q1, v1, implicit, cond = integrate(A, kin["qpos"], v, M, fs, fc, qa)
        worst["qvel"], worst["qpos"] = max(worst["qvel"], err(v1, o.get("qvel"))), max(worst["qpos"], err(q1, o.get("qpos")))
        worst["cond"] = max(worst["cond"], cond)
        counts["implicit" if implicit else "explicit"] += 1
        step["qvel"][e], step["implicit"][e] = o.get("qvel"), implicit
    c["closed"] = dict(worst=worst, counts=counts, bias2_share=float(np.median(share)), gravity_mag=float(np.min(gmag)), step=step)
    return c["closed"]


# ---- the tests

@pytest.mark.parametrize("variant,kind", V.SMOOTH_CASES)
def test_the_oracle_matches_the_closed_forms(oracle_mod, variant, kind):
    """actuator_force, qfrc_actuator, qfrc_bias at rest, M, and qvel / qpos after one step, every env, within 1e-9 of the field's
    largest magnitude; frames() against the oracle's xpos / xmat at the same bound and against mjcf.forward_kinematics at 2e-6."""
    w = closed(oracle_mod, case(oracle_mod, variant, kind))["worst"]
    print(variant, kind, "closed forms: force %.1e qfrc_actuator %.1e gravity %.1e M %.1e qvel %.1e qpos %.1e | cond(M + hD) <= %.1e | frames vs "
          "mjcf.forward_kinematics %.1e" % (w["actuator_force"], w["qfrc_actuator"], w["gravity"], w["M"], w["qvel"], w["qpos"], w["cond"], w["kin"]))
    assert w["cond"] * 2.0 ** -52 <= 0.1 * BOUND
    assert w["kin"] <= 2e-6
    for k in ("actuator_force", "qfrc_actuator", "gravity", "M", "qvel", "qpos"):
        assert w[k] <= BOUND, (variant, kind, k, w[k])


@pytest.mark.parametrize("variant,kind", V.SMOOTH_CASES)
def test_the_states_reach_what_the_variant_changes(oracle_mod, variant, kind):
    """The conditions that keep the device tests honest, on the reference alone:
      exclusion   : the f32 and the f64 oracle differ in their row counts in at most 2 % of the envs (keep's cap) on these states
                    (after the substeps the device test counts them: at most 1 of 256 in any case);
      ctrl clamp  : every case: both ends engaged, each in >= 5 % of the (env, actuator) slots; actuators: also ctrl outside the
                    range of unlimited actuators in >= 5 %;
      force clamp : actuators: engaged and, on unlimited actuators, |force| beyond the range, each in >= 1 % of the slots; the
                    bias2 term, as physics_support.rel would see its loss (largest |bias2 x velocity| of the env over max(1, largest
                    |force|)), has a median >= 1e-3: ten times the rule's cap on a single env;
      actfrc clamp: actuators: engaged in >= 5 % of the (env, actuated dof) slots; smooth_combined on the cube, which lifts it:
                    |qfrc_actuator| of the arm beyond the shipped range in as many;
      integrator  : the decision falls as the variant says: euler_damped 128 implicit / 128 explicit, euler_plain all explicit,
                    implicitfast all implicit, smooth_combined all implicit; no case has bias2 != 0 under implicitfast;
      gravity     : at rest the closed form's gravity force is at least 0.1 in every env;
      every case  : the f64 oracle's qfrc_smooth or post-step qvel differs from the shipped model's on the same states by more than
                    1e-3 (per env, relative as physics_support.rel) in at least 90 % of the envs (euler_damped on the Airbot: of the odd envs, see the
                    module docstring)."""
    c = case(oracle_mod, variant, kind)
    z = closed(oracle_mod, c)
    n, slots = z["counts"], V.N * int(c["dims"].nu)
    c64, c32 = S.counts_of(c["ref"]["f64"], c["npyr"]), S.counts_of(c["ref"]["f32"], c["npyr"])
    excl0 = int((c64 != c32).any(1).sum())
    base = case(oracle_mod, None, kind)
    zb = closed(oracle_mod, base)
    fs = lambda cc: np.stack([r["qfrc_smooth"] for r in cc["ref"]["f64"]])
    moved = np.maximum(S.rel(fs(c), fs(base)), S.rel(z["step"]["qvel"], zb["step"]["qvel"])) > 1e-3
    print(variant, kind, "ctrl clamp lo %d hi %d, free outside %d; force clamp %d, free beyond %d; actfrc clamp %d; implicit %d explicit %d; "
          "moved %d; excluded %d; bias2 share %.1e" % (n["ctrl_lo"], n["ctrl_hi"], n["ctrl_free_outside"], n["force_clamped"], n["force_free_outside"],
                                                         n["actfrc_clamped"], n["implicit"], n["explicit"], int(moved.sum()), excl0, z["bias2_share"]))
    assert excl0 <= 0.02 * V.N
    acts = variant in ("actuators", "actuators_dr", "smooth_combined")
    if acts:
        assert min(n["ctrl_lo"], n["ctrl_hi"], n["ctrl_free_outside"]) >= 0.05 * slots / 2, n        # (half the actuators each)
        assert min(n["force_clamped"], n["force_free_outside"]) >= 0.01 * slots, n
        assert z["bias2_share"] >= 1e-3
        if kind == "cube" and variant == "smooth_combined":
            beyond = sum((np.abs(r["qfrc_actuator"][:3]) > 24.0).sum() for r in c["ref"]["f64"])
            assert n["actfrc_clamped"] == 0 and beyond >= 0.05 * V.N * 3, beyond
        else:
            assert n["actfrc_clamped"] >= 0.05 * slots, n
    else:
        assert min(n["ctrl_lo"], n["ctrl_hi"]) >= 0.05 * slots and n["ctrl_free_outside"] == 0, n
    assert int(c["A"]["opt_integrator"][0]) != V.INT_IMPLICITFAST or not np.any(c["A"]["actuator_biasprm"][:, 2])
    want = dict(euler_damped=(V.N // 2, V.N // 2), euler_plain=(0, V.N), implicitfast=(V.N, 0), smooth_combined=(V.N, 0))
    if variant in want:
        assert (n["implicit"], n["explicit"]) == want[variant], n
        if variant == "euler_damped":
            assert (z["step"]["implicit"] == (np.arange(V.N) % 2 == 0)).all()
    else:
        assert (n["implicit"], n["explicit"]) == ((V.N, 0) if kind in S.IMPLICIT else (0, V.N)), n
    assert z["gravity_mag"] >= 0.1
    if variant == "euler_damped" and kind in S.IMPLICIT:
        assert moved[1::2].sum() >= 0.9 * (V.N // 2) and not moved[0::2].any(), (int(moved[1::2].sum()), int(moved[0::2].sum()))
    else:
        assert moved.sum() >= 0.9 * V.N, int(moved.sum())
