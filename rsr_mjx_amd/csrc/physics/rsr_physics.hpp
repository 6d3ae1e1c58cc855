// rsr_physics.hpp -- the physics layer's buffer layouts (side, dynamics, constraint, transition and inverse buffer) and the launch arguments of its ops,
// one struct per op of rsr_launch.hpp that needs its own (host and device).
#pragma once
#include "../../../include/rsr_physics.h"
#include "../rsr_solver.hpp"

namespace rsr {

// One entry per output element (host-expanded from the table): type, site, ref site or -1, component.  nsd = 0: no stage.
// acc_site: the one site of the table's accelerometers (-1: none); only compiled in for Dims::XFRC.
struct SensArgs {
  const int4* el;
  int nsd, acc_site;
};

// Side buffer (rsr_physics_view), per env, floats: qacc [nv] | actuator_force [nu] | xquat [nbody*4] | ncon | contacts [ncon_max][9]
// (dist, pos[3], normal[3], geom1, geom2) | ncon_dropped, padded to 16 floats.  Filled by these kernels only (rsr_step leaves it).
struct PhysLayout { int qacc, aforce, xquat, ncon, con, ncon_drop, stride; };
__host__ __device__ inline PhysLayout phys_layout(int nv, int nu, int nbody, int ncon_max) {
  PhysLayout p;
  p.qacc = 0; p.aforce = nv; p.xquat = nv + nu; p.ncon = p.xquat + 4 * nbody; p.con = p.ncon + 1; p.ncon_drop = p.con + 9 * ncon_max;
  p.stride = (p.ncon_drop + 1 + 15) & ~15;
  return p;
}
struct PhysArgs {
  const float* ctrl;    // [N][nu] or null (keep the record's ctrl)
  float* out;           // side buffer [N][PhysLayout::stride] or null
  const int* ids;       // [grid] the envs to run (rsr_physics_forward_envs), or null: env = workgroup index
  int nsteps;           // substeps (the step kernel)
  float* sd;            // sensordata [N][RSR_MAX_SENSORDATA], written when sens.nsd > 0
  SensArgs sens;
};
// data.xfrc_applied [nbody*6] (force, torque: world frame, at the body's COM) and data.qfrc_applied [nv] (rsr_physics_set_applied):
// the handle's buffers [N][...], xfrc null = off (Launch::ap), or one env's rows (AppliedStage, rsr_applied.hpp)
struct Applied {
  const float* xfrc;
  const float* qfrc;
};
// rsr_physics_transition_fd (rsr_transition.hpp).  Its buffer, per env, floats: [ncol][2 nv + RSR_MAX_SENSORDATA], one row per
// perturbed coordinate (ncol = 2 nv + nu: qpos tangent, qvel, ctrl): d qpos [nv] | d qvel [nv] | d sensordata [nsd], the rest of
// the row zeros.  The states buffer (RSR_FD_STATES): the perturbed inputs [N][ncol][2][xw] (qpos | qvel | ctrl), then, y0
// floats in, the end states [N][ncol][2][yw] (qpos | qvel); index 2: the run (+eps, then -eps or the unperturbed state).
struct FdLayout { int ncol, w, env, xw, yw; };
__host__ __device__ inline FdLayout fd_layout(int nq, int nv, int nu) {
  FdLayout f;
  f.ncol = 2 * nv + nu; f.w = 2 * nv + RSR_MAX_SENSORDATA; f.env = f.ncol * f.w; f.xw = nq + nv + nu; f.yw = nq + nv;
  return f;
}
// The launch arguments of OP_PHYS_TRANSITION (Launch::fd)
struct FdArgs {
  float* out;           // the transition buffer [N][FdLayout::env]
  float* states;        // the states buffer, or null: not kept
  const int* ids;       // [grid / ncol] the envs to run, or null: env = workgroup index / ncol
  float eps;
  int flags;            // RSR_FD_*
};
// rsr_physics_rollout: ctrl [N][T][nu]; trajectory rows [N][T][w], each pointer null = not recorded
struct RollArgs {
  const float* ctrl;
  int T;
  float *qpos, *qvel, *time, *aforce, *ncon, *sd;
};

// rsr_physics_dynamics (rsr_dynamics.hpp).  Its buffer, per env, floats: qM [nv*nv] | qfrc_bias [nv] | qfrc_passive [nv] |
// qfrc_actuator [nv] | jac_site_xpos [RSR_MAX_JAC_SITES*3] | jac [RSR_MAX_JAC_SITES][6][nv] (rows jacp x y z, jacr x y z),
// padded to 16 floats.
struct DynLayout { int qM, bias, passive, actuator, sxpos, jac, stride; };
__host__ __device__ inline DynLayout dyn_layout(int nv) {
  DynLayout d;
  d.qM = 0; d.bias = nv * nv; d.passive = d.bias + nv; d.actuator = d.passive + nv; d.sxpos = d.actuator + nv;
  d.jac = d.sxpos + 3 * RSR_MAX_JAC_SITES;
  d.stride = (d.jac + RSR_MAX_JAC_SITES * 6 * nv + 15) & ~15;
  return d;
}
// rsr_physics_constraint (rsr_constraint.hpp).  Its buffer, per env, floats: qfrc_constraint [nv] | qacc [nv] | efc counts [4]
// (nefc, ne, nf, nl) | efc_force [nefc_max] | ncon | contacts [ncon_max][9] (as the side buffer's) | contact wrench [ncon_max][7]
// (normal force, force[3], torque[3]), padded to 16 floats.
struct ConLayout { int qfc, qacc, counts, force, ncon, con, wrench, stride; };
__host__ __device__ inline ConLayout con_layout(int nv, int nefc_max, int ncon_max) {
  ConLayout c;
  c.qfc = 0; c.qacc = nv; c.counts = 2 * nv; c.force = c.counts + 4; c.ncon = c.force + nefc_max; c.con = c.ncon + 1;
  c.wrench = c.con + 9 * ncon_max;
  c.stride = (c.wrench + 7 * ncon_max + 15) & ~15;
  return c;
}
// The launch arguments of OP_PHYS_DYNAMICS (Launch::d)
struct DynArgs {
  float* out;           // the dynamics buffer [N][DynLayout::stride]
  const int* ids;       // [grid] the envs to run, or null: env = workgroup index
  const int* sites;     // [nsite] site ids of the Jacobians (device)
  int nsite;
};
static_assert(sizeof(DynArgs) == 32, "dynamics_kernel's kernel-argument block");
// The launch arguments of OP_PHYS_CONSTRAINT (Launch::c)
struct ConArgs {
  float* out;           // the constraint buffer [N][ConLayout::stride]
  const int* ids;       // [grid] the envs to run, or null: env = workgroup index
};
// rsr_physics_inverse (rsr_inverse.hpp).  Its buffer, per env, floats: qfrc_inverse [nv] | qfrc_constraint [nv] | qacc [nv] |
// qfrc_actuator [nv] | efc counts [4] (nefc, ne, nf, nl) | efc_force [nefc_max], padded to 16 floats.
struct InvLayout { int qfi, qfc, qacc, act, counts, force, stride; };
__host__ __device__ inline InvLayout inv_layout(int nv, int nefc_max) {
  InvLayout i;
  i.qfi = 0; i.qfc = nv; i.qacc = 2 * nv; i.act = 3 * nv; i.counts = 4 * nv; i.force = i.counts + 4;
  i.stride = (i.force + nefc_max + 15) & ~15;
  return i;
}
// The kernel arguments of inverse_kernel.  The launch has no op or Launch field of its own (rsr_launch.hpp is a source of the env
// kernels): it is sent as OP_PHYS_DYNAMICS with a null dynamics buffer (Launch::d.out), the op's unused Launch::p carrying the
// arguments: p.out the inverse buffer, p.ids the envs, p.ctrl the accelerations, p.nsteps the flags, and INVERSE_TAG where a
// sensor table's accelerometer site would stand (inverse_launch_args).  Only a Launch that carries the tag and both pointers is
// read back as an inverse launch (inverse_args); any other dynamics op without a buffer is refused, not launched.
struct InvArgs {
  float* out;           // the inverse buffer [N][InvLayout::stride]
  const int* ids;       // [grid] the envs to run, or null: env = workgroup index
  const float* qacc;    // [N][nv] the accelerations, row e env e's
  int flags;            // RSR_INV_*
};
constexpr int INVERSE_TAG = -0x494e56;          // (no site id is negative but -1, "none")
inline PhysArgs inverse_launch_args(const InvArgs& v) { return PhysArgs{v.qacc, v.out, v.ids, v.flags, nullptr, SensArgs{nullptr, 0, INVERSE_TAG}}; }
// false: p is not what inverse_launch_args makes of a complete InvArgs
inline bool inverse_args(const PhysArgs& p, InvArgs* v) {
  if (p.sens.acc_site != INVERSE_TAG || !p.ctrl || !p.out || p.sd || p.sens.el || p.sens.nsd != 0) return false;
  *v = InvArgs{p.out, p.ids, p.ctrl, p.nsteps};
  return true;
}
// rsr_physics_sample_rollouts (rsr_sample.hpp).  sample_kernel takes a PhysArgs, a RollArgs and K; like the inverse launch it
// has no op or Launch field of its own: it is sent as OP_PHYS_CONSTRAINT with a null constraint buffer (Launch::c.out; the
// constraint entry point always has one).  Launch::p carries the env list, nsteps and the sensor table, with its three buffers
// null; Launch::r ctrl [M][K][T][nu], T and the trajectory rows [M][K][T][w]; and two fields the op never reads carry the rest:
// Launch::fd.flags K, Launch::d.nsite SAMPLE_TAG (sample_launch_args; X is the Launch, which is declared after this file).  Only
// a Launch that carries the tag and a complete set of arguments is read back as a sampled-rollout launch (sample_args); any other
// constraint op without a buffer is refused, not launched.
constexpr int SAMPLE_TAG = -0x534d50;           // (no site count is negative)
template <class X>
inline void sample_launch_args(X& x, const int* ids, const RollArgs& r, int K) {
  x.p.ctrl = nullptr; x.p.out = nullptr; x.p.ids = ids; x.p.sd = nullptr;
  x.r = r;
  x.c = ConArgs{nullptr, nullptr};
  x.d = DynArgs{nullptr, nullptr, nullptr, SAMPLE_TAG};
  x.fd = FdArgs{nullptr, nullptr, nullptr, 0.0f, K};
}
// false: x is not what sample_launch_args makes of complete arguments; otherwise *K
template <class X>
inline bool sample_args(const X& x, int* K) {
  const RollArgs& r = x.r;
  if (x.c.out || x.d.out || x.d.nsite != SAMPLE_TAG || x.fd.out || x.fd.states || x.fd.flags < 1) return false;
  if (x.p.ctrl || x.p.out || x.p.sd || x.p.nsteps < 1 || !r.ctrl || r.T < 1) return false;
  if (!(r.qpos || r.qvel || r.time || r.aforce || r.ncon || r.sd) || (r.sd && x.p.sens.nsd < 1)) return false;
  *K = x.fd.flags;
  return true;
}

}  // namespace rsr
