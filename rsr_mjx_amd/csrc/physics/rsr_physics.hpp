// rsr_physics.hpp -- the physics layer's buffer layouts (side, dynamics, constraint, transition and inverse buffer, nominal scratch) its ops (PhysOp) and their launch
// arguments, one struct per op that needs its own (host and device).
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
// the handle's buffers [N][...], xfrc null = off (PhysLaunch::ap), or one env's rows (AppliedStage, rsr_applied.hpp)
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
// The launch arguments of OP_PHYS_TRANSITION (PhysLaunch::fd)
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
// The launch arguments of OP_PHYS_DYNAMICS (PhysLaunch::d)
struct DynArgs {
  float* out;           // the dynamics buffer [N][DynLayout::stride]
  const int* ids;       // [grid] the envs to run, or null: env = workgroup index
  const int* sites;     // [nsite] site ids of the Jacobians (device)
  int nsite;
};
static_assert(sizeof(DynArgs) == 32, "dynamics_kernel's kernel-argument block");
// The launch arguments of OP_PHYS_CONSTRAINT (PhysLaunch::c)
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
// The launch arguments of OP_PHYS_INVERSE (PhysLaunch::inv)
struct InvArgs {
  float* out;           // the inverse buffer [N][InvLayout::stride]
  const int* ids;       // [grid] the envs to run, or null: env = workgroup index
  const float* qacc;    // [N][nv] the accelerations, row e env e's
  int flags;            // RSR_INV_*
};
// The launch arguments of OP_PHYS_SWEEP (PhysLaunch::sw): what sampled_kernel<.., SweepOp> (rsr_sample.hpp) takes beside SampleOp's arguments
// (PhysArgs p, RollArgs r, and Applied while the forces are on).
struct SweepArgs {
  const float* leaf[RSR_DR_COUNT];   // per-sample leaves [M][K][width], indexed by enum rsr_dr_field; null: the env's own leaf
  int K;                             // samples per slot
  int ctrl_per_sample;               // r.ctrl is [M][K][T][nu]; 0: [M][T][nu], shared by a slot's K samples
  // rsr_physics_feedback_rollouts (rsr_feedback.hpp); fb_gain null: open loop, r.ctrl is applied as it stands
  const float* fb_gain;              // [M][T][nu][2 nv], or with fb_per_sample [M][K][T][nu][2 nv]
  const float* fb_qpos;              // [..][T][nq]
  const float* fb_qvel;              // [..][T][nv]
  float* ctrl_out;                   // [M][K][T][nu] the applied ctrl, or null
  int fb_per_sample;                 // the three feedback rows are per sample
  int fb_clamp;                      // clamp to actuator_ctrlrange where actuator_ctrllimited
};
// rsr_physics_trajectory_fd (rsr_trajectory.hpp), both of its launches (PhysLaunch::tj).  The nominal scratch, per (slot, t),
// floats: qpos [nq] | qvel [nv] | qacc_warmstart [nv], the state before control step t: written by nominal_kernel, read by
// trajectory_fd_kernel.  Every row of ctrl and of the caller's buffers is indexed by slot.
struct TrajArgs {
  const float* ctrl;    // [M][T][nu]
  int T;
  float* nominal;       // the handle's scratch [M][T][nq + 2 nv]
  float *qpos, *qvel;   // the nominal rows [M][T+1][nq] / [M][T+1][nv], each null = not recorded (OP_TRAJ_NOMINAL)
  float* columns;       // [M][T][ncol][2 nv + nsd], tight rows (OP_TRAJ_FD)
  float eps;
  int flags;            // RSR_FD_CENTERED or 0
};
// rsr_physics_lqr_backward (rsr_lqr.hpp): the caller's buffers, every row indexed by slot (PhysLaunch::lq).  nx = 2 nv.
struct LqrArgs {
  const float* columns; // [M][T][nx + nu][row_stride], entries >= nx of a row are not read
  int row_stride, T;
  const float *lx, *lu, *lxx, *luu;   // [M][T+1][nx], [M][T][nu], [M][T+1][nx][nx], [M][T][nu][nu]
  const float* lux;     // [M][T][nu][nx], or null: zero
  const float* mu;      // [M]
  int flags;            // RSR_LQR_REG_STATE or 0
  float *gain, *k, *dv, *status;      // [M][T][nu][nx], [M][T][nu], [M][2], [M]
  float *vx, *vxx;      // [M][T+1][nx], [M][T+1][nx][nx], each null = not recorded
};
// rsr_physics_lqr_box (box_backward_kernel, rsr_lqr.hpp): the plain pass's arguments and the bounds on k_t (PhysLaunch::bx)
struct BoxArgs {
  LqrArgs lq;
  const float *lo, *hi; // [M][T][nu], -inf / +inf: no bound
  float* clamped;       // [M][T][nu] -1 at lo, +1 at hi, 0 free, or null
  float* qp;            // [M][T][2] Newton steps taken, code, or null
  int max_iter;         // 1 .. 64
};
// rsr_physics_ik (rsr_ik.hpp): the caller's buffers, every row indexed by slot, and the task table by value (PhysLaunch::ik): the
// op has no device table and no state in the handle.
struct IkArgs {
  const float* target_pos;   // [M][nsite][3]
  const float* target_quat;  // [M][nsite][4] (w, x, y, z), or null: no orientation row
  const float* qpos0;        // [M][nq] the starts, or null: the record's qpos of the slot's env
  const float* damping;      // [M]
  const int* ids;            // [M] the env of every slot, or null: env = slot
  float* qpos;               // [M][nq]
  float* err;                // [M][2] perr, rerr at the returned qpos
  int* info;                 // [M][2] iterations taken, status
  int sites[RSR_MAX_JAC_SITES];
  float wp[RSR_MAX_JAC_SITES], wr[RSR_MAX_JAC_SITES];   // row weights, 0 = off
  unsigned dofs;             // bit i: dof i may move
  int nsite, iters, limits;
  float tol_pos, tol_rot, max_step;
};
static_assert(sizeof(IkArgs) == 64 + 12 * RSR_MAX_JAC_SITES + 32, "ik_kernel's kernel-argument block");
// rsr_physics_cost_rollouts (rsr_cost.hpp): what sampled_kernel<.., CostOp> takes beside SweepOp's arguments (PhysLaunch::cs).  The
// references and weights are rows [M][T][w] by slot, shared by a slot's K samples; the outputs are rows by (slot, sample).
struct CostArgs {
  const float *qpos_ref, *qvel_ref, *ctrl_ref, *sensor_ref;   // [M][T][nq | nv | nu | nsd]; qvel / ctrl / sensor null: zeros
  const float *w_qpos, *w_qvel, *w_ctrl, *w_sensor;           // [M][T][nv | nv | nu | nsd]; null: the term is off
  float* cost;          // [M][K]
  float* step_cost;     // [M][K][T], or null
  float* terms;         // [M][K][4] (qpos, qvel, ctrl, sensor), or null
  float* dx;            // [M][K][T][2 nv] dq | dv, or null
  float* ctrl_out;      // [M][K][T][nu] the applied ctrl, or null (sw.ctrl_out stays null: the cost stage writes the row)
};
static_assert(sizeof(CostArgs) == 13 * sizeof(void*), "the cost op's kernel-argument block");
// rsr_physics_kalman (rsr_kalman.hpp): the caller's buffers, every row indexed by slot (PhysLaunch::kf).  nx = 2 nv.
struct KalmanArgs {
  const float* columns; // [M][T][nx + nu][row_stride]: of row j < nx the entries i < nx (A_t[i][j]) and nx + r, r < ny (C_t[r][j])
  int row_stride, T, ny;
  const float *dy, *r, *q;            // [M][T][ny], [M][T][ny] (+inf: missing), [M][T][nx]
  const float* x0;      // [M][nx], or null: zeros
  const float* P0;      // [M][nx][nx]
  float *xf, *pf;       // [M][T+1][nx], [M][T+1][nx][nx] (null = not recorded; needed by the smoother)
  float *xs, *ps;       // [M][T+1][nx] (null: no smoother), [M][T+1][nx][nx] (null = not recorded)
  float *nll, *status;  // [M] (null = not recorded), [M][2]
};
// rsr_physics_cost_expand (rsr_expand.hpp): the caller's buffers, every row indexed by slot (PhysLaunch::ex).  nx = 2 nv.
struct ExpandArgs {
  const float* columns; // [M][T][nx + nu][row_stride]: of every row the entries nx + j, j < ny (C_t | D_t); null without w_sensor
  int row_stride, T, ny;
  const float *ctrl_ref, *sensor_ref;                    // [M][T][nu | ny], each null: zeros
  const float *w_qpos, *w_qvel, *w_ctrl, *w_sensor;      // [M][T][nv | nv | nu | ny]; null: the term is off
  const float *dx, *ctrl, *sensordata;                   // [M][T][nx | nu | ny] the residual sources on the nominal run
  float *lx, *lu, *lxx, *luu, *lux;                      // [M][T+1][nx], [M][T][nu], [M][T+1][nx][nx], [M][T][nu][nu], [M][T][nu][nx]
};

// The physics ops of a family unit's launch entry (launch_physics, rsr_physics_kernels.hpp).  An entry takes its op as an int, of
// enum Op (rsr_launch.hpp) or of this enum: these start above enum Op's, so that no value names two ops.  A new op is a member
// here, a field of PhysLaunch if it needs one, and a case of launch_physics: nothing outside physics/ changes.
enum PhysOp {
  OP_PHYS_FORWARD = 64,  // rsr_physics_forward[_envs] (p): grid = envs or listed envs (p.ids)
  OP_PHYS_STEP,          // rsr_physics_step (p)
  OP_PHYS_ROLLOUT,       // rsr_physics_rollout (p, r)
  OP_PHYS_DYNAMICS,      // rsr_physics_dynamics (d): grid = envs or listed envs (d.ids)
  OP_PHYS_CONSTRAINT,    // rsr_physics_constraint (c): grid = envs or listed envs (c.ids)
  OP_PHYS_TRANSITION,    // rsr_physics_transition_fd (p, fd): grid = envs x columns, or listed envs (fd.ids) x columns
  OP_PHYS_INVERSE,       // rsr_physics_inverse (inv): grid = envs or listed envs (inv.ids)
  OP_PHYS_SAMPLE,        // rsr_physics_sample_rollouts (p, r, K): grid = envs x K, or listed envs (p.ids) x K; r.ctrl [M][K][T][nu],
                         // the trajectory rows [M][K][T][w]
  OP_PHYS_SWEEP,         // rsr_physics_param_rollouts and rsr_physics_feedback_rollouts (p, r, sw): grid and rows as OP_PHYS_SAMPLE's;
                         // r.ctrl [M][K][T][nu] or [M][T][nu]
  OP_TRAJ_NOMINAL,       // rsr_physics_trajectory_fd, first launch (p, tj): grid = envs or listed envs (p.ids)
  OP_TRAJ_FD,            // rsr_physics_trajectory_fd, second launch (p, tj): grid = envs x T x columns, or listed envs (p.ids) x T x columns
  OP_LQR_BACKWARD,       // rsr_physics_lqr_backward (lq): grid = slots; reads neither the model nor the record
  OP_IK,                 // rsr_physics_ik (ik): grid = slots, the env of a slot from ik.ids
  OP_COST_ROLLOUTS,      // rsr_physics_cost_rollouts (p, r, sw, cs): grid and rows as OP_PHYS_SWEEP's
  OP_KALMAN,             // rsr_physics_kalman (kf): grid = slots; reads neither the model nor the record
  OP_BOX_BACKWARD,       // rsr_physics_lqr_box (bx): grid = slots; reads neither the model nor the record
  OP_EXPAND,             // rsr_physics_cost_expand (ex): grid = slots x (T + 1); reads neither the model nor the record
};
// The physics ops' arguments (Launch::ph), one field per op that needs its own
struct PhysLaunch {
  PhysArgs p;           // OP_PHYS_FORWARD, OP_PHYS_STEP, OP_PHYS_ROLLOUT, OP_PHYS_TRANSITION, OP_PHYS_SAMPLE, OP_PHYS_SWEEP, OP_TRAJ_*
  RollArgs r;           // OP_PHYS_ROLLOUT, OP_PHYS_SAMPLE, OP_PHYS_SWEEP
  DynArgs d;            // OP_PHYS_DYNAMICS
  ConArgs c;            // OP_PHYS_CONSTRAINT
  FdArgs fd;            // OP_PHYS_TRANSITION
  InvArgs inv;          // OP_PHYS_INVERSE
  int K;                // OP_PHYS_SAMPLE: the control sequences per env
  SweepArgs sw;         // OP_PHYS_SWEEP
  TrajArgs tj;          // OP_TRAJ_NOMINAL, OP_TRAJ_FD
  LqrArgs lq;           // OP_LQR_BACKWARD
  IkArgs ik;            // OP_IK
  CostArgs cs;          // OP_COST_ROLLOUTS (with p, r and sw)
  KalmanArgs kf;        // OP_KALMAN
  BoxArgs bx;           // OP_BOX_BACKWARD
  ExpandArgs ex;        // OP_EXPAND
  Applied ap;           // the ops that take p or c: the applied forces, or ap.xfrc null: none (the plain kernels)
};

}  // namespace rsr
