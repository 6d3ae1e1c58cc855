// rsr_physics_kernels.hpp -- the physics-level kernels (include/rsr_physics.h): each family unit instantiates them for its Dims,
// with its flags and next to its env kernels, and launches them through launch_physics.  One body per kind, physics_kernel (step and
// forward), rollout_kernel, dynamics_kernel (rsr_dynamics.hpp), constraint_kernel (rsr_constraint.hpp), transition_kernel
// (rsr_transition.hpp), inverse_kernel (rsr_inverse.hpp), sampled_kernel (rsr_sample.hpp: one body, three ops) and the two
// of rsr_trajectory.hpp, nominal_kernel and trajectory_fd_kernel, lqr_kernel with box_backward_kernel (rsr_lqr.hpp, one body), kalman_kernel (rsr_kalman.hpp) and expand_kernel (rsr_expand.hpp), which run
// no physics and take of a family only nv and nu, and ik_kernel (rsr_ik.hpp), which runs the kinematics and mass-matrix stages
// alone; all but dynamics_kernel, inverse_kernel, lqr_kernel, kalman_kernel, expand_kernel and ik_kernel are instantiated plain and with applied forces:
// the applied kernels take the handle's Applied buffers as one more argument and pass forward<C> their env's rows as its force
// stage (rsr_applied.hpp).
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_sensors.hpp"
#include "rsr_applied.hpp"
#include "rsr_dynamics.hpp"
#include "rsr_constraint.hpp"
#include "rsr_transition.hpp"
#include "rsr_inverse.hpp"
#include "rsr_sample.hpp"
#include "rsr_sweep.hpp"
#include "rsr_trajectory.hpp"
#include "rsr_lqr.hpp"
#include "rsr_kalman.hpp"
#include "rsr_ik.hpp"
#include "rsr_cost.hpp"
#include "rsr_expand.hpp"

namespace rsr {

// ================================================================ physics-only kernels (rsr_physics_step / rsr_physics_forward)
// mjx_env.step(model, data, ctrl, n_substeps) and mjx_env.init's mjx.forward (reference _src/mjx_env.py:30-73) on the record's
// pipeline state: no env prologue / epilogue, no wrappers, no PRNG.  The per-env model leaves of the batch apply.  One wave per env,
// a plain launch.  Each family's physics kernels are built in the unit of its env kernels (same flags, same inlined stages): the
// substeps compile to the same arithmetic as inside rsr_step, and a physics step is bit-identical to the env step it stands in for
// (tests/test_physics_gpu.py).
//

// the side buffer row of env e from the last forward pass (qacc_i: this lane's qacc of that pass)
template <class C>
__device__ __forceinline__ void store_side(const DModel& m, const Smem<C>& s, float* out, int e, int lane, float qacc_i) {
  const PhysLayout PL = phys_layout(C::NV, C::NU, C::NB, C::NCON);
  float* o = out + (size_t)e * PL.stride;
  if (lane < C::NV) o[PL.qacc + lane] = qacc_i;
  if (lane < C::NU) o[PL.aforce + lane] = s.aforce[lane];
  for (int t = lane; t < C::NB * 4; t += 64) o[PL.xquat + t] = s.xquat[t];
  const int nc = s.ncon;
  for (int c = lane; c < C::NCON; c += 64) {
    float* w = o + PL.con + 9 * c;
    const bool on = c < nc;
    const int pr = on ? s.cpair[c] : 0;
    w[0] = on ? s.cdist[c] : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { w[1 + k] = on ? s.cpos[3 * c + k] : 0.0f; w[4 + k] = on ? s.cnrm[3 * c + k] : 0.0f; }
    w[7] = on ? (float)m.pair_geom1[pr] : -1.0f; w[8] = on ? (float)m.pair_geom2[pr] : -1.0f;
  }
  if (lane == 0) { o[PL.ncon] = (float)nc; o[PL.ncon_drop] = (float)s.ncon_drop; }
}

// STEP: nsteps x (forward, integrate); otherwise one forward.  Position-dependent outputs (xpos, xquat, site_xpos, contacts) are
// those of the last forward pass, i.e. before the final integration (MJX Data semantics, as in the record after rsr_step).
// Ap: none (the plain kernel), or Applied: the applied forces ([N][nbody*6] / [N][nv]) enter every forward pass.
template <class C, bool STEP, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void physics_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, Ap... ap) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = p.ids ? p.ids[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  if (e < 0 || e >= a.n) return;                                // (an id out of range runs nothing)
  float* rec = a.state + (size_t)e * L.rec;
  const auto stage = force_stage<C>(e, ap.xfrc..., ap.qfrc...);
  PROF_DECL
  // the record load is written out here and in rollout_kernel: through load_pipeline or a helper of its own it compiles to
  // other code
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float warm = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  float time = rec[L.time];
  load_overrides<C>(m, s, a, e, lane);
  if (lane < C::NU) s.ctrl[lane] = p.ctrl ? p.ctrl[(size_t)e * C::NU + lane] : rec[L.ctrl + lane];
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle (the joystick's kick is env logic; applied forces are the
                                  // force stage); the accelerometer's body as in the env kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  WSYNC();
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsteps = STEP ? p.nsteps : 1;
  for (int fr = 0; fr < nsteps; ++fr) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS, stage);
    if constexpr (STEP) {
      integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
      time += hot.timestep;
    }
  }
  WSYNC();
  if (p.sens.nsd > 0) {                                          // (wave-uniform; no table: the stage is skipped)
    const float v = sensor_stage<C>(m, s, lane, f.qacc, p.sens);
    if (lane < p.sens.nsd) p.sd[(size_t)e * RSR_MAX_SENSORDATA + lane] = v;
  }
  if constexpr (STEP) store_pipeline<C>(s, rec, L, lane, warm, time);
  else {                          // mjx.forward leaves qpos as it was (kinematics normalises the quaternions in LDS only)
    if (lane < C::NV) rec[L.warm + lane] = warm;
    for (int t = lane; t < C::NB * 3; t += 64) rec[L.xpos + t] = s.xpos[t];
    for (int t = lane; t < C::NS * 3; t += 64) rec[L.site_xpos + t] = s.spos[t];
  }
  if (p.out) store_side<C>(m, s, p.out, e, lane, f.qacc);
}

// rsr_physics_rollout: T control steps of physics_kernel<C, true> in one launch.  The state stays in LDS and the warm start in its
// register from one control step to the next (in physics_kernel both make a round trip through the record, which is exact), so
// the trajectory is bit-identical to T step launches.  After control step t the wave writes its rows t of the requested
// trajectories: per env the rows are contiguous in time ([N][T][w]).  The record, the side buffer and the sensordata row are
// written once, at the end, as physics_kernel<C, true> writes them.  Applied forces (Ap) are held for all T control steps.
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void rollout_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, RollArgs r, Ap... ap) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = (int)blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  float* rec = a.state + (size_t)e * L.rec;
  const auto stage = force_stage<C>(e, ap.xfrc..., ap.qfrc...);
  PROF_DECL
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float warm = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  float time = rec[L.time];
  load_overrides<C>(m, s, a, e, lane);
  if constexpr (C::XFRC) {
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsd = p.sens.nsd;
  // one loop over the T * nsteps substeps, as in physics_kernel, the control-step boundary a wave-uniform branch (a loop over
  // control steps around the substep loop spills 19 VGPRs of the Go2 kernels at their 128-register budget, this 13: DESIGN.md 4c)
  if (lane < C::NU) s.ctrl[lane] = r.ctrl[(size_t)e * r.T * C::NU + lane];
  WSYNC();
  const int total = r.T * p.nsteps;
  int t = 0, fr = 0;
  for (int k = 0; k < total; ++k) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS, stage);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    time += hot.timestep;
    if (++fr < p.nsteps) continue;
    fr = 0;
    WSYNC();
    const size_t row = (size_t)e * r.T + t;
    float sv = 0.0f;
    if (nsd > 0) {
      sv = sensor_stage<C>(m, s, lane, f.qacc, p.sens);
      if (t == r.T - 1 && lane < nsd) p.sd[(size_t)e * RSR_MAX_SENSORDATA + lane] = sv;      // the view: the last control step's
    }
    if (r.qpos) for (int q = lane; q < C::NQ; q += 64) r.qpos[row * C::NQ + q] = s.qpos[q];
    if (r.qvel && lane < C::NV) r.qvel[row * C::NV + lane] = s.qvel[lane];
    if (r.time && lane == 0) r.time[row] = time;
    if (r.aforce && lane < C::NU) r.aforce[row * C::NU + lane] = s.aforce[lane];
    if (r.ncon && lane == 0) r.ncon[row] = (float)s.ncon;
    if (r.sd && lane < nsd) r.sd[row * nsd + lane] = sv;
    if (++t < r.T) {
      if (lane < C::NU) s.ctrl[lane] = r.ctrl[(row + 1) * C::NU + lane];
      WSYNC();
    }
  }
  store_pipeline<C>(s, rec, L, lane, warm, time);
  if (p.out) store_side<C>(m, s, p.out, e, lane, f.qacc);
}

// the physics ops (PhysOp, rsr_physics.hpp) of a family's launch entry, one case each; -1: not one of them (nothing is launched)
static_assert((int)OP_STEP_OCCUPANCY < (int)OP_PHYS_FORWARD, "an entry takes an Op or a PhysOp as one int: the values must not meet");
template <class C, int WAVES>
int launch_physics(int op, const Launch& x) {
  // (the LDS of the transition and of the trajectory's columns: Smem<C> and the words the first run's end state waits in; the
  // backward pass has an image of its own, LqrDims<C>, the control-limited one BoxDims<C> behind it; inverse kinematics adds IkDims<C> behind Smem<C>, the cost rollouts their
  // accumulators; the Kalman filter and smoother have an image of their own, KalmanDims<C>, and so has the cost expansion, ExpandDims<C>)
  const size_t lds = op == OP_COST_ROLLOUTS ? cost_lds_bytes<C>() : op == OP_IK ? ik_lds_bytes<C>() : op == OP_EXPAND ? expand_lds_bytes<C>() : op == OP_KALMAN ? kalman_lds_bytes<C>(x.ph.kf.xs != nullptr) : op == OP_LQR_BACKWARD ? lqr_lds_bytes<C>() : op == OP_BOX_BACKWARD ? box_lds_bytes<C>() : op == OP_TRAJ_FD || op == OP_PHYS_TRANSITION ? fd_lds_bytes<C>() : sizeof(Smem<C>);
  auto go = [&](auto kernel, auto... args) { hipLaunchKernelGGL(kernel, dim3(x.grid), dim3(64), lds, x.stream, x.dm, x.L, x.a, args...); return 0; };
  const PhysLaunch& ph = x.ph;
  const bool ap = ph.ap.xfrc != nullptr;     // applied forces on
  // the two launches of rsr_physics_trajectory_fd (rsr_trajectory.hpp)
  if (op == OP_TRAJ_NOMINAL) return ap ? go(nominal_kernel<C, WAVES, Applied>, ph.p, ph.tj, ph.ap) : go(nominal_kernel<C, WAVES>, ph.p, ph.tj);
  if (op == OP_TRAJ_FD) return ap ? go(trajectory_fd_kernel<C, WAVES, Applied>, ph.p, ph.tj, ph.ap) : go(trajectory_fd_kernel<C, WAVES>, ph.p, ph.tj);
  if (op == OP_LQR_BACKWARD) return go(lqr_kernel<C, WAVES>, ph.lq);      // rsr_physics_lqr_backward (rsr_lqr.hpp)
  if (op == OP_BOX_BACKWARD) return go(box_backward_kernel<C, WAVES>, ph.bx);   // rsr_physics_lqr_box (rsr_lqr.hpp)
  if (op == OP_IK) return go(ik_kernel<C, WAVES>, ph.ik);                 // rsr_physics_ik (rsr_ik.hpp)
  if (op == OP_KALMAN) return go(kalman_kernel<C, WAVES>, ph.kf);         // rsr_physics_kalman (rsr_kalman.hpp)
  if (op == OP_EXPAND) return go(expand_kernel<C, WAVES>, ph.ex);         // rsr_physics_cost_expand (rsr_expand.hpp)
  // rsr_physics_cost_rollouts (rsr_sample.hpp, rsr_cost.hpp)
  if (op == OP_COST_ROLLOUTS) return ap ? go(sampled_kernel<C, WAVES, CostOp, Applied>, ph.p, ph.r, CostOp::Args{ph.sw, ph.cs}, ph.ap) : go(sampled_kernel<C, WAVES, CostOp>, ph.p, ph.r, CostOp::Args{ph.sw, ph.cs});
  switch (op) {
    case OP_PHYS_STEP: return ap ? go(physics_kernel<C, true, WAVES, Applied>, ph.p, ph.ap) : go(physics_kernel<C, true, WAVES>, ph.p);
    case OP_PHYS_FORWARD: return ap ? go(physics_kernel<C, false, WAVES, Applied>, ph.p, ph.ap) : go(physics_kernel<C, false, WAVES>, ph.p);
    case OP_PHYS_ROLLOUT: return ap ? go(rollout_kernel<C, WAVES, Applied>, ph.p, ph.r, ph.ap) : go(rollout_kernel<C, WAVES>, ph.p, ph.r);
    case OP_PHYS_TRANSITION: return ap ? go(transition_kernel<C, WAVES, Applied>, ph.p, ph.fd, ph.ap) : go(transition_kernel<C, WAVES>, ph.p, ph.fd);
    case OP_PHYS_DYNAMICS: return go(dynamics_kernel<C, WAVES>, ph.d);      // (applied forces enter none of its outputs, nor the inverse's)
    case OP_PHYS_CONSTRAINT: return ap ? go(constraint_kernel<C, WAVES, Applied>, ph.c, ph.ap) : go(constraint_kernel<C, WAVES>, ph.c);
    case OP_PHYS_INVERSE: return go(inverse_kernel<C, WAVES>, ph.inv);
    case OP_PHYS_SAMPLE: return ap ? go(sampled_kernel<C, WAVES, SampleOp, Applied>, ph.p, ph.r, ph.K, ph.ap) : go(sampled_kernel<C, WAVES, SampleOp>, ph.p, ph.r, ph.K);
    case OP_PHYS_SWEEP: return ap ? go(sampled_kernel<C, WAVES, SweepOp, Applied>, ph.p, ph.r, ph.sw, ph.ap) : go(sampled_kernel<C, WAVES, SweepOp>, ph.p, ph.r, ph.sw);
    default: return -1;
  }
}

}  // namespace rsr
