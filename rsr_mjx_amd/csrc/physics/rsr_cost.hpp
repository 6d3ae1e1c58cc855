// rsr_cost.hpp -- rsr_physics_cost_rollouts (include/rsr_physics.h): the rollout of rsr_physics_param_rollouts, or with the gain
// rows set of the closed-loop call, and the running cost of every sample formed where its state is: in the wave's LDS at the
// control-step boundary.  What MPPI, predictive sampling and CEM reduce a trajectory to, what an iLQR line search compares and what
// system identification minimises: a weighted least-squares tracking cost per (slot, sample), with nothing of the trajectory
// written to memory unless the caller asks for it.
//
// One wave per (slot, sample): sweep_kernel's launch shape and loop (rsr_sweep.hpp), restated statement for statement as that
// kernel restates sample_kernel, with one stage more.  At the end of control step t, after sensor_stage and the rows of the
// trajectory and before the next ctrl row overwrites s.ctrl, cost_stage takes the residuals against row (slot, t) of the
// references, one lane per entry:
//   dq = qpos (-) qpos_ref   differentiate_pos with zero_at_equal, negated as feedback_ctrl negates it     lane < NV
//   dv = qvel - qvel_ref                                                                                   lane < NV
//   du = s.ctrl - ctrl_ref   the control that was applied, after the gain rows and the clamp                lane < NU
//   ds = sensordata - sensor_ref   the value sensor_stage has just returned                                lane < nsd
// and forms, with no contraction (every product and every sum rounds once),
//   lane:  p = (((w_qpos dq) dq + (w_qvel dv) dv) + (w_ctrl du) du) + (w_sensor ds) ds    a term that is off, or a lane past its
//                                                                                         width, adds +0
//   step:  c_t = 0.5 wave_sum(p)            the project's wave_sum: the same pairing of the 64 lanes in every launch
//   cost:  acc = acc + c_t                  from acc = +0, t = 0 .. T-1
// The four term sums (rsr_cost_out::terms) are 0.5 wave_sum of each lane product alone, accumulated the same way.  The
// accumulators are five words of LDS behind Smem<C> that lane 0 alone adds to (cost_lds_bytes): the Airbot kernels have no
// register to carry across forward<C>.  A sample's numbers depend on its own inputs only: the optional outputs add stores and,
// for the terms, sums of their own, never a change to the arithmetic of another output.
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_sensors.hpp"
#include "rsr_applied.hpp"
#include "rsr_sweep.hpp"

namespace rsr {

// LDS of a cost_kernel workgroup: Smem<C>, then the accumulators cost | qpos | qvel | ctrl | sensor term (padded to 8 floats)
template <class C>
constexpr size_t cost_acc_offset() { return (sizeof(Smem<C>) + 15) & ~size_t(15); }
template <class C>
constexpr size_t cost_lds_bytes() { return cost_acc_offset<C>() + 8 * sizeof(float); }

// The residuals and the cost of one control step, from the state in s.qpos / s.qvel, the applied control in s.ctrl and this
// lane's sensordata value sv.  ref_row: row (slot, t) of the references and weights; row: row (slot, sample, t) of the outputs;
// b: the workgroup, row of cost and terms, written when `last`.  Called by all 64 lanes in wave-uniform code, after a fence that
// follows integrate; every null check is on a kernel argument.  Every global load is issued before the first use, so that the
// rows cost one round trip; a pointer that is null, or whose term is off, is not read.
template <class C>
__device__ __forceinline__ void cost_stage(const Hot& hot, const Smem<C>& s, float* acc, const CostArgs& c, size_t ref_row, size_t row,
                                           size_t b, bool last, int lane, float sv, int nsd) {
#pragma clang fp contract(off)
  static_assert(C::NQ <= 64 && C::NV <= 64 && C::NU <= 64 && RSR_MAX_SENSORDATA <= 64, "one lane per entry of the state, of ctrl and of sensordata");
  const bool need_dq = c.qpos_ref && (c.w_qpos || c.dx), need_dv = c.w_qvel || c.dx;
  const int iq = lane < C::NQ ? lane : 0, iv = lane < C::NV ? lane : 0, iu = lane < C::NU ? lane : 0, is = lane < nsd ? lane : 0;
  float yq = 0.0f, yv = 0.0f, yu = 0.0f, ys = 0.0f, wq = 0.0f, wv = 0.0f, wu = 0.0f, ws = 0.0f;
  if (need_dq) yq = ((gp_f)(c.qpos_ref + ref_row * (size_t)C::NQ))[iq];
  if (need_dv && c.qvel_ref) yv = ((gp_f)(c.qvel_ref + ref_row * (size_t)C::NV))[iv];
  if (c.w_ctrl && c.ctrl_ref) yu = ((gp_f)(c.ctrl_ref + ref_row * (size_t)C::NU))[iu];
  if (c.w_sensor && c.sensor_ref) ys = ((gp_f)(c.sensor_ref + ref_row * (size_t)nsd))[is];
  if (c.w_qpos) wq = ((gp_f)(c.w_qpos + ref_row * (size_t)C::NV))[iv];
  if (c.w_qvel) wv = ((gp_f)(c.w_qvel + ref_row * (size_t)C::NV))[iv];
  if (c.w_ctrl) wu = ((gp_f)(c.w_ctrl + ref_row * (size_t)C::NU))[iu];
  if (c.w_sensor) ws = ((gp_f)(c.w_sensor + ref_row * (size_t)nsd))[is];
  float dq = 0.0f, dv = 0.0f;
  if (need_dq) {                                 // (the helper gives ref (-) qpos; the negation is exact.  All lanes: it shuffles)
    const float d = -differentiate_pos<C>(hot, s, lane, lane < C::NQ ? yq : 0.0f, true);
    dq = lane < C::NV ? d : 0.0f;
  }
  if (need_dv) dv = lane < C::NV ? s.qvel[iv] - yv : 0.0f;
  const float du = c.w_ctrl && lane < C::NU ? s.ctrl[iu] - yu : 0.0f;
  const float ds = c.w_sensor && lane < nsd ? sv - ys : 0.0f;
  // a lane past a term's width holds d = 0 and a finite weight of another lane: +0
  const float pq = c.w_qpos && lane < C::NV ? (wq * dq) * dq : 0.0f;
  const float pv = c.w_qvel && lane < C::NV ? (wv * dv) * dv : 0.0f;
  const float pu = c.w_ctrl && lane < C::NU ? (wu * du) * du : 0.0f;
  const float ps = c.w_sensor && lane < nsd ? (ws * ds) * ds : 0.0f;
  const float ct = 0.5f * wave_sum(((pq + pv) + pu) + ps);
  if (lane == 0) acc[0] = acc[0] + ct;
  if (c.terms) {
    const float tq = 0.5f * wave_sum(pq), tv = 0.5f * wave_sum(pv), tu = 0.5f * wave_sum(pu), ts = 0.5f * wave_sum(ps);
    if (lane == 0) { acc[1] = acc[1] + tq; acc[2] = acc[2] + tv; acc[3] = acc[3] + tu; acc[4] = acc[4] + ts; }
  }
  if (c.step_cost && lane == 0) c.step_cost[row] = ct;
  if (c.dx && lane < C::NV) { c.dx[row * (2 * C::NV) + lane] = dq; c.dx[row * (2 * C::NV) + C::NV + lane] = dv; }
  if (c.ctrl_out && lane < C::NU) c.ctrl_out[row * C::NU + lane] = s.ctrl[lane];
  if (last && lane == 0) {
    c.cost[b] = acc[0];
    if (c.terms) { c.terms[4 * b] = acc[1]; c.terms[4 * b + 1] = acc[2]; c.terms[4 * b + 2] = acc[3]; c.terms[4 * b + 3] = acc[4]; }
  }
}

// Workgroup b: slot b / K (env p.ids[slot], or slot), sample b % K, K = sw.K.  p, r, sw: as sweep_kernel takes them (sw.ctrl_out is
// null; every pointer of r may be).  c: the references and weights [M][T][w] by slot, and the outputs by (slot, sample).
// Ap: none, or Applied: the env's applied forces enter every pass, held for all T control steps.
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void cost_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, RollArgs r, SweepArgs sw, CostArgs c, Ap... ap) {
  static_assert(4 * WAVES * cost_lds_bytes<C>() <= 160 * 1024, "4 x WAVES workgroups share a CU's LDS");
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  float* acc = reinterpret_cast<float*>(smem_raw + cost_acc_offset<C>());
  const int K = sw.K;
  const int b = (int)blockIdx.x, slot = b / K, lane = threadIdx.x;
  const int e = p.ids ? p.ids[slot] : slot;
  if (e < 0 || e >= a.n) return;                                // (an id out of range runs nothing)
  const float* rec = a.state + (size_t)e * L.rec;
  const auto stage = force_stage<C>(e, ap.xfrc..., ap.qfrc...);
  PROF_DECL
  // the record load of rollout_kernel, written out
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float warm = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  float time = rec[L.time];
  load_overrides<C>(m, s, a, e, lane);
  overlay_leaves<C>(m, s, sw, b, lane);          // the sample's leaves over the env's own (same lanes, same words: no fence between)
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  if (lane < 8) acc[lane] = 0.0f;                // (published to lane 0 by the fence below)
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsd = p.sens.nsd;
  // the slot's ctrl rows, or the sample's (uniform over the launch)
  const size_t cb = sw.ctrl_per_sample ? (size_t)b : (size_t)slot;
  // one loop over the T * nsteps substeps, the control-step boundary a wave-uniform branch, as in rollout_kernel
  if (lane < C::NU) s.ctrl[lane] = r.ctrl[cb * r.T * C::NU + lane];
  if (sw.fb_gain) feedback_ctrl<C>(m, hot, s, sw, (sw.fb_per_sample ? (size_t)b : (size_t)slot) * r.T, (size_t)b * r.T, lane);
  WSYNC();
  const int total = r.T * p.nsteps;              // (T * nsteps < 2^31: rsr_physics_cost_rollouts)
  int t = 0, fr = 0;
  for (int k = 0; k < total; ++k) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS, stage);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    time += hot.timestep;
    if (++fr < p.nsteps) continue;
    fr = 0;
    WSYNC();
    const int lt = lrec_lane(lane);            // opaque, as in sample_kernel: the rows' addresses are formed here, not kept across
                                               // the solver
    const size_t row = (size_t)b * r.T + t;
    float sv = 0.0f;
    if (nsd > 0) sv = sensor_stage<C>(m, s, lt, f.qacc, p.sens);      // (wave-uniform; no table: the stage is skipped)
    if (r.qpos) for (int q = lt; q < C::NQ; q += 64) r.qpos[row * C::NQ + q] = s.qpos[q];
    if (r.qvel && lt < C::NV) r.qvel[row * C::NV + lt] = s.qvel[lt];
    if (r.time && lt == 0) r.time[row] = time;
    if (r.aforce && lt < C::NU) r.aforce[row * C::NU + lt] = s.aforce[lt];
    if (r.ncon && lt == 0) r.ncon[row] = (float)s.ncon;
    if (r.sd && lt < nsd) r.sd[row * nsd + lt] = sv;
    // s.ctrl still holds the control of this step: the next row is loaded below
    cost_stage<C>(hot, s, acc, c, (size_t)slot * r.T + t, row, (size_t)b, t == r.T - 1, lt, sv, nsd);
    if (++t < r.T) {
      if (lt < C::NU) s.ctrl[lt] = r.ctrl[(cb * r.T + t) * C::NU + lt];
      if (sw.fb_gain) feedback_ctrl<C>(m, hot, s, sw, (sw.fb_per_sample ? (size_t)b : (size_t)slot) * r.T + t, (size_t)b * r.T + t, lt);
      WSYNC();
    }
  }
}

}  // namespace rsr
