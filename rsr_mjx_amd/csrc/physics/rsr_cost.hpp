// rsr_cost.hpp -- rsr_physics_cost_rollouts (include/rsr_physics.h): the rollout of rsr_physics_param_rollouts, or with the gain
// rows set of the closed-loop call, and the running cost of every sample formed where its state is: in the wave's LDS at the
// control-step boundary.  What MPPI, predictive sampling and CEM reduce a trajectory to, what an iLQR line search compares and what
// system identification minimises: a weighted least-squares tracking cost per (slot, sample), with nothing of the trajectory
// written to memory unless the caller asks for it.
//
// cost_stage is what sampled_kernel's COST switch adds to the (slot, sample) loop (rsr_sample.hpp, which includes this header).  At
// the end of control step t, after sensor_stage and the rows of the trajectory and before the next ctrl row overwrites s.ctrl,
// it takes the residuals against row (slot, t) of the references, one lane per entry:
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

// LDS of a cost-rollout workgroup (sampled_kernel<.., CostOp>): Smem<C>, then the accumulators cost | qpos | qvel | ctrl | sensor term (padded to 8 floats)
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

}  // namespace rsr
