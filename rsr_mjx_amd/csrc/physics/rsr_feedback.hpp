// rsr_feedback.hpp -- the control law of rsr_physics_feedback_rollouts (include/rsr_physics.h): affine state feedback computed on
// the device at every control-step boundary of sampled_kernel's SWEEP switch (rsr_sample.hpp), from the sample's own state in LDS:
//   u_j = ctrl_j + sum_i gain[j][i] (qpos (-) qpos_ref)_i + sum_i gain[j][nv + i] (qvel - qvel_ref)_i
// with (-) in the tangent space of qpos (differentiate_pos of rsr_transition.hpp: MuJoCo's mj_differentiatePos).  What an iLQR
// forward pass, MPPI with a feedback term and CEM over controller gains ask of a rollout.  A stage of its own header, called from the
// kernel's SWEEP switch alone (tests/test_sampled_kernel_api.py).
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_transition.hpp"

namespace rsr {

// s.ctrl <- the law at rows `ref_row` of sw.fb_gain [.][NU][2 NV], sw.fb_qpos [.][NQ], sw.fb_qvel [.][NV], from the nominal ctrl
// the caller has just stored in s.ctrl (lane j wrote s.ctrl[j] and reads it back itself) and the state in s.qpos / s.qvel; row
// `out_row` of sw.ctrl_out [.][NU], when given, receives what was applied.  Called by all 64 lanes in wave-uniform code; the
// caller's fence after it publishes s.ctrl.  The sum runs in index order from the nominal ctrl, one fma per term, every lane over
// all 2 NV terms (the shuffles need every lane), so a zero gain row leaves the nominal ctrl bit for bit.
template <class C>
__device__ __forceinline__ void feedback_ctrl(const DModel& m, const Hot& hot, Smem<C>& s, const SweepArgs& sw, size_t ref_row, size_t out_row,
                                              int lane) {
  static_assert(C::NQ <= 64 && C::NV <= 64 && C::NU <= 64, "one lane per entry of the state and of ctrl");
  WSYNC();                                       // s.qpos / s.qvel were written by other lanes (the record load, or integrate)
  const gp_f p_gain = (gp_f)(sw.fb_gain + ref_row * (size_t)(C::NU * 2 * C::NV));
  const gp_f p_qref = (gp_f)(sw.fb_qpos + ref_row * (size_t)C::NQ), p_vref = (gp_f)(sw.fb_qvel + ref_row * (size_t)C::NV);
  const float yq = lane < C::NQ ? p_qref[lane] : 0.0f;
  // (the helper gives ref (-) qpos; the negation is exact.  zero_at_equal: at the reference state every term of the sum is a zero,
  // so a sample that starts on the nominal trajectory with the nominal ctrl stays on it bit for bit whatever the gain)
  const float dq = -differentiate_pos<C>(hot, s, lane, yq, true);
  const float dv = lane < C::NV ? s.qvel[lane] - p_vref[lane] : 0.0f;
  const int j = lane < C::NU ? lane : 0;
  const gp_f g = p_gain + j * (2 * C::NV);
  float u = s.ctrl[j];
#pragma unroll
  for (int i = 0; i < C::NV; ++i) u = __builtin_fmaf(g[i], __shfl(dq, i), u);
#pragma unroll
  for (int i = 0; i < C::NV; ++i) u = __builtin_fmaf(g[C::NV + i], __shfl(dv, i), u);
  if (sw.fb_clamp && m.actuator_ctrllimited[j]) u = fminf(fmaxf(u, m.actuator_ctrlrange[2 * j]), m.actuator_ctrlrange[2 * j + 1]);
  if (lane < C::NU) {
    s.ctrl[lane] = u;
    if (sw.ctrl_out) sw.ctrl_out[out_row * C::NU + lane] = u;
  }
}

}  // namespace rsr
