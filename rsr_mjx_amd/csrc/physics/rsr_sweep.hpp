// rsr_sweep.hpp -- overlay_leaves, the stage rsr_physics_param_rollouts adds to the (slot, sample) rollout (sampled_kernel's SWEEP
// switch, rsr_sample.hpp): after load_overrides has staged the env's own leaves in LDS (its per-env values, or the model's), it
// replaces each leaf the caller sampled with row b of the caller's [M][K][width] tensor.  From there on nothing knows where a leaf
// came from, so each sample is bit for bit the trajectory rsr_physics_rollout records on a batch whose env holds that record row
// and, as its per-env leaves, that sample's (tests/test_param_rollouts_gpu.py).
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_sensors.hpp"
#include "rsr_applied.hpp"
#include "rsr_feedback.hpp"

namespace rsr {

// Row b (= slot * K + sample) of every sampled leaf over its LDS image; a null pointer leaves the image load_overrides wrote.
// The lane-to-entry mapping is load_overrides's (friction by geom slot, everything else one lane per entry), so each lane
// overwrites words it has just written itself: no fence between the two stages.  As there, every global load is issued before
// the first LDS store, so that the leaves cost one round trip, not one each; the null checks are wave-uniform (kernel arguments).
template <class C>
__device__ void overlay_leaves(const DModel& m, Smem<C>& s, const SweepArgs& sw, int b, int lane) {
  auto row = [&](int field, int width) { const float* p = sw.leaf[field]; return p ? (gp_f)(p + (size_t)b * width) : (gp_f) nullptr; };
  const gp_f p_fric = row(RSR_DR_GEOM_FRICTION, C::NG * 3), p_mass = row(RSR_DR_BODY_MASS, C::NB);
  const gp_f p_damp = row(RSR_DR_DOF_DAMPING, C::NV), p_floss = row(RSR_DR_DOF_FRICTIONLOSS, C::NV);
  constexpr int NFR = (C::NGA * 3 + 63) / 64;
  float v_fric[NFR];
#pragma unroll
  for (int k = 0; k < NFR; ++k) v_fric[k] = 0.0f;
  if (p_fric) {
#pragma unroll
    for (int k = 0; k < NFR; ++k) {                             // friction of the geom slots (geoms of the contact pairs)
      const int t = lane + 64 * k, tt = t < C::NGA * 3 ? t : 0;
      const int sidx = C::NGA == C::NG ? tt : 3 * m.geom_slot_ids[tt / 3] + tt % 3;
      v_fric[k] = p_fric[sidx];
    }
  }
  const int dl = lane < C::NV ? lane : 0;
  float v_mass = 0, v_damp = 0, v_floss = 0;
  if (p_mass) v_mass = p_mass[lane < C::NB ? lane : 0];
  if (p_damp) v_damp = p_damp[dl];
  if (p_floss) v_floss = p_floss[dl];
  float v_ipos = 0, v_q0 = 0, v_arma = 0, v_gain = 0, v_bias = 0;
  gp_f p_ipos = nullptr, p_q0 = nullptr, p_arma = nullptr, p_gain = nullptr, p_bias = nullptr;
  if constexpr (C::DREX) {
    static_assert(C::NB * 3 <= 64 && C::NQ <= 64 && C::NU * 3 <= 64, "one lane per extended leaf entry");
    p_ipos = row(RSR_DR_BODY_IPOS, C::NB * 3); p_q0 = row(RSR_DR_QPOS0, C::NQ); p_arma = row(RSR_DR_DOF_ARMATURE, C::NV);
    p_gain = row(RSR_DR_ACTUATOR_GAINPRM, C::NU * 3); p_bias = row(RSR_DR_ACTUATOR_BIASPRM, C::NU * 3);
    if (p_ipos) v_ipos = p_ipos[lane < C::NB * 3 ? lane : 0];
    if (p_q0) v_q0 = p_q0[lane < C::NQ ? lane : 0];
    if (p_arma) v_arma = p_arma[dl];
    if (p_gain) v_gain = p_gain[lane < C::NU * 3 ? lane : 0];
    if (p_bias) v_bias = p_bias[lane < C::NU * 3 ? lane : 0];
  }
  if (p_fric) {
#pragma unroll
    for (int k = 0; k < NFR; ++k) { const int t = lane + 64 * k; if (t < C::NGA * 3) s.fric[t] = v_fric[k]; }
  }
  if (p_mass && lane < C::NB) s.mass[lane] = v_mass;
  if (p_damp && lane < C::NV) s.damp[lane] = v_damp;
  if (p_floss && lane < C::NV) s.floss[lane] = v_floss;
  if constexpr (C::DREX) {
    if (p_ipos && lane < C::NB * 3) s.dx_ipos[lane] = v_ipos;
    if (p_q0 && lane < C::NQ) s.dx_qpos0[lane] = v_q0;
    if (p_arma && lane < C::NV) s.dx_arma[lane] = v_arma;
    if (p_gain && lane < C::NU * 3) s.dx_gain[lane] = v_gain;
    if (p_bias && lane < C::NU * 3) s.dx_bias[lane] = v_bias;
  }
}

}  // namespace rsr
