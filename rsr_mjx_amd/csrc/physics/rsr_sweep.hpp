// rsr_sweep.hpp -- rsr_physics_param_rollouts (include/rsr_physics.h): K sets of model leaves per listed env, each run for T
// control steps from the env's record as it stands; what system identification, domain-randomised planning and CEM over
// friction, damping or gains ask of the model.
//
// One wave per (slot, sample): sample_kernel's launch shape and loop (rsr_sample.hpp), restated statement for statement as that
// kernel restates rollout_kernel, with one stage more.  After load_overrides has staged the env's own leaves in LDS (its per-env
// values, or the model's), overlay_leaves replaces each leaf the caller sampled with row b of the caller's [M][K][width] tensor.
// From there on nothing knows where a leaf came from, so each sample is bit for bit the trajectory rsr_physics_rollout records on
// a batch whose env holds that record row and, as its per-env leaves, that sample's (tests/test_param_rollouts_gpu.py).  ctrl is
// per sample, or one sequence shared by a slot's K samples (the identification case: one logged control sequence).  The record is
// read only, and nothing but the caller's trajectory buffers is written: no record, no side buffer, no sensordata row.
//
// rsr_physics_feedback_rollouts is the same launch with sw.fb_gain set: feedback_ctrl (rsr_feedback.hpp) then turns the ctrl row
// just loaded into ctrl + gain (x (-) x_ref) on the sample's own state, at the start and at every control-step boundary.  The
// branch is wave-uniform (a kernel argument), and with it off the kernel runs the statements it ran before.
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

// Workgroup b: slot b / K (env p.ids[slot], or slot), sample b % K, K = sw.K.  p: nsteps, the env list and the sensor table (its
// buffers are null).  r: ctrl [M][K][T][nu] (sw.ctrl_per_sample) or [M][T][nu], and the trajectory rows [M][K][T][w], indexed by
// slot: sample b's are rows b * T .. b * T + T-1.  sw: the sampled leaves [M][K][width], row b sample b's.
// Ap: none, or Applied: the env's applied forces enter every pass, held for all T control steps.
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void sweep_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, RollArgs r, SweepArgs sw, Ap... ap) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
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
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsd = p.sens.nsd;
  // the slot's ctrl rows, or the sample's (uniform over the launch)
  const size_t cb = sw.ctrl_per_sample ? (size_t)b : (size_t)slot;
  // one loop over the T * nsteps substeps, the control-step boundary a wave-uniform branch, as in rollout_kernel
  if (lane < C::NU) s.ctrl[lane] = r.ctrl[cb * r.T * C::NU + lane];
  if (sw.fb_gain) feedback_ctrl<C>(m, hot, s, sw, (sw.fb_per_sample ? (size_t)b : (size_t)slot) * r.T, (size_t)b * r.T, lane);
  WSYNC();
  const int total = r.T * p.nsteps;              // (T * nsteps < 2^31: rsr_physics_param_rollouts)
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
    if (++t < r.T) {
      if (lt < C::NU) s.ctrl[lt] = r.ctrl[(cb * r.T + t) * C::NU + lt];
      if (sw.fb_gain) feedback_ctrl<C>(m, hot, s, sw, (sw.fb_per_sample ? (size_t)b : (size_t)slot) * r.T + t, (size_t)b * r.T + t, lt);
      WSYNC();
    }
  }
}

}  // namespace rsr
