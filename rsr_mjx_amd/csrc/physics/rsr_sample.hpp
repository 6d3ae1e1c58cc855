// rsr_sample.hpp -- rsr_physics_sample_rollouts (include/rsr_physics.h): K control sequences of T control steps per listed env,
// each from the env's record as it stands; what a sampling planner (predictive sampling, MPPI, CEM) asks of the model.
//
// One wave per (slot, sample): the grid is count x K, transition_kernel's launch shape around rollout_kernel's loop.  Every wave
// of a slot starts from the same record row, with that env's per-env leaves and applied forces, and runs exactly the run of
// rollout_kernel on that row -- the same written-out load, load_overrides, one flattened loop of forward<C> / integrate<C> over
// the T * nsteps substeps with the warm start carried in its register, sensor_stage<C> after the last pass of a control step --
// so each sample is bit for bit the trajectory rsr_physics_rollout records on a batch whose env holds that row and those leaves
// (tests/test_sample_gpu.py).  The record is read only: K waves share a row, and the planner's batch goes on from where it
// stands.  Nothing but the caller's trajectory buffers is written: no record, no side buffer, no sensordata row.
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_sensors.hpp"
#include "rsr_applied.hpp"

namespace rsr {

// Workgroup b: slot b / K (env p.ids[slot], or slot), sample b % K.  p: nsteps, the env list and the sensor table (its buffers
// are null).  r: ctrl [M][K][T][nu] and the trajectory rows [M][K][T][w], indexed by slot: sample b's are rows b * T .. b * T + T-1.
// Ap: none, or Applied: the env's applied forces enter every pass, held for all T control steps.
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void sample_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, RollArgs r, int K, Ap... ap) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
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
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsd = p.sens.nsd;
  // one loop over the T * nsteps substeps, the control-step boundary a wave-uniform branch, as in rollout_kernel
  if (lane < C::NU) s.ctrl[lane] = r.ctrl[(size_t)b * r.T * C::NU + lane];
  WSYNC();
  const int total = r.T * p.nsteps;              // (T * nsteps < 2^31: rsr_physics_sample_rollouts)
  int t = 0, fr = 0;
  for (int k = 0; k < total; ++k) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS, stage);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    time += hot.timestep;
    if (++fr < p.nsteps) continue;
    fr = 0;
    WSYNC();
    const int lt = lrec_lane(lane);            // opaque, as in transition_kernel: the rows' addresses are formed here, not kept across
                                               // the solver (with the plain lane the Go2 joystick kernels take 44 B/lane of
                                               // scratch and the handstand ones 8, with this none does: DESIGN.md 4i)
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
      if (lt < C::NU) s.ctrl[lt] = r.ctrl[(row + 1) * C::NU + lt];
      WSYNC();
    }
  }
}

}  // namespace rsr
