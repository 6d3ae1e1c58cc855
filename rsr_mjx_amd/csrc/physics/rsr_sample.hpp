// rsr_sample.hpp -- the (slot, sample) rollouts (include/rsr_physics.h): K runs of T control steps per listed env, each from the
// env's record as it stands.  One kernel body, sampled_kernel, instantiated per op; an op's switch adds its stages at compile
// time, so each op runs its own instructions and none of another's:
//   SampleOp   rsr_physics_sample_rollouts: K control sequences per env; what a sampling planner (predictive sampling, MPPI, CEM)
//              asks of the model.  Neither switch is on: the loop alone.
//   SweepOp    rsr_physics_param_rollouts: K sets of model leaves per env; what system identification, domain-randomised planning
//              and CEM over friction, damping or gains ask.  SWEEP adds overlay_leaves (rsr_sweep.hpp) after load_overrides: each
//              leaf the caller sampled replaces its LDS image with row b of the caller's [M][K][width] tensor, and from there on
//              nothing knows where a leaf came from.  ctrl is per sample, or one sequence shared by a slot's K samples (the
//              identification case: one logged control sequence).  rsr_physics_feedback_rollouts is the same launch with
//              sw.fb_gain set: feedback_ctrl (rsr_feedback.hpp) then turns the ctrl row just loaded into ctrl + gain (x (-) x_ref)
//              on the sample's own state, at the start and at every control-step boundary.  The branch is wave-uniform (a kernel
//              argument), and with it off the kernel runs the statements it ran before.
//   CostOp     rsr_physics_cost_rollouts: SweepOp's run and the running cost of every sample, formed where its state is.  COST
//              (with SWEEP) adds the five accumulators behind Smem<C> and cost_stage (rsr_cost.hpp) at the end of control step t,
//              after sensor_stage and the rows of the trajectory and before the next ctrl row overwrites s.ctrl.
//
// One wave per (slot, sample): the grid is count x K, transition_kernel's launch shape around rollout_kernel's loop.  Every wave
// of a slot starts from the same record row, with that env's per-env leaves and applied forces, and runs exactly the run of
// rollout_kernel on that row -- the same written-out load, load_overrides, one flattened loop of forward<C> / integrate<C> over
// the T * nsteps substeps with the warm start carried in its register, sensor_stage<C> after the last pass of a control step --
// so each sample is bit for bit the trajectory rsr_physics_rollout records on a batch whose env holds that row and, as its
// per-env leaves, that sample's (tests/test_sample_gpu.py, tests/test_param_rollouts_gpu.py).  The record is read only: K waves
// share a row, and the planner's batch goes on from where it stands.  Nothing but the caller's buffers is written: no record, no
// side buffer, no sensordata row.
#pragma once
#include <type_traits>
#include "../rsr_launch.hpp"
#include "rsr_sensors.hpp"
#include "rsr_applied.hpp"
#include "rsr_sweep.hpp"
#include "rsr_cost.hpp"

namespace rsr {

// The three ops and what each takes behind RollArgs; the kernel-argument bytes are those of the arguments written out one by one.
struct SampleOp { using Args = int; };                                  // K
struct SweepOp  { using Args = SweepArgs; };
struct CostOp   { struct Args { SweepArgs sw; CostArgs c; }; };
// the sweep's arguments in an op's (SampleOp has none: its K, which no SWEEP statement reads)
__device__ __forceinline__ const int& sweep_args(const int& K) { return K; }
__device__ __forceinline__ const SweepArgs& sweep_args(const SweepArgs& x) { return x; }
__device__ __forceinline__ const SweepArgs& sweep_args(const CostOp::Args& x) { return x.sw; }

// Workgroup b: slot b / K (env p.ids[slot], or slot), sample b % K.  p: nsteps, the env list and the sensor table (its buffers
// are null).  r: ctrl [M][K][T][nu] (SampleOp, or sw.ctrl_per_sample) or [M][T][nu], and the trajectory rows [M][K][T][w], indexed
// by slot: sample b's are rows b * T .. b * T + T-1; CostOp: every pointer of r may be null.  x: K, or sw: K and the sampled leaves
// [M][K][width], row b sample b's (CostOp: sw.ctrl_out is null), or sw and c: the references and weights [M][T][w] by slot and the
// outputs by (slot, sample).  Ap: none, or Applied: the env's applied forces enter every pass, held for all T control steps.
template <class C, int WAVES, class Op, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void sampled_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, RollArgs r, typename Op::Args x, Ap... ap) {
  constexpr bool SWEEP = !std::is_same<Op, SampleOp>::value, COST = std::is_same<Op, CostOp>::value;
  if constexpr (COST) static_assert(4 * WAVES * cost_lds_bytes<C>() <= 160 * 1024, "4 x WAVES workgroups share a CU's LDS");
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const auto& sw = sweep_args(x);
  int K;
  if constexpr (SWEEP) K = sw.K; else K = x;
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
  if constexpr (SWEEP) overlay_leaves<C>(m, s, sw, b, lane);      // the sample's leaves over the env's own (same lanes, same words: no fence between)
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  if constexpr (COST) {                          // the accumulators from +0 (published to lane 0 by the fence below)
    float* acc = reinterpret_cast<float*>(smem_raw + cost_acc_offset<C>());
    if (lane < 8) acc[lane] = 0.0f;
  }
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsd = p.sens.nsd;
  size_t cb = 0;                                 // SWEEP: the slot's ctrl rows, or the sample's (uniform over the launch)
  if constexpr (SWEEP) cb = sw.ctrl_per_sample ? (size_t)b : (size_t)slot;
  // one loop over the T * nsteps substeps, the control-step boundary a wave-uniform branch, as in rollout_kernel
  if constexpr (SWEEP) {
    if (lane < C::NU) s.ctrl[lane] = r.ctrl[cb * r.T * C::NU + lane];
    if (sw.fb_gain) feedback_ctrl<C>(m, hot, s, sw, (sw.fb_per_sample ? (size_t)b : (size_t)slot) * r.T, (size_t)b * r.T, lane);
  } else {
    if (lane < C::NU) s.ctrl[lane] = r.ctrl[(size_t)b * r.T * C::NU + lane];
  }
  WSYNC();
  const int total = r.T * p.nsteps;              // (T * nsteps < 2^31: every entry refuses more)
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
                                               // scratch and the handstand ones 8, with this none does: DESIGN.md 4i, 4j)
    const size_t row = (size_t)b * r.T + t;
    float sv = 0.0f;
    if (nsd > 0) sv = sensor_stage<C>(m, s, lt, f.qacc, p.sens);      // (wave-uniform; no table: the stage is skipped)
    if (r.qpos) for (int q = lt; q < C::NQ; q += 64) r.qpos[row * C::NQ + q] = s.qpos[q];
    if (r.qvel && lt < C::NV) r.qvel[row * C::NV + lt] = s.qvel[lt];
    if (r.time && lt == 0) r.time[row] = time;
    if (r.aforce && lt < C::NU) r.aforce[row * C::NU + lt] = s.aforce[lt];
    if (r.ncon && lt == 0) r.ncon[row] = (float)s.ncon;
    if (r.sd && lt < nsd) r.sd[row * nsd + lt] = sv;
    if constexpr (COST) {                        // s.ctrl still holds the control of this step: the next row is loaded below
      float* acc = reinterpret_cast<float*>(smem_raw + cost_acc_offset<C>());
      cost_stage<C>(hot, s, acc, x.c, (size_t)slot * r.T + t, row, (size_t)b, t == r.T - 1, lt, sv, nsd);
    }
    if (++t < r.T) {
      if constexpr (SWEEP) {
        if (lt < C::NU) s.ctrl[lt] = r.ctrl[(cb * r.T + t) * C::NU + lt];
        if (sw.fb_gain) feedback_ctrl<C>(m, hot, s, sw, (sw.fb_per_sample ? (size_t)b : (size_t)slot) * r.T + t, (size_t)b * r.T + t, lt);
      } else {
        if (lt < C::NU) s.ctrl[lt] = r.ctrl[(row + 1) * C::NU + lt];
      }
      WSYNC();
    }
  }
}

}  // namespace rsr
