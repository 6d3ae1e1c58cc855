// rsr_trajectory.hpp -- rsr_physics_trajectory_fd (include/rsr_physics.h): the transition Jacobians A_t, B_t, C_t, D_t of
// rsr_physics_transition_fd at every control step of a nominal trajectory, what the backward pass of iLQR, a time-varying LQR,
// linearised MPC and an EKF smoother over a log ask of the model.
//
// Two launches on the caller's stream.  nominal_kernel, one wave per slot, runs the trajectory once: sampled_kernel's record load and
// flattened loop without the overlay and feedback stages, so it is bit for bit the K = 1 run of rsr_physics_sample_rollouts.
// Before control step t it stores qpos | qvel | qacc_warmstart to row (slot, t) of the handle's nominal scratch: what the record
// would hold after t calls of rsr_physics_step.  trajectory_fd_kernel, one wave per (slot, t, column), is then the body of
// transition_kernel (rsr_transition.hpp) with the start of a run read from that row and from ctrl[slot, t] instead of from the
// record: once the nominal states are there the M T ncol columns do not depend on each other, so the second launch is T times as
// wide as a transition_fd launch and the whole call takes about T + 2 control steps of latency where the loop of transition_fd and
// step takes 3 T.  One launch could not do this without a grid-wide wait between the two phases (the waves of step t's columns
// need the nominal state the slot's wave reaches only after t control steps); the stream orders the two for nothing.  The record is
// read only, and nothing but the scratch and the caller's buffers is written.
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_sensors.hpp"
#include "rsr_applied.hpp"
#include "rsr_transition.hpp"

namespace rsr {

// floats of a row of the nominal scratch: qpos [NQ] | qvel [NV] | qacc_warmstart [NV]
template <class C>
constexpr int nominal_row() { return C::NQ + 2 * C::NV; }

// Workgroup b: slot b (env p.ids[b], or b).  p: nsteps and the env list (its buffers and the sensor table are not used).
// tj: ctrl [M][T][nu], the scratch rows [M][T][nominal_row] and the optional nominal rows [M][T+1][nq] / [M][T+1][nv].
// Ap: none, or Applied: the env's applied forces enter every pass, held for all T control steps.
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void nominal_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, TrajArgs tj, Ap... ap) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int slot = (int)blockIdx.x, lane = threadIdx.x;
  const int e = p.ids ? p.ids[slot] : slot;
  if (e < 0 || e >= a.n) return;                                // (an id out of range runs nothing)
  const float* rec = a.state + (size_t)e * L.rec;
  const auto stage = force_stage<C>(e, ap.xfrc..., ap.qfrc...);
  PROF_DECL
  // the record load of rollout_kernel, written out
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float warm = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  load_overrides<C>(m, s, a, e, lane);
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  float Mrow[C::NV];
  FwdOut<C> f;
  // the state before control step t (t < T: the scratch row) and row t of the nominal trajectory (t <= T)
  auto keep = [&](int t, int ln, float w) {
    if (t < tj.T) {
      float* o = tj.nominal + ((size_t)slot * tj.T + t) * nominal_row<C>();
      for (int q = ln; q < C::NQ; q += 64) o[q] = s.qpos[q];
      if (ln < C::NV) { o[C::NQ + ln] = s.qvel[ln]; o[C::NQ + C::NV + ln] = w; }
    }
    const size_t row = (size_t)slot * (tj.T + 1) + t;
    if (tj.qpos) for (int q = ln; q < C::NQ; q += 64) tj.qpos[row * C::NQ + q] = s.qpos[q];
    if (tj.qvel && ln < C::NV) tj.qvel[row * C::NV + ln] = s.qvel[ln];
  };
  // one loop over the T * nsteps substeps, the control-step boundary a wave-uniform branch, as in rollout_kernel
  if (lane < C::NU) s.ctrl[lane] = tj.ctrl[(size_t)slot * tj.T * C::NU + lane];
  WSYNC();
  keep(0, lane, warm);
  const int total = tj.T * p.nsteps;             // (T * nsteps < 2^31: rsr_physics_trajectory_fd)
  int t = 0, fr = 0;
  for (int k = 0; k < total; ++k) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS, stage);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    if (++fr < p.nsteps) continue;
    fr = 0;
    WSYNC();
    const int lt = lrec_lane(lane);            // opaque, as in sampled_kernel: the rows' addresses are formed here, not kept across
                                               // the solver
    keep(++t, lt, warm);
    if (t < tj.T) {
      if (lt < C::NU) s.ctrl[lt] = tj.ctrl[((size_t)slot * tj.T + t) * C::NU + lt];
      WSYNC();
    }
  }
}

// Workgroup b: slot b / (T ncol) (env p.ids[slot], or slot), control step (b / ncol) % T, column b % ncol.  p: nsteps, the env
// list and the sensor table (its buffers are not written).  tj: the scratch rows nominal_kernel left, ctrl [M][T][nu], and the
// columns [M][T][ncol][2 nv + nsd]: workgroup b writes row b, every entry of it.  The body is transition_kernel's, statement for
// statement but for where a run starts from and where the column goes; the launch adds the same LDS (fd_lds_bytes).
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void trajectory_fd_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, TrajArgs tj, Ap... ap) {
  static_assert(C::NQ <= 64 && C::NV <= 64 && C::NU <= 64 && RSR_MAX_SENSORDATA <= 64, "one lane per entry of the kept end state");
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  float* park = reinterpret_cast<float*>(smem_raw + fd_park_offset<C>());
  constexpr int NCOL = 2 * C::NV + C::NU;
  const int b = (int)blockIdx.x, cell = b / NCOL, col = b - cell * NCOL, slot = cell / tj.T, lane = threadIdx.x;      // cell = slot * T + t
  const int e = p.ids ? p.ids[slot] : slot;
  if (e < 0 || e >= a.n) return;                                // (an id out of range runs nothing)
  const auto stage = force_stage<C>(e, ap.xfrc..., ap.qfrc...);
  PROF_DECL
  const int nsd = p.sens.nsd;
  // a run's start: the record load of physics_kernel with the scratch row (slot, t) for the record and ctrl[slot, t] for its ctrl,
  // then the perturbation
  float warm = 0.0f;
  auto begin_run = [&](float dlt) {
    const int ln = lrec_lane(lane);             // opaque, so that no address of the first run's load stays live across the solver for the second
    const float* nom = tj.nominal + (size_t)cell * nominal_row<C>();
    for (int t = ln; t < C::NQ; t += 64) s.qpos[t] = nom[t];
    if (ln < C::NV) { s.qvel[ln] = nom[C::NQ + ln]; warm = nom[C::NQ + C::NV + ln]; }
    load_overrides<C>(m, s, a, e, ln);
    if (ln < C::NU) s.ctrl[ln] = tj.ctrl[(size_t)cell * C::NU + ln];
    if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
      if (ln == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
    }
    WSYNC();
    // dlt through the opaque zero of ln, as in transition_kernel
    const float dl = asf(__builtin_bit_cast(int, dlt) + (ln - lane));
    if (dlt != 0.0f) perturb_state<C>(hot, s, ln, col, dl);      // (wave-uniform; not centred: the second run is the nominal state itself)
    WSYNC();
  };
  float Mrow[C::NV];
  FwdOut<C> f;
  begin_run(tj.eps);
  // the two runs as one loop over their 2 * nsteps substeps, the end of a run a wave-uniform branch, as in transition_kernel
  const int total = 2 * p.nsteps;              // (nsteps < 2^30: rsr_physics_trajectory_fd)
  int run = 0, fr = 0;
  for (int k = 0; k < total; ++k) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS, stage);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    if (++fr < p.nsteps) continue;
    fr = 0;
    WSYNC();
    const int lt = lrec_lane(lane);            // opaque: the addresses of the run's end are formed here, not kept across the solver
    float sv = 0.0f;
    if (nsd > 0) sv = sensor_stage<C>(m, s, lt, f.qacc, p.sens);      // (wave-uniform; no table: the stage is skipped)
    const bool centered = (tj.flags & RSR_FD_CENTERED) != 0;
    if (run == 0) {
      if (lt < C::NQ) park[lt] = s.qpos[lt];
      if (lt < C::NV) park[C::NQ + lt] = s.qvel[lt];
      park[C::NQ + C::NV + lt] = sv;
      WSYNC();                                   // the next run's load overwrites what was just read
      run = 1;
      begin_run(centered ? -tj.eps : 0.0f);
    } else {
      // the column: one contiguous row of the caller's buffer, tight (2 nv + nsd entries)
      const float hstep = centered ? 2.0f * tj.eps : tj.eps;
      const float yq = lt < C::NQ ? park[lt] : 0.0f, yv = lt < C::NV ? park[C::NQ + lt] : 0.0f, ys = park[C::NQ + C::NV + lt];
      const float dq = differentiate_pos<C>(hot, s, lt, yq);
      float* o = tj.columns + (size_t)b * (2 * C::NV + nsd);
      if (lt < C::NV) { o[lt] = dq / hstep; o[C::NV + lt] = (yv - s.qvel[lt]) / hstep; }
      if (lt < nsd) o[2 * C::NV + lt] = (ys - sv) / hstep;
    }
  }
}

}  // namespace rsr
