// rsr_airbot.hpp -- the Airbot env kernels (cube / sf and T-shape): reset_kernel and the work-queue step_kernel.
#pragma once
#include "rsr_env.hpp"

namespace rsr {

// cube_env.py:215-229
template <class C>
__device__ void cube_obs(const DModel& m, const Smem<C>& s, const float* target_pos, const float* ncp, float* obs) {
  const int cube = m.env_ids[ID_CUBE], site = m.env_ids[ID_SITE];
  for (int i = 0; i < 6; ++i) obs[i] = s.qpos[m.env_ids[ID_JOINTQ + i]];
  for (int i = 0; i < 3; ++i) {
    float sp = s.spos[3 * site + i], cp = s.xpos[3 * cube + i], tp = target_pos[i];
    obs[6 + i] = sp; obs[9 + i] = tp; obs[12 + i] = cp; obs[17 + i] = tp - cp; obs[20 + i] = cp - sp;
  }
  obs[15] = ncp[0]; obs[16] = ncp[1];
}

// T-shape env_ids layout (rsr_mjx_amd/envs/config.py: tshape_env_fields); egeom[0..3] = base_block, vertical_block,
// base_target, vertical_target
enum { TID_T = 0, TID_TARGET = 1, TID_SITE = 2, TID_TAIL = 3, TID_TTAIL = 4, TID_GBASE = 5, TID_JOINTQ = 9 };

// T_shape_env.py:223-234
template <class C>
__device__ void tshape_obs(const DModel& m, const Smem<C>& s, const float* tb, const float* tv, float xita, const float* newT,
                           float* obs) {
  const int site = m.env_ids[TID_SITE];
  for (int i = 0; i < 6; ++i) obs[i] = s.qpos[m.env_ids[TID_JOINTQ + i]];
  obs[6] = s.spos[3 * site + 2];
  for (int i = 0; i < 3; ++i) { obs[7 + i] = tb[i] - s.egeom[i]; obs[10 + i] = tv[i] - s.egeom[3 + i]; }
  obs[13] = xita;
  obs[14] = newT[0] - s.spos[3 * site]; obs[15] = newT[1] - s.spos[3 * site + 1];
}

// ---------------------------------------------------------------- reset kernel
// cube / sf: cube_env.py:95-143 ; T-shape: T_shape_env.py:98-137 ; + Episode/AutoReset wrapper resets
template <class C, int ENV>
__global__ __launch_bounds__(64) void reset_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  float* rec = a.state + (size_t)e * L.rec;
  const float* R = m.env_reset;
  constexpr int JQ = ENV == ENV_TSHAPE ? (int)TID_JOINTQ : (int)ID_JOINTQ;     // arm joint qpos addresses in env_ids
  constexpr int RCTRL = ENV == ENV_TSHAPE ? 7 : 8;                            // ctrl init in env_reset
  uint32_t* bits = reinterpret_cast<uint32_t*>(s.scratch_b());         // PRNG scratch
  load_overrides<C>(m, s, a, e, lane);
  const uint32_t k0 = a.keys[2 * e], k1 = a.keys[2 * e + 1];
  random_bits(k0, k1, 10, bits, lane);                        // rng, rng1..rng4 = split(rng, 5)
  WSYNC();
  uint32_t kk[5][2];
#pragma unroll
  for (int r = 0; r < 5; ++r) { kk[r][0] = bits[2 * r]; kk[r][1] = bits[2 * r + 1]; }
  WSYNC();
  const float lo = -R[0], hi = R[0];
  random_bits(kk[1][0], kk[1][1], C::NQ, bits, lane);
  WSYNC();
  if (lane < C::NQ) s.qpos[lane] = m.qpos0[lane] + uniform_from_bits(bits[lane], lo, hi);
  WSYNC();
  if (lane < 6) s.qpos[m.env_ids[JQ + lane]] += R[1 + lane];
  if (ENV != ENV_TSHAPE && lane == 6) s.qpos[m.env_ids[ID_FINGERQ]] = R[7];
  random_bits(kk[2][0], kk[2][1], C::NV, bits, lane);
  WSYNC();
  if (lane < C::NV) s.qvel[lane] = uniform_from_bits(bits[lane], lo, hi);
  WSYNC();
  random_bits(kk[3][0], kk[3][1], C::NU, bits, lane);
  WSYNC();
  float ctrl_init = lane < C::NU ? R[RCTRL + lane] + uniform_from_bits(bits[lane], lo, hi) : 0.0f;
  WSYNC();
  if constexpr (ENV != ENV_TSHAPE) {
    random_bits(kk[4][0], kk[4][1], 3, bits, lane);
    WSYNC();
    if (lane < 3) s.qpos[m.env_ids[ID_SITEQ] + lane] = uniform_from_bits(bits[lane], R[13 + lane], R[16 + lane]);
    WSYNC();
    random_bits(kk[0][0], kk[0][1], 3, bits, lane);
    WSYNC();
    if (lane < 3) s.qpos[m.env_ids[ID_BOXQ] + lane] = uniform_from_bits(bits[lane], R[19 + lane], R[22 + lane]);
  }
  if (lane < C::NU) s.ctrl[lane] = 0.0f;                      // pipeline_init runs forward with ctrl = 0
  WSYNC();
  float Mrow[C::NV], warm = 0.0f;
  FwdOut<C> f;
  PROF_DECL
  forward<C>(m, hot, s, lane, Mrow, warm, f, a.debug ? a.debug + (size_t)e * RSR_DEBUG_FLOATS : nullptr PROF_PASS);
  WSYNC();
  if (lane < C::NU) s.ctrl[lane] = ctrl_init;                 // data.replace(ctrl=joint_ctrl), no re-forward
  WSYNC();
  store_pipeline<C>(s, rec, L, lane, warm, 0.0f);
  if (lane == 0) {
    float obs[C::OBS];
    if constexpr (ENV == ENV_TSHAPE) {
      const int site = m.env_ids[TID_SITE], tb = m.env_ids[TID_T];
      float newT[2] = {R[12], R[13]};
      for (int i = 0; i < 3; ++i) {
        rec[L.target_base_pos + i] = s.egeom[6 + i]; rec[L.target_vertical_pos + i] = s.egeom[9 + i];
        rec[L.site_pos + i] = s.spos[3 * site + i]; rec[L.T_pos + i] = s.xpos[3 * tb + i];
      }
      rec[L.target_w] = s.xquat[4 * m.env_ids[TID_TARGET]] * 10.0f;
      rec[L.new_T_pos] = newT[0]; rec[L.new_T_pos + 1] = newT[1];
      rec[L.xita] = R[14];
      tshape_obs<C>(m, s, &s.egeom[6], &s.egeom[9], R[14], newT, obs);
    } else {
      const int cube = m.env_ids[ID_CUBE], tgt = m.env_ids[ID_TARGET], site = m.env_ids[ID_SITE];
      float tp[3], ncp[2] = {R[25], R[26]};
      for (int i = 0; i < 3; ++i) {
        tp[i] = s.xpos[3 * tgt + i];
        rec[L.target_pos + i] = tp[i];
        rec[L.site_pos + i] = s.spos[3 * site + i];
        rec[L.cube_pos + i] = s.xpos[3 * cube + i];
      }
      rec[L.new_cube_pos] = ncp[0]; rec[L.new_cube_pos + 1] = ncp[1];
      rec[L.last_action] = 0.0f;
      cube_obs<C>(m, s, tp, ncp, obs);
    }
    for (int i = 0; i < C::OBS; ++i) { rec[L.obs + i] = obs[i]; rec[L.f_obs + i] = obs[i]; }
    store_reset_outputs<C>(s, f, rec, L);
  }
  store_first_state<C>(s, rec, L, lane, warm, true);      // AutoResetWrapper.reset: cache first_pipeline_state
}

// ---------------------------------------------------------------- step kernel
// cube / sf: cube_env.py:145-213, test/airbot.py:165-252 ; T-shape: T_shape_env.py:139-221 ; + wrappers.
// LDS is dynamic so that the register budget is set by RSR_WAVES_PER_EU below, not by the compiler's
// LDS-derived occupancy guess (which lands one register over the 2-waves/SIMD budget and halves residency).
template <class C, int ENV>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RSR_WAVES_PER_EU, RSR_WAVES_PER_EU)))
void step_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, Sched sc) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int lane = threadIdx.x;
  const bool wrap_episode = m.wrap_flags & 1, wrap_autoreset = (m.wrap_flags & 2) != 0;
  constexpr int JQ = ENV == ENV_TSHAPE ? (int)TID_JOINTQ : (int)ID_JOINTQ;
  // Ticket space: the first n_whole envs are stepped as ONE unit each (all substeps: no hand-off, no flag, one ticket), the rest
  // as `units` phases each, phase-major.  Long units first, short units last: the launch still drains in short units, and only the
  // envs that start late pay the per-unit overhead (ticket round trip, flag poll, state round trip through memory, store drain).
  const int units = sc.units, n_whole = sc.n_whole, n_split = a.n - n_whole, total = n_whole + units * n_split;
  int* const ticket = sc.ticket + (sc.launch_id & 1u);
  // A wave's first ticket is its workgroup index where that ticket is a whole-env unit (which nobody waits for) -- 2048 waves
  // drawing from one counter at launch serialise at ~90 atomics per microsecond, ~20 us before the last wave has its first
  // unit -- and the counter hands out the tickets from n_static on.  (Tickets of split envs are only ever drawn from the counter,
  // in dependency order, so the wave that holds (env, phase - 1) is running whatever the residency of the grid.)
  const int n_static = (int)gridDim.x < n_whole ? (int)gridDim.x : n_whole;
  if (blockIdx.x == 0 && lane == 0) __hip_atomic_store(sc.ticket + ((sc.launch_id + 1u) & 1u), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch's counter
  auto draw = [&]() {
    int t = 0;
    if (lane == 0) t = n_static + __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return t;
  };
  int tk_next = (int)blockIdx.x < n_static ? (int)blockIdx.x : draw();
  for (;;) {                                                   // persistent wave: one work unit per trip
  // The next unit's ticket is drawn when the current unit's substeps are done, ahead of its stores / epilogue: the atomic's round
  // trip (~2 us under load, 16 units per wave and launch) overlaps them.  (Drawn at the START of the current unit it binds the
  // last units of a launch to waves that are still busy for a whole unit while others idle: measured -3.4 % on the cube.)
  const int tk = uniform_i(tk_next);
  if (tk >= total) break;                                      // every wave reaches this: the queue only drains
  int phase = 0, e = tk, eu = 1;                               // eu = units of this env's class
  if (tk >= n_whole) { const int t2 = tk - n_whole; phase = t2 / n_split; e = n_whole + (t2 - phase * n_split); eu = units; }
  const bool first = phase == 0, last = phase == eu - 1;
  float* rec = a.state + (size_t)e * L.rec;
  PROF_DECL
  // ---- load the record ----
  // what no other unit of this launch writes first: the per-env model leaves and the env's bookkeeping words, so that their round
  // trip overlaps the flag poll below
  load_overrides<C>(m, s, a, e, lane);
  const float done_prev = rec[L.done];
  float steps = rec[L.steps];
  if (wrap_autoreset && done_prev != 0.0f) steps = 0.0f;     // AutoResetWrapper.step pre-step
  // env info read before it is updated
  float tp[3] = {0, 0, 0}, aux_old[2];
  if constexpr (ENV == ENV_TSHAPE) { aux_old[0] = rec[L.new_T_pos]; aux_old[1] = rec[L.new_T_pos + 1]; }
  else {
    tp[0] = rec[L.target_pos]; tp[1] = rec[L.target_pos + 1]; tp[2] = rec[L.target_pos + 2];
    aux_old[0] = rec[L.new_cube_pos]; aux_old[1] = rec[L.new_cube_pos + 1];
  }
  float warm = 0.0f, time;
  unsigned handoff_err = 0u;
  if (first) {
    for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
    if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
    time = rec[L.time];
  } else {
    // the previous phase of this env (another wave, any CU) has published its state: poll its flag, then read every handed-off
    // word past the caches.  The spin is bounded; a timeout is sticky: counted in sc.err, carried to the env's later phases in
    // the flag's error bit, and reported by the last phase as stats[3] = -1 (the unit runs on whatever the record holds).
    const unsigned want = (sc.launch_id << 8) | (unsigned)phase;
    int spins = 0;
    unsigned fl;
    while (((fl = __hip_atomic_load(sc.flags + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & ~RSR_FLAG_ERR) != want && spins < sc.spin_cap) { __builtin_amdgcn_s_sleep(8); ++spins; }
    fl = (unsigned)uniform_i((int)fl);
    const bool timed_out = (fl & ~RSR_FLAG_ERR) != want;
    handoff_err = timed_out ? RSR_FLAG_ERR : (fl & RSR_FLAG_ERR);
    if (timed_out && lane == 0) {
      __hip_atomic_fetch_add(sc.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(sc.err + 1, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = ld_sc1(&rec[L.qpos + t]);
    if (lane < C::NV) { s.qvel[lane] = ld_sc1(&rec[L.qvel + lane]); warm = ld_sc1(&rec[L.warm + lane]); }
    if (lane < C::NU) s.ctrl[lane] = ld_sc1(&rec[L.ctrl + lane]);
    time = ld_sc1(&rec[L.time]);
  }
  // ---- prologue: ctrl shaping; uses the stale xpos / site_xpos of the previous forward pass ----
  if (first && lane < C::NU) {
#pragma clang fp contract(off)   // env algebra is evaluated op by op, as the reference's JAX-CPU path does
    float delta = m.env_action_scale[lane] * a.action[(size_t)e * C::NU + lane];
    float act = rec[L.ctrl + lane] + delta;
    if (lane == 3) act = -((1.57f + rec[L.qpos + m.env_ids[JQ + 1]]) + rec[L.qpos + m.env_ids[JQ + 2]]);
    float delta0 = m.env_action_scale[0] * a.action[(size_t)e * C::NU];
    float act0 = rec[L.ctrl] + delta0;
    if (lane == 4) {
      if constexpr (ENV == ENV_TSHAPE) {      // T_shape_env.py:146-153: aim from the end effector at the T's tail
        const int site = m.env_ids[TID_SITE], tail = m.env_ids[TID_TAIL];
        float dx = rec[L.site_xpos + 3 * tail] - rec[L.site_xpos + 3 * site];
        float dy = rec[L.site_xpos + 3 * tail + 1] - rec[L.site_xpos + 3 * site + 1];
        float ang = atan2f(dy, dx + 0.00001f);
        act = (-ang + act0) + 1.5708f;
      } else {                                // cube_env.py:152-159
        const int cube = m.env_ids[ID_CUBE];
        float dx = tp[0] - rec[L.xpos + 3 * cube], dy = tp[1] - rec[L.xpos + 3 * cube + 1];
        float ang = atan2f(dy, dx + 0.00001f);
        act = (-ang + act0) + 1.5708f;
        if (m.env_kind == ENV_AIRBOT_SF) {    // test/airbot.py:180-184: hold the wrist target within 3 cm of the goal
          float dz = tp[2] - rec[L.xpos + 3 * cube + 2];
          if (sqrtf(dx * dx + dy * dy + dz * dz) < 0.03f) act = rec[L.last_action];
          rec[L.last_action] = act;
        }
      }
    }
    s.ctrl[lane] = clampf(act, m.env_ctrl_lo[lane], m.env_ctrl_hi[lane]);
  }
  WSYNC();
  PROF(PS_LOAD)
  // ---- n_frames x mjx.step ----
  float Mrow[C::NV];
  FwdOut<C> f;
  for (int fr = phase * hot.n_frames / eu; fr < (phase + 1) * hot.n_frames / eu; ++fr) {
#if defined(RSR_PROFILE) || defined(RSR_TIMELINE)
    float* dbg = nullptr;
#else
    float* dbg = (a.debug && fr == m.n_frames - 1) ? a.debug + (size_t)e * RSR_DEBUG_FLOATS : nullptr;
#endif
    // the lane index passes through an opaque zero per substep: values derived from it (masks, LDS addresses) are then
    // recomputed in each substep instead of being hoisted out of the loop, kept live across the solver and spilled
    const int lane_s = lrec_lane(lane);
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, dbg PROF_PASS);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    time += hot.timestep;
  }
  tk_next = draw();
  if (!last) {
    // hand the pipeline state to the next phase: write-through stores, drained, then the flag (one wave = one workgroup)
    for (int t = lane; t < C::NQ; t += 64) st_sc1(&rec[L.qpos + t], s.qpos[t]);
    if (lane < C::NV) { st_sc1(&rec[L.qvel + lane], s.qvel[lane]); st_sc1(&rec[L.warm + lane], warm); }
    if (lane < C::NU) st_sc1(&rec[L.ctrl + lane], s.ctrl[lane]);
    if (lane == 0) st_sc1(&rec[L.time], time);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0 && !(first && e == sc.withhold_env))
      __hip_atomic_store(sc.flags + e, (sc.launch_id << 8) | (unsigned)(phase + 1) | handoff_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#if defined(RSR_PROFILE) || defined(RSR_TIMELINE)
    if (a.debug && lane == 0) prof_timeline(a.debug + (size_t)e * RSR_DEBUG_FLOATS + 7300 + 8 * phase, prof_rt0_, prof_ct0_);
#endif
    WSYNC();
    continue;
  }
  // ---- epilogue: reward, done, obs, info; derived data are from the last forward pass ----
  float done = 0.0f;
  float* obs_lds = s.scratch_b();                                     // staged so that auto-reset can override it
  if (lane == 0) {
#pragma clang fp contract(off)
    const float* W = m.env_reward;
    float reward, met[C::NMET];
    // the record words the wrapper code below reads back, fetched here in one batch: left at their uses they follow the metric
    // stores (same base pointer, run-time offsets: the compiler must keep the order) and each waits out a memory round trip
    float prev_done = 0.0f, em_old[2 + C::NMET];
#pragma unroll
    for (int i = 0; i < 2 + C::NMET; ++i) em_old[i] = 0.0f;
    if (wrap_episode) {
      prev_done = rec[L.episode_done];
#pragma unroll
      for (int i = 0; i < 2 + C::NMET; ++i) em_old[i] = rec[L.episode_metrics + i];
    }
    const float met_kept = rec[L.metrics + (ENV == ENV_TSHAPE ? 3 : 1)];      // the metric this env never writes
    if constexpr (ENV == ENV_TSHAPE) {
      const int site = m.env_ids[TID_SITE], tail = m.env_ids[TID_TAIL], ttail = m.env_ids[TID_TTAIL], tbody = m.env_ids[TID_T];
      float sp[3] = {s.spos[3 * site], s.spos[3 * site + 1], s.spos[3 * site + 2]};
      const float* gb = &s.egeom[0]; const float* gv = &s.egeom[3];
      float tb[3], tv[3];
      for (int i = 0; i < 3; ++i) { tb[i] = rec[L.target_base_pos + i]; tv[i] = rec[L.target_vertical_pos + i]; }
      float a0 = tb[0] - gb[0], a1 = tb[1] - gb[1], a2 = tb[2] - gb[2];
      float dis_base = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
      if (dis_base < 0.005f) dis_base = 0.0f;
      float push_base = 1.0f / (1.0f + 10.0f * dis_base);
      float b0 = tv[0] - gv[0], b1 = tv[1] - gv[1], b2 = tv[2] - gv[2];
      float dis_vert = sqrtf(b0 * b0 + b1 * b1 + b2 * b2);
      if (dis_vert < 0.005f) dis_vert = 0.0f;
      float push_vert = 1.0f / (1.0f + 10.0f * dis_vert);
      float ba[3] = {gv[0] - gb[0], gv[1] - gb[1], gv[2] - gb[2]}, ta[3] = {tv[0] - tb[0], tv[1] - tb[1], tv[2] - tb[2]};
      float dotp = ba[0] * ta[0] + ba[1] * ta[1] + ba[2] * ta[2];
      float nb = sqrtf(ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2]), nt = sqrtf(ta[0] * ta[0] + ta[1] * ta[1] + ta[2] * ta[2]);
      float xita = acosf(clampf(dotp / (nb * nt), -1.0f, 1.0f));
      float push_w = 1.0f / (1.0f + 6.0f * xita);
      float push = (0.1515f * push_base + 0.1515f * push_vert + 0.66f * push_w) * W[0];
      float site_z = sp[2] < 0.83f ? 1.0f : 0.0f;
      float z_reward = 4.0f / (1.0f + 3.0f * fabsf(sp[2] - 0.805f));
      site_z = site_z + z_reward;
      float tx = s.spos[3 * tail], ty = s.spos[3 * tail + 1];
      float dx = s.spos[3 * ttail] - tx, dy = s.spos[3 * ttail + 1] - ty;
      float ang = atan2f(dy, dx + 0.00001f);
      float dist = sqrtf(dx * dx + dy * dy) + 0.025f;
      float y_ = dist * sinf(ang), x_ = dist * cosf(ang);
      float newT[2] = {dx - x_ + tx, dy - y_ + ty};
      float e0 = sp[0] - aux_old[0], e1 = sp[1] - aux_old[1];
      float s2c = sqrtf(e0 * e0 + e1 * e1);
      s2c = s2c < 0.02f ? 0.0f : s2c - 0.02f;
      float siet = (1.0f - tanhf(5.0f * s2c)) * W[1];
      float health = W[2] * fabsf((sp[2] < W[3] ? 1.0f : 0.0f) - 1.0f);
      reward = clampf(push + siet + health + site_z, -100.0f, 100.0f);
      done = s.xpos[3 * tbody + 2] < 0.6f ? 1.0f : 0.0f;
      tshape_obs<C>(m, s, tb, tv, xita, newT, obs_lds);
      met[0] = push; met[1] = siet; met[2] = health; met[3] = met_kept; met[4] = site_z;
      rec[L.metrics + 0] = push; rec[L.metrics + 1] = siet; rec[L.metrics + 2] = health; rec[L.metrics + 4] = site_z;
      for (int i = 0; i < 3; ++i) { rec[L.site_pos + i] = sp[i]; rec[L.T_pos + i] = s.xpos[3 * tbody + i]; }
      rec[L.new_T_pos] = newT[0]; rec[L.new_T_pos + 1] = newT[1];
      rec[L.xita] = xita;
    } else {
      const int cube = m.env_ids[ID_CUBE], site = m.env_ids[ID_SITE];
      float cp[3] = {s.xpos[3 * cube], s.xpos[3 * cube + 1], s.xpos[3 * cube + 2]};
      float sp[3] = {s.spos[3 * site], s.spos[3 * site + 1], s.spos[3 * site + 2]};
      float d0 = tp[0] - cp[0], d1 = tp[1] - cp[1], d2 = tp[2] - cp[2];
      const bool sf = m.env_kind == ENV_AIRBOT_SF;
      float btd = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
      if (btd < W[4]) btd = 0.0f;                       // 0.005 (cube_env.py:166) / 0.003 (test/airbot.py:191)
      float push = (1.0f / (1.0f + 3.0f * btd)) * W[0];
      float task_complete = btd < W[4] ? W[5] : 0.0f;   // test/airbot.py:196
      float site_z = sp[2] < 0.82f ? 1.0f : 0.0f;
      float dx = tp[0] - cp[0], dy = tp[1] - cp[1];
      float ang = atan2f(dy, dx + 0.00001f);
      float dist = sqrtf(dx * dx + dy * dy) + 0.04f;
      float y_ = dist * sinf(ang), x_ = dist * cosf(ang);
      float ncp[2] = {dx - x_ + cp[0], dy - y_ + cp[1]};
      float e0 = sp[0] - aux_old[0], e1 = sp[1] - aux_old[1];
      float s2c = sqrtf(e0 * e0 + e1 * e1);
      s2c = s2c < 0.042f ? 0.0f : s2c - 0.042f;
      float siet = (1.0f - tanhf(5.0f * s2c)) * W[1];
      if (btd < 0.005f) siet = W[1];
      float hd = sp[2] < W[3] ? 1.0f : 0.0f;
      if (sf && (sp[0] > 1.0f || sp[0] < -0.6f || sp[1] > 0.3f || sp[1] < -0.3f || cp[2] < 0.6f)) hd = 1.0f;   // test/airbot.py:227-233
      float health = W[2] * fabsf(hd - 1.0f);
      reward = clampf(sf ? push + siet + health + task_complete + site_z : push + siet + health + site_z, -100.0f, 100.0f);
      done = sf ? (btd < W[4] ? 1.0f : 0.0f) : (cp[2] < 0.6f ? 1.0f : 0.0f);
      cube_obs<C>(m, s, tp, ncp, obs_lds);
      met[0] = push; met[1] = met_kept; met[2] = siet;
      rec[L.metrics + 0] = push; rec[L.metrics + 2] = siet;
      for (int i = 0; i < 3; ++i) { rec[L.site_pos + i] = sp[i]; rec[L.cube_pos + i] = cp[i]; }
      rec[L.new_cube_pos] = ncp[0]; rec[L.new_cube_pos + 1] = ncp[1];
    }
    rec[L.reward] = reward;
    // EpisodeWrapper.step (action_repeat = 1)
    if (wrap_episode) {
      steps += 1.0f;
      bool over = steps >= (float)m.episode_length;
      rec[L.truncation] = over ? 1.0f - done : 0.0f;
      // brax: metric = (metric + x) * (1 - prev_done).  Written as a select: the same value for finite metrics, and an env whose
      // simulation went non-finite once (a blow-up) starts its next episode's sums clean instead of carrying NaN * 0 = NaN forever.
      float* em = rec + L.episode_metrics;
      em[0] = prev_done != 0.0f ? 0.0f : em_old[0] + reward;
      em[1] = prev_done != 0.0f ? 0.0f : em_old[1] + 1.0f;
#pragma unroll
      for (int i = 0; i < C::NMET; ++i) em[2 + i] = prev_done != 0.0f ? 0.0f : em_old[2 + i] + met[i];
      if (over) done = 1.0f;
      rec[L.episode_done] = done;
    }
    rec[L.steps] = steps;
    rec[L.done] = done;
    int* st = reinterpret_cast<int*>(rec + L.stats);
    st[0] = f.st.niter; st[1] = f.st.ls_total; st[2] = s.ncon; st[3] = handoff_err ? -1 : s.ncon_drop;
  }
  WSYNC();
  done = rdlane(done, 0);
  if (wrap_autoreset && done != 0.0f) {
    // AutoResetWrapper.step post-step: the cached first state replaces the pipeline state and obs
    for (int t = lane; t < L.persist_end; t += 64) rec[t] = rec[L.f_qpos + t];
    for (int t = lane; t < C::OBS; t += 64) rec[L.obs + t] = rec[L.f_obs + t];
  } else {
    store_pipeline<C>(s, rec, L, lane, warm, time);
    for (int t = lane; t < C::OBS; t += 64) rec[L.obs + t] = obs_lds[t];
  }
#ifdef RSR_PROFILE
  PROF(PS_EPILOGUE)
  if (a.debug && lane == 0) {      // stage cycle counters leave the kernel only through the debug buffer
    float* d = a.debug + (size_t)e * RSR_DEBUG_FLOATS + 7200;
    for (int i = 0; i < PS_COUNT; ++i) d[i] = (float)prof_.acc[i];
  }
#endif
#if defined(RSR_PROFILE) || defined(RSR_TIMELINE)
  if (a.debug && lane == 0) prof_timeline(a.debug + (size_t)e * RSR_DEBUG_FLOATS + 7300 + 8 * phase, prof_rt0_, prof_ct0_);
#endif
  WSYNC();                                                     // the next unit reuses this wave's LDS image
  }
}

}  // namespace rsr
