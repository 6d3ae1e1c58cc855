// rsr_go2.hpp -- the Go2 env kernels: joystick (go2/joystick.py) and handstand / footstand (go2/handstand.py).
#pragma once
#include "rsr_go2_sensors.hpp"

namespace rsr {

enum { RW_TRACK_LIN = 0, RW_TRACK_ANG, RW_LIN_VEL_Z, RW_ANG_VEL_XY, RW_ORIENT, RW_DOF_LIMITS, RW_POSE, RW_TERM, RW_STAND_STILL,
       RW_TORQUES, RW_ACTION_RATE, RW_ENERGY, RW_FEET_CLEAR, RW_FEET_HEIGHT, RW_FEET_SLIP, RW_FEET_AIR, RW_ALL_FEET_AIR,
       RW_SYM_GAIT, RW_LR_SYM, RW_FB_SYM, RW_FEET_OFF_STILL, RW_COUNT };

// joystick.py:284-340: 48-dim "state" obs into obs_lds; advances ginfo rng by five splits.  The five splits are a serial
// chain of register-only evaluations; the five draws (3, 3, 3, 12, 12 elements) are then one evaluation with a lane per
// word pair and one barrier (ten evaluations with two barriers each when every split and draw went through LDS).
template <class C>
__device__ __forceinline__ void go2_obs(const DModel& m, Smem<C>& s, const G2Sens& sn, float* obs_lds, uint32_t* bits, int lane, float home_l) {
#pragma clang fp contract(off)
  const float* F = m.env_go2f;
  const bool idel = m.env_go2i[1] > 0;
  uint32_t rng0 = __float_as_uint(s.ginfo[G2_RNG]), rng1 = __float_as_uint(s.ginfo[G2_RNG + 1]);
  rng0 = (uint32_t)uniform_i((int)rng0); rng1 = (uint32_t)uniform_i((int)rng1);
  const float level = F[2];
  // order of the draws: gyro, gravity, linvel, joint angles, joint velocities
  uint32_t dk[5][2];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    uint32_t ks[2][2];
    tf_split_reg<2>(rng0, rng1, lane, ks);
    rng0 = ks[0][0]; rng1 = ks[0][1]; dk[d][0] = ks[1][0]; dk[d][1] = ks[1][1];
  }
  {
    // lanes [0,2) [2,4) [4,6): the three 3-element draws; [6,12) [12,18): the two 12-element draws
    const int d = lane < 6 ? (lane >> 1) : (lane < 12 ? 3 : 4);
    const int idx = lane < 6 ? (lane & 1) : (lane < 12 ? lane - 6 : lane - 12);
    uint32_t k0 = dk[4][0], k1 = dk[4][1];
#pragma unroll
    for (int q = 3; q >= 0; --q) if (d == q) { k0 = dk[q][0]; k1 = dk[q][1]; }
    WSYNC();
    tf_bits_batched(k0, k1, d < 3 ? 3 : 12, idx, d < 3 ? 3 * d : (d == 3 ? 9 : 21), lane < 18, bits);
    WSYNC();
  }
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    const int n = d < 3 ? 3 : 12, off = d < 3 ? 3 * d : (d == 3 ? 9 : 21);
    if (lane < n) {
      const float u = uniform_from_bits(bits[off + lane], 0.0f, 1.0f);
      float src, scale; int dst;
      if (d == 0) { src = idel ? s.ginfo[G2_GYRO_BUF + lane] : pick3(sn.gyro, lane); scale = F[5]; dst = 3 + lane; }
      else if (d == 1) { src = idel ? s.ginfo[G2_GRAV_BUF + lane] : pick3(sn.gravity, lane); scale = F[6]; dst = 6 + lane; }
      else if (d == 2) { src = idel ? s.ginfo[G2_LINVEL_BUF + lane] : pick3(sn.linvel, lane); scale = F[7]; dst = lane; }
      else if (d == 3) { src = s.qpos[7 + lane]; scale = F[3]; dst = 9 + lane; }
      else { src = s.qvel[6 + lane]; scale = F[4]; dst = 21 + lane; }
      float a = 2.0f * u; float b = a - 1.0f; float c = b * level; float e = c * scale;
      float val = src + e;
      if (d == 3) val = val - home_l;             // home_l = env_go2_home[7 + lane] (lanes < 12), loaded by the caller ahead of time
      obs_lds[dst] = val;
    }
  }
  if (lane < 12) obs_lds[33 + lane] = s.ginfo[G2_LAST_ACT + lane];
  if (lane < 3) obs_lds[45 + lane] = s.ginfo[G2_CMD + lane];
  if (lane == 0) { s.ginfo[G2_RNG] = __uint_as_float(rng0); s.ginfo[G2_RNG + 1] = __uint_as_float(rng1); }
  WSYNC();
}

// joystick.py:341-366: element t of obs["privileged_state"]; read right after go2_obs (info: old last_contact, air + dt)
template <class C>
__device__ __forceinline__ float go2_priv_elem(const DModel& m, const Smem<C>& s, const G2Sens& sn, const float* obs_lds, int t) {
  if (t < 48) return obs_lds[t];
  t -= 48;
  if (t < 3) return pick3(sn.gyro, t);
  if (t < 6) return pick3(sn.accel, t - 3);
  if (t < 9) return pick3(sn.gravity, t - 6);
  if (t < 12) return pick3(sn.linvel, t - 9);
  if (t < 15) return pick3(sn.gang, t - 12);
  if (t < 27) return s.qpos[7 + t - 15] - m.env_go2_home[7 + t - 15];
  if (t < 39) return s.qvel[6 + t - 27];
  if (t < 51) return s.aforce[t - 39];
  if (t < 55) return s.ginfo[G2_LAST_CONTACT + t - 51];
  if (t < 67) { int k = t - 55; return s.slinvel[3 * m.env_ids[1 + k / 3] + k % 3]; }
  if (t < 71) return s.ginfo[G2_AIR + t - 67];
  if (t < 74) return s.ginfo[G2_XFRC + t - 71];
  return s.ginfo[G2_SINCE_PERT] >= s.ginfo[G2_STEPS_PERT] ? 1.0f : 0.0f;
}

// The same element fetched as a gather: every element but the 15 sensor values (registers) and the kick flag is one LDS
// word, so the lanes compute an address with selects and issue ONE load (go2_priv_elem walks fifteen divergent branches,
// each waiting for its own load).  FIRST: t < 64 (the only elements that can be sensor values).  foot_site: env_ids[1..4].
template <class C, bool FIRST>
__device__ __forceinline__ float go2_priv_gather(const DModel& m, const Smem<C>& s, const G2Sens& sn, const float* obs_lds, int t,
                                                 const int (&foot_site)[4], float kick_flag, float home_l) {
#pragma clang fp contract(off)
  const int k = t - 48;
  const float* p = obs_lds + (t < 48 ? t : 0);
  p = (k >= 15 && k < 27) ? &s.qpos[7 + (k - 15)] : p;
  p = (k >= 27 && k < 39) ? &s.qvel[6 + (k - 27)] : p;
  p = (k >= 39 && k < 51) ? &s.aforce[k - 39] : p;
  p = (k >= 51 && k < 55) ? &s.ginfo[G2_LAST_CONTACT + (k - 51)] : p;
  {
    const int kk = k - 55, ft = kk / 3;
    const int site = ft == 0 ? foot_site[0] : ft == 1 ? foot_site[1] : ft == 2 ? foot_site[2] : foot_site[3];
    p = (k >= 55 && k < 67) ? &s.slinvel[3 * site + (kk - 3 * ft)] : p;
  }
  p = (k >= 67 && k < 71) ? &s.ginfo[G2_AIR + (k - 67)] : p;
  p = (k >= 71 && k < 74) ? &s.ginfo[G2_XFRC + (k - 71)] : p;
  const int hk = k - 15 < 0 ? 0 : (k - 15 > 11 ? 11 : k - 15);
  const float h = __shfl(home_l, hk);            // lane j holds home[7 + j]
  float v = *p;
  if (k >= 15 && k < 27) v = v - h;
  if constexpr (FIRST) {
    const int grp = k < 0 ? 0 : k / 3, comp = k < 0 ? 0 : k - 3 * grp;
    const float v_gy = pick3(sn.gyro, comp), v_ac = pick3(sn.accel, comp), v_gr = pick3(sn.gravity, comp), v_li = pick3(sn.linvel, comp), v_ga = pick3(sn.gang, comp);
    const float sv = grp == 0 ? v_gy : (grp == 1 ? v_ac : (grp == 2 ? v_gr : (grp == 3 ? v_li : v_ga)));
    if (k >= 0 && k < 15) v = sv;
  }
  if (k == 74) v = kick_flag;
  return v;
}

// ---------------------------------------------------------------- Go2 reset kernel (joystick.py:123-203 + wrappers)
template <class C>
__global__ __launch_bounds__(64) void go2_reset_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  float* rec = a.state + (size_t)e * L.rec;
  const float* F = m.env_go2f;
  uint32_t* bits = reinterpret_cast<uint32_t*>(s.scratch_b());
  float* obs_lds = s.scratch_b() + 64;
  load_overrides<C>(m, s, a, e, lane);
  for (int t = lane; t < C::NINFO; t += 64) s.ginfo[t] = 0.0f;
  uint32_t rng0 = a.keys[2 * e], rng1 = a.keys[2 * e + 1], ks[4][2];
  if (lane < C::NQ) s.qpos[lane] = m.env_go2_home[lane];
  if (lane < C::NV) s.qvel[lane] = 0.0f;
  {
    uint32_t k2[2][2];
    tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
    float dxy = tf_uniform(k2[1][0], k2[1][1], 2, -0.5f, 0.5f, bits, lane);
    if (lane < 2) s.qpos[lane] = m.env_go2_home[lane] + dxy;
    tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
    float yaw = rdlane(tf_uniform(k2[1][0], k2[1][1], 1, -3.14f, 3.14f, bits, lane), 0);
    if (lane == 0) {
#pragma clang fp contract(off)
      float sn = sinf(yaw * 0.5f), cs = cosf(yaw * 0.5f);
      Q4 q = Q4{m.env_go2_home[3], m.env_go2_home[4], m.env_go2_home[5], m.env_go2_home[6]}, r = Q4{cs, 0.0f * sn, 0.0f * sn, 1.0f * sn};
      Q4 o;
      o.w = q.w * r.w - q.x * r.x - q.y * r.y - q.z * r.z;
      o.x = q.w * r.x + q.x * r.w + q.y * r.z - q.z * r.y;
      o.y = q.w * r.y - q.x * r.z + q.y * r.w + q.z * r.x;
      o.z = q.w * r.z + q.x * r.y - q.y * r.x + q.z * r.w;
      st4(&s.qpos[3], o);
    }
    tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
    float v6 = tf_uniform(k2[1][0], k2[1][1], 6, -0.5f, 0.5f, bits, lane);
    if (lane < 6) s.qvel[lane] = v6;
  }
  WSYNC();
  if (lane < C::NU) s.ctrl[lane] = s.qpos[7 + lane];          // mjx_env.init(..., ctrl = qpos[7:])
  if (lane == 0) { s.xfrc_body = 0; s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  WSYNC();
  float Mrow[C::NV], warm = 0.0f;
  FwdOut<C> f;
  PROF_DECL
  forward<C>(m, hot, s, lane, Mrow, warm, f, a.debug ? a.debug + (size_t)e * RSR_DEBUG_FLOATS : nullptr PROF_PASS);
  WSYNC();
  tf_split<4>(rng0, rng1, bits, lane, ks); rng0 = ks[0][0]; rng1 = ks[0][1];
  {
    float t_pert = rdlane(tf_uniform(ks[1][0], ks[1][1], 1, F[17], F[18], bits, lane), 0);
    float dur = rdlane(tf_uniform(ks[2][0], ks[2][1], 1, F[19], F[20], bits, lane), 0);
    float mag = rdlane(tf_uniform(ks[3][0], ks[3][1], 1, F[21], F[22], bits, lane), 0);
    if (lane == 0) {
      s.ginfo[G2_STEPS_PERT] = rintf(t_pert / F[0]); s.ginfo[G2_PERT_DUR_S] = dur;
      s.ginfo[G2_PERT_DUR] = rintf(dur / F[0]); s.ginfo[G2_PERT_MAG] = mag;
    }
  }
  {
    uint32_t k3[3][2];
    tf_split<3>(rng0, rng1, bits, lane, k3); rng0 = k3[0][0]; rng1 = k3[0][1];
    float uu = rdlane(tf_uniform(k3[1][0], k3[1][1], 1, 0.0f, 1.0f, bits, lane), 0);
    float amp = lane < 3 ? F[10 + lane] : 0.0f;
    float cmd = tf_uniform(k3[2][0], k3[2][1], 3, -amp, amp, bits, lane);
    if (lane < 3) s.ginfo[G2_CMD + lane] = cmd;
    if (lane == 0) {
#pragma clang fp contract(off)
      float t_cmd = -log1pf(-uu) * F[16];
      s.ginfo[G2_STEPS_CMD] = rintf(t_cmd / F[0]);
      s.ginfo[G2_RNG] = __uint_as_float(rng0); s.ginfo[G2_RNG + 1] = __uint_as_float(rng1);
    }
  }
  WSYNC();
  G2Sens sn;
  go2_sensors<C>(m, s, sn);
  go2_accelerometer<C>(m, s, lane, f.qacc, sn);
  go2_obs<C>(m, s, sn, obs_lds, bits, lane, m.env_go2_home[7 + (lane < 12 ? lane : 0)]);
  for (int t = lane; t < GO2_PRIV; t += 64) { float v = go2_priv_elem<C>(m, s, sn, obs_lds, t); rec[L.priv_obs + t] = v; rec[L.f_priv_obs + t] = v; }
  store_pipeline<C>(s, rec, L, lane, warm, 0.0f);
  for (int t = lane; t < C::NINFO; t += 64) rec[L.go2_info + t] = s.ginfo[t];
  for (int t = lane; t < C::OBS; t += 64) { rec[L.obs + t] = obs_lds[t]; rec[L.f_obs + t] = obs_lds[t]; }
  if (lane == 0) {
    store_reset_outputs<C>(s, f, rec, L);
    rec[L.f_time] = 0.0f;
  }
  store_first_state<C>(s, rec, L, lane, warm, false);
}

// ---------------------------------------------------------------- Go2 step kernel (joystick.py:204-280 + wrappers)
template <class C>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RSR_GO2_WAVES_PER_EU, RSR_GO2_WAVES_PER_EU)))
void go2_step_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  float* rec = a.state + (size_t)e * L.rec;
  const bool wrap_episode = m.wrap_flags & 1, wrap_autoreset = (m.wrap_flags & 2) != 0;
  const float* F = m.env_go2f;
  const float dt = F[0];
  uint32_t* bits = reinterpret_cast<uint32_t*>(s.scratch_b());
  float* obs_lds = s.scratch_b() + 64;
  float* rwl = s.scratch_b() + 128;                                   // scaled reward terms staged for the metrics write
  PROF_DECL
  float warm = 0.0f, time;
  load_pipeline<C>(s, rec, L, lane, warm, time);
  load_overrides<C>(m, s, a, e, lane);
  for (int t = lane; t < C::NINFO; t += 64) s.ginfo[t] = rec[L.go2_info + t];
  const float done_prev = rec[L.done];
  float steps = rec[L.steps];
  if (wrap_autoreset && done_prev != 0.0f) steps = 0.0f;
  const float act_in = lane < C::NU ? a.action[(size_t)e * C::NU + lane] : 0.0f;
  WSYNC();
  // ---- perturbation kick (:594-644): half-sine force pulse on the torso, or wait and draw the next direction ----
  if (m.env_go2i[2]) {
    const bool kicking = s.ginfo[G2_SINCE_PERT] >= s.ginfo[G2_STEPS_PERT];      // wave-uniform (LDS)
    if (kicking) {
      WSYNC();
      if (lane == 0) {
#pragma clang fp contract(off)
        float t = s.ginfo[G2_PERT_STEPS] * dt;
        float ph = 3.14159265358979323846f * t;
        float u_t = 0.5f * sinf(ph / s.ginfo[G2_PERT_DUR_S]);
        float f1 = u_t * F[23]; float f2 = f1 * s.ginfo[G2_PERT_MAG];
        float force = f2 / s.ginfo[G2_PERT_DUR_S];
        for (int c = 0; c < 3; ++c) s.ginfo[G2_XFRC + c] = force * s.ginfo[G2_PERT_DIR + c];
        if (s.ginfo[G2_PERT_STEPS] >= s.ginfo[G2_PERT_DUR]) s.ginfo[G2_SINCE_PERT] = 0.0f;
        s.ginfo[G2_PERT_STEPS] += 1.0f;
      }
    } else {
      uint32_t k2[2][2];
      tf_split<2>(__float_as_uint(s.ginfo[G2_RNG]), __float_as_uint(s.ginfo[G2_RNG + 1]), bits, lane, k2);
      float angle = rdlane(tf_uniform(k2[1][0], k2[1][1], 1, 0.0f, 6.2831855f, bits, lane), 0);
      WSYNC();
      if (lane == 0) {
        s.ginfo[G2_RNG] = __uint_as_float(k2[0][0]); s.ginfo[G2_RNG + 1] = __uint_as_float(k2[0][1]);
        float since = s.ginfo[G2_SINCE_PERT] + 1.0f;
        s.ginfo[G2_SINCE_PERT] = since;
        s.ginfo[G2_XFRC] = 0.0f; s.ginfo[G2_XFRC + 1] = 0.0f; s.ginfo[G2_XFRC + 2] = 0.0f;
        if (since >= s.ginfo[G2_STEPS_PERT]) {
          s.ginfo[G2_PERT_STEPS] = 0.0f;
          s.ginfo[G2_PERT_DIR] = cosf(angle); s.ginfo[G2_PERT_DIR + 1] = sinf(angle); s.ginfo[G2_PERT_DIR + 2] = 0.0f;
        }
      }
    }
    WSYNC();
  }
  if (lane == 0) {
    s.acc_body = m.site_bodyid[m.env_ids[0]];
    s.xfrc_body = m.env_go2i[2] ? m.env_ids[10] : 0;
    s.xfrc[0] = s.ginfo[G2_XFRC]; s.xfrc[1] = s.ginfo[G2_XFRC + 1]; s.xfrc[2] = s.ginfo[G2_XFRC + 2];
  }
  WSYNC();
  // ---- action delay FIFO (:207-215) and motor targets (:216) ----
  const int adel = m.env_go2i[0];
  float actual = act_in;
  if (adel > 0) {
    float shifted = 0.0f;
    const int nbuf = adel * C::NU;
    if (lane < C::NU) actual = s.ginfo[G2_ACT_BUF + lane];
    if (lane < nbuf) shifted = s.ginfo[G2_ACT_BUF + C::NU + lane];
    WSYNC();
    if (lane < nbuf) s.ginfo[G2_ACT_BUF + lane] = shifted;
    if (lane < C::NU) s.ginfo[G2_ACT_BUF + nbuf + lane] = act_in;
  }
  if (lane < C::NU) {
#pragma clang fp contract(off)
    float sc = actual * F[1];
    s.ctrl[lane] = m.env_go2_home[7 + lane] + sc;
  }
  WSYNC();
  PROF(PS_LOAD)
  float Mrow[C::NV];
  FwdOut<C> f;
  const int prio_q = prio_quarter(a, e);
  for (int fr = 0; fr < m.n_frames; ++fr) {
#if defined(RSR_PROFILE) || defined(RSR_TIMELINE)
    float* dbg = nullptr;
#else
    float* dbg = (a.debug && fr == m.n_frames - 1) ? a.debug + (size_t)e * RSR_DEBUG_FLOATS : nullptr;
#endif
    const int lane_s = lrec_lane(lane);        // see step_kernel
    prio_substep(a.prio_mode, prio_q, fr);
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, dbg PROF_PASS);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    time += hot.timestep;
  }
  // per-joint constants of the epilogue (home pose, soft limits): vector loads take a couple of thousand cycles under load, so
  // they are issued here and consumed after the sensor / FIFO / contact code
  const int jl = lrec_lane(lane < 12 ? lane : 0);      // opaque: not merged with the prologue's load of the same address, which
                                                        // would keep the value live (or spilled) across the whole substep loop
  const float home_l = m.env_go2_home[7 + jl], soft_lo = m.env_go2_soft[jl], soft_hi = m.env_go2_soft[12 + jl];
  // (the Episode wrapper's running sums and the feet of the contact pairs likewise)
  int foot_of_pair = -1;                    // lane p < NP: the foot whose geom pair p holds (pairs are static), or -1
  if (lane < C::NP) {
    const int g1 = m.pair_geom1[lane], g2 = m.pair_geom2[lane], fl = m.env_ids[5];
#pragma unroll
    for (int fi = 0; fi < 4; ++fi) { const int gf = m.env_ids[6 + fi]; if ((g2 == gf && g1 == fl) || (g1 == gf && g2 == fl)) foot_of_pair = fi; }
  }
  const float prev_done = wrap_episode ? rec[L.episode_done] : 0.0f;
  const float em_old = (wrap_episode && lane < C::NMET + 2) ? rec[L.episode_metrics + lane] : 0.0f;
  // ---- sensors of the last forward pass, IMU FIFOs (:220-235) ----
  G2Sens sn;
  go2_sensors<C>(m, s, sn);
  go2_accelerometer<C>(m, s, lane, f.qacc, sn);
  PROF(PS_E_SENS)
  const int idel = m.env_go2i[1];
  if (idel > 0) {
    float v = 0.0f;
    const int nb = idel * 3;
    int base = lane < nb ? G2_GYRO_BUF : (lane < 2 * nb ? G2_LINVEL_BUF : G2_GRAV_BUF);
    int off = lane < nb ? lane : (lane < 2 * nb ? lane - nb : lane - 2 * nb);
    if (lane < 3 * nb) v = s.ginfo[base + 3 + off];
    WSYNC();
    if (lane < 3 * nb) s.ginfo[base + off] = v;
    if (lane < 3) { s.ginfo[G2_GYRO_BUF + nb + lane] = pick3(sn.gyro, lane); s.ginfo[G2_LINVEL_BUF + nb + lane] = pick3(sn.linvel, lane); s.ginfo[G2_GRAV_BUF + nb + lane] = pick3(sn.gravity, lane); }
    WSYNC();
  }
  PROF(PS_E_FIFO)
  // ---- foot contacts (:236-245) ----
  // lane p < NP knows which foot pair p belongs to (the pairs are static); lane i < ncon looks its contact's pair up there
  int contact[4];
  int foot_site[4];
#pragma unroll
  for (int fi = 0; fi < 4; ++fi) foot_site[fi] = m.env_ids[1 + fi];
  {
    const int nc = s.ncon, ci = lane < nc ? lane : 0;
    const int cp = s.cpair[ci]; const float cd = s.cdist[ci];
    const int fo = __shfl(foot_of_pair, cp & 63);
    const int my_foot = (lane < nc && cd < 0.0f) ? fo : -1;
#pragma unroll
    for (int fi = 0; fi < 4; ++fi) contact[fi] = __ballot(my_foot == fi) != 0ull ? 1 : 0;
  }
  int first_contact[4]; float feet_z[4];
  for (int fi = 0; fi < 4; ++fi) {
    bool filt = contact[fi] || s.ginfo[G2_LAST_CONTACT + fi] != 0.0f;
    first_contact[fi] = (s.ginfo[G2_AIR + fi] > 0.0f) && filt;
    feet_z[fi] = s.spos[3 * foot_site[fi] + 2];
  }
  WSYNC();
  if (lane < 4) {
    s.ginfo[G2_AIR + lane] += dt;
    s.ginfo[G2_SWING + lane] = fmaxf(s.ginfo[G2_SWING + lane], s.spos[3 * (lane == 0 ? foot_site[0] : lane == 1 ? foot_site[1] : lane == 2 ? foot_site[2] : foot_site[3]) + 2]);
  }
  WSYNC();
  PROF(PS_E_FEET)
  go2_obs<C>(m, s, sn, obs_lds, bits, lane, home_l);
  PROF(PS_E_OBS)
  float priv[2];                                              // this lane's elements of privileged_state (info as of now)
  {
    const float kick_flag = s.ginfo[G2_SINCE_PERT] >= s.ginfo[G2_STEPS_PERT] ? 1.0f : 0.0f;
    priv[0] = go2_priv_gather<C, true>(m, s, sn, obs_lds, lane, foot_site, kick_flag, home_l);
    priv[1] = go2_priv_gather<C, false>(m, s, sn, obs_lds, lane + 64 < GO2_PRIV ? lane + 64 : GO2_PRIV - 1, foot_site, kick_flag, home_l);
  }
  float done = sn.up[2] < 0.0f ? 1.0f : 0.0f;
  PROF(PS_E_PRIV)
  // ---- rewards (:367-593): the per-joint pieces of the seven 12-term sums are computed by lanes 0..11 and staged; lane 0 adds
  // them up in the reference's order and evaluates the rest of the scalar algebra op by op ----
  float* rstage = s.scratch_b() + 160;                        // [7][12]
  if (lane < 12) {
#pragma clang fp contract(off)
    const float q = s.qpos[7 + lane], dq = q - home_l;
    const float lo_ = q - soft_lo, hi_ = q - soft_hi;
    const float w = (lane % 3 == 2) ? 0.1f : 1.0f;
    const float t = s.aforce[lane];
    const float dd = act_in - s.ginfo[G2_LAST_ACT + lane];
    rstage[lane] = fabsf(dq);
    rstage[12 + lane] = -(lo_ < 0.0f ? lo_ : 0.0f) + (hi_ > 0.0f ? hi_ : 0.0f);
    rstage[24 + lane] = dq * dq * w;
    rstage[36 + lane] = t * t;
    rstage[48 + lane] = fabsf(t);
    rstage[60 + lane] = fabsf(s.qvel[6 + lane]) * fabsf(t);
    rstage[72 + lane] = dd * dd;
  }
  WSYNC();
  float reward = 0.0f;
  if (lane == 0) {
#pragma clang fp contract(off)
    const float* SC = m.env_go2_scales;
    const float* cmd = &s.ginfo[G2_CMD];
    float cmd_norm = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1] + cmd[2] * cmd[2]);
    float moving = cmd_norm > 0.01f ? 1.0f : 0.0f, still = cmd_norm < 0.01f ? 1.0f : 0.0f;
    float rw[RW_COUNT];
    {
      float e0 = cmd[0] - sn.linvel[0], e1 = cmd[1] - sn.linvel[1];
      rw[RW_TRACK_LIN] = expf(-(e0 * e0 + e1 * e1) / F[8]);
      float ea = cmd[2] - sn.gyro[2];
      rw[RW_TRACK_ANG] = expf(-(ea * ea) / F[8]);
    }
    rw[RW_LIN_VEL_Z] = sn.glin[2] * sn.glin[2];
    rw[RW_ANG_VEL_XY] = sn.gang[0] * sn.gang[0] + sn.gang[1] * sn.gang[1];
    rw[RW_ORIENT] = sn.up[0] * sn.up[0] + sn.up[1] * sn.up[1];
    {
      float sa = 0, lim = 0, pose = 0, s2 = 0, s1 = 0, en = 0, ar = 0;
#pragma unroll 1
      for (int i0 = 0; i0 < 12; i0 += 4) {
#pragma unroll
        for (int i = i0; i < i0 + 4; ++i) {
          sa += rstage[i]; lim += rstage[12 + i]; pose += rstage[24 + i];
          s2 += rstage[36 + i]; s1 += rstage[48 + i]; en += rstage[60 + i]; ar += rstage[72 + i];
        }
      }
      rw[RW_STAND_STILL] = sa * still; rw[RW_DOF_LIMITS] = lim; rw[RW_POSE] = expf(-pose);
      rw[RW_TERM] = done;
      rw[RW_TORQUES] = sqrtf(s2) + s1; rw[RW_ENERGY] = en; rw[RW_ACTION_RATE] = ar;
    }
    {
      float slip = 0, clear = 0, height = 0, air = 0; int nair = 0;
      for (int fi = 0; fi < 4; ++fi) {
        const int sid = foot_site[fi];
        float vx = s.slinvel[3 * sid], vy = s.slinvel[3 * sid + 1];
        float v2 = vx * vx + vy * vy;
        slip += v2 * (float)contact[fi];
        clear += fabsf(feet_z[fi] - F[9]) * sqrtf(sqrtf(v2));
        float err = s.ginfo[G2_SWING + fi] / F[9] - 1.0f;
        height += err * err * (float)first_contact[fi];
        air += (s.ginfo[G2_AIR + fi] - 0.1f) * (float)first_contact[fi];
        nair += !contact[fi];
      }
      rw[RW_FEET_SLIP] = slip * moving; rw[RW_FEET_CLEAR] = clear; rw[RW_FEET_HEIGHT] = height * moving; rw[RW_FEET_AIR] = air * moving;
      rw[RW_ALL_FEET_AIR] = (nair >= 3 ? 1.0f : 0.0f) * moving;
      rw[RW_FEET_OFF_STILL] = (float)nair * still;
      float p1 = 0, p2 = 0;
      for (int i = 0; i < 3; ++i) { float x = s.qpos[7 + 3 + i] - s.qpos[7 + 6 + i], y = s.qpos[7 + i] - s.qpos[7 + 9 + i]; p1 += x * x; p2 += y * y; }
      rw[RW_SYM_GAIT] = (p1 + p2) * moving;
      const float* at = &s.ginfo[G2_AIR]; const float* ct = &s.ginfo[G2_CONTACT_T];
      float la = (at[1] + at[3]) / 2.0f, lc = (ct[1] + ct[3]) / 2.0f, ra = (at[0] + at[2]) / 2.0f, rc = (ct[0] + ct[2]) / 2.0f;
      rw[RW_LR_SYM] = ((la - ra) * (la - ra) + (lc - rc) * (lc - rc)) * moving;
      float fa = (at[0] + at[1]) / 2.0f, fc = (ct[0] + ct[1]) / 2.0f, ba = (at[2] + at[3]) / 2.0f, bc = (ct[2] + ct[3]) / 2.0f;
      rw[RW_FB_SYM] = ((fa - ba) * (fa - ba) + (fc - bc) * (fc - bc)) * moving;
    }
    for (int k = 0; k < RW_COUNT; ++k) { rw[k] = rw[k] * SC[k]; rwl[k] = rw[k]; }
    const int order[RW_COUNT] = {RW_TRACK_LIN, RW_TRACK_ANG, RW_LIN_VEL_Z, RW_ANG_VEL_XY, RW_ORIENT, RW_STAND_STILL, RW_TERM, RW_POSE,
                                 RW_TORQUES, RW_ACTION_RATE, RW_ENERGY, RW_FEET_SLIP, RW_FEET_CLEAR, RW_FEET_HEIGHT, RW_FEET_AIR,
                                 RW_DOF_LIMITS, RW_ALL_FEET_AIR, RW_SYM_GAIT, RW_LR_SYM, RW_FB_SYM, RW_FEET_OFF_STILL};
    float total = 0.0f;
    for (int k = 0; k < RW_COUNT; ++k) total = total + rwl[order[k]];
    reward = clampf(total * dt, 0.0f, 10000.0f);
  }
  reward = rdlane(reward, 0);
  WSYNC();
  PROF(PS_E_REWARD)
  // ---- bookkeeping (:255-277): last actions, command resampling (threefry), timers ----
  if (lane < C::NU) { s.ginfo[G2_LAST_LAST_ACT + lane] = s.ginfo[G2_LAST_ACT + lane]; s.ginfo[G2_LAST_ACT + lane] = act_in; }
  float steps_cmd = s.ginfo[G2_STEPS_CMD] - 1.0f;
  {
    uint32_t rng0 = __float_as_uint(s.ginfo[G2_RNG]), rng1 = __float_as_uint(s.ginfo[G2_RNG + 1]);
    uint32_t k3[3][2], k4[4][2];
    rng0 = (uint32_t)uniform_i((int)rng0); rng1 = (uint32_t)uniform_i((int)rng1);
    tf_split_reg<3>(rng0, rng1, lane, k3);
    tf_split_reg<4>(k3[1][0], k3[1][1], lane, k4);          // sample_command: rng, y_rng, w_rng, z_rng
    float amp = lane < 3 ? F[10 + lane] : 0.0f;
    {
      // the four draws in one evaluation: lanes [0,2) y, [2,4) z, [4,6) w (3 elements each), lane 6 the resampling time (1)
      const int d = lane < 6 ? (lane >> 1) : 3;
      uint32_t k0 = k3[2][0], k1 = k3[2][1];
      if (d == 0) { k0 = k4[1][0]; k1 = k4[1][1]; }
      if (d == 1) { k0 = k4[3][0]; k1 = k4[3][1]; }
      if (d == 2) { k0 = k4[2][0]; k1 = k4[2][1]; }
      WSYNC();
      tf_bits_batched(k0, k1, d < 3 ? 3 : 1, lane < 6 ? (lane & 1) : 0, 3 * d, lane < 7, bits);
      WSYNC();
    }
    const float y = lane < 3 ? uniform_from_bits(bits[lane], -amp, amp) : 0.0f;
    const float uz = lane < 3 ? uniform_from_bits(bits[3 + lane], 0.0f, 1.0f) : 0.0f;
    const float uw = lane < 3 ? uniform_from_bits(bits[6 + lane], 0.0f, 1.0f) : 0.0f;
    const float uu = uniform_from_bits(bits[9], 0.0f, 1.0f);
    WSYNC();
    if (lane < 3 && steps_cmd <= 0.0f) {
#pragma clang fp contract(off)
      float z = uz < F[13 + lane] ? 1.0f : 0.0f, w = uw < 0.5f ? 1.0f : 0.0f;
      float x = s.ginfo[G2_CMD + lane];
      float yz = y * z; float dif = x - yz; float wd = w * dif;
      s.ginfo[G2_CMD + lane] = x - wd;
    }
    if (lane == 0) {
#pragma clang fp contract(off)
      if (done != 0.0f || steps_cmd <= 0.0f) { float t1 = -log1pf(-uu) * F[16]; steps_cmd = rintf(t1 / dt); }
      s.ginfo[G2_STEPS_CMD] = steps_cmd;
      s.ginfo[G2_RNG] = __uint_as_float(k3[0][0]); s.ginfo[G2_RNG + 1] = __uint_as_float(k3[0][1]);
    }
  }
  if (lane < 4) {
#pragma clang fp contract(off)
    float c = (float)(lane == 0 ? contact[0] : (lane == 1 ? contact[1] : (lane == 2 ? contact[2] : contact[3]))), nc = 1.0f - c;   // (no lane-indexed array: scratch)
    s.ginfo[G2_AIR + lane] = (s.ginfo[G2_AIR + lane] + dt) * nc;
    s.ginfo[G2_CONTACT_T + lane] = (s.ginfo[G2_CONTACT_T + lane] + dt) * c;
    s.ginfo[G2_LAST_CONTACT + lane] = c;
    s.ginfo[G2_SWING + lane] *= nc;
  }
  WSYNC();
  if (lane == 0) {
#pragma clang fp contract(off)
    float swing_mean = (((s.ginfo[G2_SWING] + s.ginfo[G2_SWING + 1]) + s.ginfo[G2_SWING + 2]) + s.ginfo[G2_SWING + 3]) / 4.0f;
    rwl[RW_COUNT] = swing_mean;
  }
  WSYNC();
  {
    // metrics and the Episode wrapper's sums: one lane per entry (rwl[0..NMET) = the scaled terms + swing_peak)
    bool over = false;
    float trunc = 0.0f;
    if (wrap_episode) {
      steps += 1.0f;
      over = steps >= (float)m.episode_length;
      trunc = over ? 1.0f - done : 0.0f;
    }
    if (lane < C::NMET) rec[L.metrics + lane] = rwl[lane];
    if (wrap_episode && lane < C::NMET + 2) {
      float* em = rec + L.episode_metrics;
      const float add = lane == 0 ? reward : (lane == 1 ? 1.0f : rwl[lane >= 2 ? lane - 2 : 0]);
      em[lane] = prev_done != 0.0f ? 0.0f : em_old + add;
    }
    if (over) done = 1.0f;
    if (lane == 0) {
      rec[L.reward] = reward;
      if (wrap_episode) { rec[L.truncation] = trunc; rec[L.episode_done] = done; }
      rec[L.steps] = steps;
      rec[L.done] = done;
      int* st = reinterpret_cast<int*>(rec + L.stats);
      st[0] = f.st.niter; st[1] = f.st.ls_total; st[2] = s.ncon; st[3] = s.ncon_drop;
    }
  }
  WSYNC();
  PROF(PS_E_BOOK)
  if (wrap_autoreset && done != 0.0f && lane < 3) s.ginfo[G2_XFRC + lane] = 0.0f;     // xfrc_applied belongs to `data`: back to the first state's zeros
  WSYNC();
  for (int t = lane; t < C::NINFO; t += 64) rec[L.go2_info + t] = s.ginfo[t];       // info is never reset by AutoReset
  if (wrap_autoreset && done != 0.0f) {
    for (int t = lane; t < L.persist_end; t += 64) rec[t] = rec[L.f_qpos + t];
    for (int t = lane; t < C::OBS; t += 64) rec[L.obs + t] = rec[L.f_obs + t];
    for (int t = lane; t < GO2_PRIV; t += 64) rec[L.priv_obs + t] = rec[L.f_priv_obs + t];
  } else {
    store_pipeline<C>(s, rec, L, lane, warm, time);
    for (int t = lane; t < C::OBS; t += 64) rec[L.obs + t] = obs_lds[t];
    rec[L.priv_obs + lane] = priv[0];
    if (lane + 64 < GO2_PRIV) rec[L.priv_obs + lane + 64] = priv[1];
  }
#ifdef RSR_PROFILE
  PROF(PS_EPILOGUE)
  if (a.debug && lane == 0) {
    float* d = a.debug + (size_t)e * RSR_DEBUG_FLOATS + 7200;
    for (int i = 0; i < PS_COUNT; ++i) d[i] = (float)prof_.acc[i];
  }
#endif
#if defined(RSR_PROFILE) || defined(RSR_TIMELINE)
  if (a.debug && lane == 0) prof_timeline(a.debug + (size_t)e * RSR_DEBUG_FLOATS + 7300, prof_rt0_, prof_ct0_);
#endif
}


// ================================================================ Go2 Handstand / Footstand (go2/handstand.py)
// env_ids: 0 imu site, 1 floor geom, 2..13 the twelve unwanted-contact geoms, 14..15 the feet geoms of the contact cost, 16 trunk body.
// env_go2f: ctrl_dt, action_scale, noise level, scales joint_pos / joint_vel / gyro / gravity / linvel, init_from_crouch,
// energy_termination_threshold, z_des, desired forward vector.  env_go2i: joint ids of the pose cost.  env_go2_home: home | pre_recovery
// qpos.  env_go2_soft: soft lower | upper limits.  info block: step at 0, last_act at 4..15, rng at G2_RNG.
enum { HS_STEP = 0, HS_LAST_ACT = 4, HS_PRIV = 94 };
enum { HM_HEIGHT = 0, HM_ORIENT, HM_CONTACT, HM_ACTION_RATE, HM_TERM, HM_DOF_LIMITS, HM_TORQUES, HM_POSE, HM_STAY_STILL, HM_ENERGY, HM_DOF_ACC, HM_COUNT };

// handstand.py:196-245: the 45-dim "state" into obs_lds; five splits of info.rng, draws in the reference's order (gyro, gravity, joint
// angles, joint velocities, linvel)
template <class C>
__device__ __forceinline__ void hs_obs(const DModel& m, Smem<C>& s, const G2Sens& sn, float* obs_lds, uint32_t* bits, int lane) {
#pragma clang fp contract(off)
  const float* F = m.env_go2f;
  uint32_t rng0 = __float_as_uint(s.ginfo[G2_RNG]), rng1 = __float_as_uint(s.ginfo[G2_RNG + 1]);
  rng0 = (uint32_t)uniform_i((int)rng0); rng1 = (uint32_t)uniform_i((int)rng1);
  const float level = F[2];
  const float home_l = m.env_go2_home[7 + (lane < 12 ? lane : 0)];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    uint32_t k2[2][2];
    tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
    const int n = (d == 2 || d == 3) ? 12 : 3;
    const float u = tf_uniform(k2[1][0], k2[1][1], n, 0.0f, 1.0f, bits, lane);
    if (lane < n) {
      float src, scale; int dst;
      if (d == 0) { src = pick3(sn.gyro, lane); scale = F[5]; dst = 3 + lane; }
      else if (d == 1) { src = pick3(sn.gravity, lane); scale = F[6]; dst = 6 + lane; }
      else if (d == 2) { src = s.qpos[7 + lane]; scale = F[3]; dst = 9 + lane; }
      else if (d == 3) { src = s.qvel[6 + lane]; scale = F[4]; dst = 21 + lane; }
      else { src = pick3(sn.linvel, lane); scale = F[7]; dst = lane; }
      float a = 2.0f * u; float b = a - 1.0f; float c = b * level; float e = c * scale;
      float val = src + e;
      if (d == 2) val = val - home_l;
      obs_lds[dst] = val;
    }
  }
  if (lane < 12) obs_lds[33 + lane] = s.ginfo[HS_LAST_ACT + lane];
  if (lane == 0) { s.ginfo[G2_RNG] = __uint_as_float(rng0); s.ginfo[G2_RNG + 1] = __uint_as_float(rng1); }
  WSYNC();
}

// handstand.py:246-259: element t of obs["privileged_state"] (94)
template <class C>
__device__ __forceinline__ float hs_priv_elem(const DModel& m, const Smem<C>& s, const G2Sens& sn, const float* obs_lds, int t) {
  if (t < 45) return obs_lds[t];
  t -= 45;
  if (t < 3) return pick3(sn.gyro, t);
  if (t < 6) return pick3(sn.accel, t - 3);
  if (t < 9) return pick3(sn.linvel, t - 6);
  if (t < 12) return pick3(sn.gang, t - 9);
  if (t < 24) return s.qpos[7 + t - 12];
  if (t < 36) return s.qvel[6 + t - 24];
  if (t < 48) return s.aforce[t - 36];
  if (t == 48) return s.spos[3 * m.env_ids[0] + 2];
  return 0.0f;
}

// handstand.py:119-160 + wrappers
template <class C>
__global__ __launch_bounds__(64) void hs_reset_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  float* rec = a.state + (size_t)e * L.rec;
  const float* F = m.env_go2f;
  uint32_t* bits = reinterpret_cast<uint32_t*>(s.scratch_b());
  float* obs_lds = s.scratch_b() + 64;
  load_overrides<C>(m, s, a, e, lane);
  for (int t = lane; t < C::NINFO; t += 64) s.ginfo[t] = 0.0f;
  uint32_t rng0 = a.keys[2 * e], rng1 = a.keys[2 * e + 1];
  uint32_t k2[2][2];
  tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
  const float ub = rdlane(tf_uniform(k2[1][0], k2[1][1], 1, 0.0f, 1.0f, bits, lane), 0);
  const bool crouch = ub < F[8];                                       // jax.random.bernoulli(key, p)
  const float q_init = m.env_go2_home[(crouch ? C::NQ : 0) + (lane < C::NQ ? lane : 0)];
  if (lane < C::NQ) s.qpos[lane] = q_init;
  if (lane < C::NV) s.qvel[lane] = 0.0f;
  WSYNC();
  {
    tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
    float dxy = tf_uniform(k2[1][0], k2[1][1], 2, -0.5f, 0.5f, bits, lane);
    if (lane < 2) s.qpos[lane] = q_init + dxy;
    tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
    float yaw = rdlane(tf_uniform(k2[1][0], k2[1][1], 1, -3.14f, 3.14f, bits, lane), 0);
    WSYNC();
    if (lane == 0) {
#pragma clang fp contract(off)
      float sn = sinf(yaw * 0.5f), cs = cosf(yaw * 0.5f);
      Q4 q = ld4(&s.qpos[3]), r = Q4{cs, 0.0f * sn, 0.0f * sn, 1.0f * sn};
      Q4 o;
      o.w = q.w * r.w - q.x * r.x - q.y * r.y - q.z * r.z;
      o.x = q.w * r.x + q.x * r.w + q.y * r.z - q.z * r.y;
      o.y = q.w * r.y - q.x * r.z + q.y * r.w + q.z * r.x;
      o.z = q.w * r.z + q.x * r.y - q.y * r.x + q.z * r.w;
      st4(&s.qpos[3], o);
    }
    tf_split<2>(rng0, rng1, bits, lane, k2); rng0 = k2[0][0]; rng1 = k2[0][1];
    float v6 = tf_uniform(k2[1][0], k2[1][1], 6, -0.5f, 0.5f, bits, lane);
    if (lane < 6 && !crouch) s.qvel[lane] = v6;
  }
  WSYNC();
  if (lane < C::NU) s.ctrl[lane] = s.qpos[7 + lane];          // mjx_env.init(..., ctrl = qpos[7:])
  if (lane == 0) {
    s.xfrc_body = 0; s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f;
    s.ginfo[G2_RNG] = __uint_as_float(rng0); s.ginfo[G2_RNG + 1] = __uint_as_float(rng1);
  }
  WSYNC();
  float Mrow[C::NV], warm = 0.0f;
  FwdOut<C> f;
  PROF_DECL
  forward<C>(m, hot, s, lane, Mrow, warm, f, a.debug ? a.debug + (size_t)e * RSR_DEBUG_FLOATS : nullptr PROF_PASS);
  WSYNC();
  G2Sens sn;
  go2_sensors<C>(m, s, sn);
  go2_accelerometer<C>(m, s, lane, f.qacc, sn);
  hs_obs<C>(m, s, sn, obs_lds, bits, lane);
  for (int t = lane; t < GO2_PRIV; t += 64) { float v = hs_priv_elem<C>(m, s, sn, obs_lds, t); rec[L.priv_obs + t] = v; rec[L.f_priv_obs + t] = v; }
  store_pipeline<C>(s, rec, L, lane, warm, 0.0f);
  for (int t = lane; t < C::NINFO; t += 64) rec[L.go2_info + t] = s.ginfo[t];
  for (int t = lane; t < C::OBS; t += 64) { rec[L.obs + t] = obs_lds[t]; rec[L.f_obs + t] = obs_lds[t]; }
  if (lane == 0) {
    store_reset_outputs<C>(s, f, rec, L);
    rec[L.f_time] = 0.0f;
  }
  store_first_state<C>(s, rec, L, lane, warm, false);
}

// handstand.py:161-195 with the rewards :264-342, + wrappers
template <class C>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RSR_HS_WAVES_PER_EU, RSR_HS_WAVES_PER_EU)))
void hs_step_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  float* rec = a.state + (size_t)e * L.rec;
  const bool wrap_episode = m.wrap_flags & 1, wrap_autoreset = (m.wrap_flags & 2) != 0;
  const float* F = m.env_go2f;
  const float dt = F[0];
  uint32_t* bits = reinterpret_cast<uint32_t*>(s.scratch_b());
  float* obs_lds = s.scratch_b() + 64;
  float* rwl = s.scratch_b() + 128;                                   // scaled reward terms staged for the metrics write
  float* qacc_lds = s.scratch_b() + 160;                              // qacc of the last forward pass, for the dof_acc term
  PROF_DECL
  float warm = 0.0f, time;
  load_pipeline<C>(s, rec, L, lane, warm, time);
  load_overrides<C>(m, s, a, e, lane);
  for (int t = lane; t < C::NINFO; t += 64) s.ginfo[t] = rec[L.go2_info + t];
  const float done_prev = rec[L.done];
  float steps = rec[L.steps];
  if (wrap_autoreset && done_prev != 0.0f) steps = 0.0f;
  const float act_in = lane < C::NU ? a.action[(size_t)e * C::NU + lane] : 0.0f;
  if (lane < C::NU) {
#pragma clang fp contract(off)
    float sc = act_in * F[1];
    s.ctrl[lane] = rec[L.ctrl + lane] + sc;                          // motor targets = state.data.ctrl + action * action_scale (:162)
  }
  if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  WSYNC();
  PROF(PS_LOAD)
  float Mrow[C::NV];
  FwdOut<C> f;
  const int prio_q = prio_quarter(a, e);
  for (int fr = 0; fr < m.n_frames; ++fr) {
#if defined(RSR_PROFILE) || defined(RSR_TIMELINE)
    float* dbg = nullptr;
#else
    float* dbg = (a.debug && fr == m.n_frames - 1) ? a.debug + (size_t)e * RSR_DEBUG_FLOATS : nullptr;
#endif
    const int lane_s = lrec_lane(lane);
    prio_substep(a.prio_mode, prio_q, fr);
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, dbg PROF_PASS);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    time += hot.timestep;
  }
  // which pairs the termination / contact cost look at (pairs are static): 1 = an unwanted-contact geom, 2 = a foot of the contact cost
  int pair_class = 0;
  if (lane < C::NP) {
    const int g2 = m.pair_geom2[lane];
#pragma unroll
    for (int k = 0; k < 12; ++k) if (g2 == m.env_ids[2 + k]) pair_class = 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) if (g2 == m.env_ids[14 + k]) pair_class = 2;
  }
  const float prev_done = wrap_episode ? rec[L.episode_done] : 0.0f;
  const float em_old = (wrap_episode && lane < C::NMET + 2) ? rec[L.episode_metrics + lane] : 0.0f;
  G2Sens sn;
  go2_sensors<C>(m, s, sn);
  go2_accelerometer<C>(m, s, lane, f.qacc, sn);
  // every pair is asked, before collision() caps the list the physics sees at NCON points (collision.geoms_colliding)
  const bool touch = lane < C::NP && ((f.touching >> lane) & 1ull) != 0ull;
  const bool unwanted = __ballot(touch && pair_class == 1) != 0ull, feet = __ballot(touch && pair_class == 2) != 0ull;
  if (lane < C::NV) qacc_lds[lane] = f.qacc;
  WSYNC();
  hs_obs<C>(m, s, sn, obs_lds, bits, lane);
  float priv[2];
  priv[0] = hs_priv_elem<C>(m, s, sn, obs_lds, lane);
  priv[1] = hs_priv_elem<C>(m, s, sn, obs_lds, lane + 64 < GO2_PRIV ? lane + 64 : GO2_PRIV - 1);
  float reward = 0.0f, done = 0.0f;
  if (lane == 0) {
#pragma clang fp contract(off)
    const float* SC = m.env_go2_scales; const float* home = m.env_go2_home; const float* soft = m.env_go2_soft;
    const int imu = m.env_ids[0];
    const float torso_height = s.spos[3 * imu + 2];
    float energy = 0.0f;
    for (int i = 0; i < 12; ++i) energy += fabsf(s.aforce[i]) * fabsf(s.qvel[6 + i]);
    done = (sn.up[2] < -0.25f || unwanted || energy > F[9]) ? 1.0f : 0.0f;
    float rw[HM_COUNT];
    {
      float h = torso_height < F[10] ? torso_height : F[10];
      float err = F[10] - h;
      rw[HM_HEIGHT] = expf(-err / 1.0f);
      const float* R = &s.smat[9 * imu];
      float c0 = R[0] * F[11]; float c1 = R[3] * F[12]; float c2 = R[6] * F[13];
      float cd = c0 + c1; float cos_dist = cd + c2;
      float nrm = 0.5f * cos_dist; float nr = nrm + 0.5f;
      rw[HM_ORIENT] = nr * nr;
      rw[HM_CONTACT] = feet ? 1.0f : 0.0f;
      float ar = 0.0f, tq = 0.0f, lim = 0.0f, dacc = 0.0f, pose = 0.0f, en = 0.0f;
      for (int i = 0; i < 12; ++i) {
        float da = a.action[(size_t)e * C::NU + i] - s.ginfo[HS_LAST_ACT + i]; ar += da * da;
        float t = s.aforce[i]; tq += t * t;
        float q = s.qpos[7 + i];
        float lo_ = q - soft[i]; float hi_ = q - soft[12 + i];
        lim += -(lo_ < 0.0f ? lo_ : 0.0f) + (hi_ > 0.0f ? hi_ : 0.0f);
        float qa = qacc_lds[6 + i]; dacc += qa * qa;
        en += fabsf(s.qvel[6 + i]) * fabsf(t);
      }
      for (int k = 0; k < 6; ++k) { const int j = m.env_go2i[k]; float dq = s.qpos[7 + j] - home[7 + j]; pose += dq * dq; }
      rw[HM_ACTION_RATE] = ar; rw[HM_TORQUES] = tq; rw[HM_TERM] = done; rw[HM_DOF_LIMITS] = lim; rw[HM_DOF_ACC] = dacc; rw[HM_POSE] = pose;
      float ss = s.qvel[0] * s.qvel[0] + s.qvel[1] * s.qvel[1];
      rw[HM_STAY_STILL] = ss + s.qvel[5] * s.qvel[5];
      rw[HM_ENERGY] = en;
    }
    for (int k = 0; k < HM_COUNT; ++k) rwl[k] = rw[k] * SC[k];
    const int order[HM_COUNT] = {HM_HEIGHT, HM_ORIENT, HM_CONTACT, HM_ACTION_RATE, HM_TORQUES, HM_TERM, HM_DOF_LIMITS, HM_DOF_ACC, HM_POSE,
                                 HM_STAY_STILL, HM_ENERGY};
    float total = 0.0f;
    for (int k = 0; k < HM_COUNT; ++k) total = total + rwl[order[k]];
    reward = clampf(total * dt, 0.0f, 10000.0f);
  }
  reward = rdlane(reward, 0); done = rdlane(done, 0);
  WSYNC();
  if (lane < C::NU) s.ginfo[HS_LAST_ACT + lane] = act_in;
  if (lane == 0) s.ginfo[HS_STEP] += 1.0f;
  WSYNC();
  {
    bool over = false;
    float trunc = 0.0f;
    if (wrap_episode) {
      steps += 1.0f;
      over = steps >= (float)m.episode_length;
      trunc = over ? 1.0f - done : 0.0f;
    }
    if (lane < C::NMET) rec[L.metrics + lane] = rwl[lane];
    if (wrap_episode && lane < C::NMET + 2) {
      float* em = rec + L.episode_metrics;
      const float add = lane == 0 ? reward : (lane == 1 ? 1.0f : rwl[lane >= 2 ? lane - 2 : 0]);
      em[lane] = prev_done != 0.0f ? 0.0f : em_old + add;
    }
    if (over) done = 1.0f;
    if (lane == 0) {
      rec[L.reward] = reward;
      if (wrap_episode) { rec[L.truncation] = trunc; rec[L.episode_done] = done; }
      rec[L.steps] = steps;
      rec[L.done] = done;
      int* st = reinterpret_cast<int*>(rec + L.stats);
      st[0] = f.st.niter; st[1] = f.st.ls_total; st[2] = s.ncon; st[3] = s.ncon_drop;
    }
  }
  WSYNC();
  for (int t = lane; t < C::NINFO; t += 64) rec[L.go2_info + t] = s.ginfo[t];       // info is never reset by AutoReset
  if (wrap_autoreset && done != 0.0f) {
    for (int t = lane; t < L.persist_end; t += 64) rec[t] = rec[L.f_qpos + t];
    for (int t = lane; t < C::OBS; t += 64) rec[L.obs + t] = rec[L.f_obs + t];
    for (int t = lane; t < GO2_PRIV; t += 64) rec[L.priv_obs + t] = rec[L.f_priv_obs + t];
  } else {
    store_pipeline<C>(s, rec, L, lane, warm, time);
    for (int t = lane; t < C::OBS; t += 64) rec[L.obs + t] = obs_lds[t];
    rec[L.priv_obs + lane] = priv[0];
    if (lane + 64 < GO2_PRIV) rec[L.priv_obs + lane + 64] = priv[1];
  }
#ifdef RSR_PROFILE
  PROF(PS_EPILOGUE)
  if (a.debug && lane == 0) {
    float* d = a.debug + (size_t)e * RSR_DEBUG_FLOATS + 7200;
    for (int i = 0; i < PS_COUNT; ++i) d[i] = (float)prof_.acc[i];
  }
#endif
}

}  // namespace rsr
