// rsr_env.hpp -- what every env unit shares: the model families' Dims, the env_ids and info-block layouts, the jax PRNG, and the
// record I/O of the kernels (per-env model leaves, pipeline state, first state, reset outputs, wrapper bookkeeping).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rsr_mjx.h"
#include "rsr_solver.hpp"

namespace rsr {

// Airbot cube: nq 22, nv 20, nu 5, nbody 14, njnt 10, ngeom 23, nsite 1, npair 45, neq 1, nf 8, nl 8
#ifndef RSR_CUBE_NCON
#define RSR_CUBE_NCON 24
#endif
using CubeDims = Dims<22, 20, 5, 14, 10, 23, 1, 45, 1, 8, 8, /*NCON*/ RSR_CUBE_NCON, /*OBS*/ 23, /*NMET*/ 3, 0, 0, 4, 0,
                      /*ISO: the target body's free joint, dofs 8..13*/ 8, 14, false, false, false, /*NGA*/ 23, false, false,
                      /*TREE1, TREE2: arm | target | cube*/ 8, 14>;
// Airbot T-shape: nq 15, nv 14, njnt 9, ngeom 25, nsite 3, npair 60; 4 env geoms at env_ids[5..8]
// Unitree Go2 feet-only: nq 19, nv 18, nu 12, 13 joints, 39 geoms, 6 sites, 4 sphere-plane pairs of condim 3
using Go2Dims = Dims<19, 18, 12, 14, 13, 39, 6, 4, /*NEQ*/ 0, /*NF*/ 12, /*NL*/ 12, /*NCON*/ 4, /*OBS*/ 48, /*NMET*/ 22, 0, 0, /*CONDIM*/ 3,
                     /*NINFO*/ 144, /*ISO*/ 0, 0, /*DREX*/ true, /*HFIELD*/ true, /*TALIAS*/ false, /*NGA: floor or height field + four feet*/ 5, /*TTAIL*/ true, /*ARROW*/ true>;
// the same without the height-field narrow phase, for models whose floor is a plane (the flat-terrain joystick): the kernel is picked
// by the model (rsr_model_create: any PAIR_HFIELD_SPHERE pair)
using Go2FlatDims = Dims<19, 18, 12, 14, 13, 39, 6, 4, /*NEQ*/ 0, /*NF*/ 12, /*NL*/ 12, /*NCON*/ 4, /*OBS*/ 48, /*NMET*/ 22, 0, 0, /*CONDIM*/ 3,
                     /*NINFO*/ 144, /*ISO*/ 0, 0, /*DREX*/ true, /*HFIELD*/ false, /*TALIAS*/ false, /*NGA: floor or height field + four feet*/ 5, /*TTAIL*/ true, /*ARROW*/ true>;
// Unitree Go2 with every collision geom against the floor (go2_mjx.xml + scene_mjx_flat_terrain.xml, the Handstand / Footstand tasks): 44 geoms,
// 30 plane pairs of condim 3 (4 spheres, 20 capsules, 6 cylinders: up to 62 contact points, 12 kept active per env -- a state with
// more is a fall, which ends the episode in the same step)
using HandDims = Dims<19, 18, 12, 14, 13, 44, 6, 30, /*NEQ*/ 0, /*NF*/ 12, /*NL*/ 12, /*NCON*/ 12, /*OBS*/ 45, /*NMET*/ 11, 0, 0, /*CONDIM*/ 3,
                      /*NINFO*/ 144, /*ISO*/ 0, 0, /*DREX*/ true, /*HFIELD*/ false, /*TALIAS*/ false, /*NGA*/ 44, /*TTAIL*/ true, /*ARROW*/ true, 0, 0, /*CAPS*/ true>;
using TShapeDims = Dims<15, 14, 5, 14, 9, 25, 3, 60, 1, 8, 8, /*NCON*/ 32, /*OBS*/ 16, /*NMET*/ 5, /*NEG*/ 4, /*EG0*/ 5, /*CONDIM*/ 4, 0, 0, 0, false, false, false,
                        /*NGA*/ 25, false, false, /*TREE1, TREE2: arm | T block*/ 8, 14>;

// env_ids layout (rsr_mjx_amd/envs/config.py)
enum { ID_CUBE = 0, ID_TARGET = 1, ID_SITE = 2, ID_BOXQ = 3, ID_SITEQ = 4, ID_FINGERQ = 5, ID_JOINTQ = 6 };

// register budgets of the step kernels (waves per SIMD); overridable per build (-D...)
#ifndef RSR_WAVES_PER_EU
#define RSR_WAVES_PER_EU 2           // Airbot step kernels
#endif
#ifndef RSR_GO2_WAVES_PER_EU
#define RSR_GO2_WAVES_PER_EU 4       // Go2 joystick
#endif
#ifndef RSR_HS_WAVES_PER_EU
#define RSR_HS_WAVES_PER_EU 3        // Go2 handstand / footstand
#endif
#ifndef RSR_DEFAULT_UNITS
#define RSR_DEFAULT_UNITS 4          // phases per env-step of the work-queue dispatch (measured: DESIGN.md 4)
#endif

// ---------------------------------------------------------------- threefry2x32 (jax.random default PRNG)
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t& o0, uint32_t& o1) {
  const int R[8] = {13, 15, 26, 6, 17, 29, 16, 24};
  uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  uint32_t x0 = c0 + ks[0], x1 = c1 + ks[1];
#pragma unroll
  for (int g = 0; g < 5; ++g) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { x0 += x1; x1 = rotl32(x1, R[(g & 1) * 4 + k]); x1 ^= x0; }
    x0 += ks[(g + 1) % 3];
    x1 += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
  o0 = x0; o1 = x1;
}
// bits[0..n) = threefry_2x32(key, iota(n)) in jax's split-halves layout; lane-parallel, result in LDS
__device__ void random_bits(uint32_t k0, uint32_t k1, int n, uint32_t* bits, int lane) {
  int half = (n + 1) / 2;
  if (lane < half) {
    uint32_t c1 = (half + lane < n) ? (uint32_t)(half + lane) : 0u, o0, o1;
    threefry2x32(k0, k1, (uint32_t)lane, c1, o0, o1);
    bits[lane] = o0;
    if (half + lane < n) bits[half + lane] = o1;
  }
}
__device__ __forceinline__ float uniform_from_bits(uint32_t b, float lo, float hi) {
#pragma clang fp contract(off)   // jax does a separate multiply and add (HIP's __fmul_rn is a plain '*')
  float u = __uint_as_float((b >> 9) | 0x3F800000u) - 1.0f;
  float scale = hi - lo;
  float prod = u * scale;
  float v = prod + lo;
  return fmaxf(lo, v);
}
// jax.random.split(key, N): every lane receives all N keys (wave-uniform); bits = LDS scratch of >= 2N words
template <int N>
__device__ __forceinline__ void tf_split(uint32_t k0, uint32_t k1, uint32_t* bits, int lane, uint32_t (&out)[N][2]) {
  WSYNC();
  random_bits(k0, k1, 2 * N, bits, lane);
  WSYNC();
#pragma unroll
  for (int r = 0; r < N; ++r) { out[r][0] = bits[2 * r]; out[r][1] = bits[2 * r + 1]; }
}
// jax.random.uniform(key, (n,), lo, hi): lane i < n returns element i
__device__ __forceinline__ float tf_uniform(uint32_t k0, uint32_t k1, int n, float lo, float hi, uint32_t* bits, int lane) {
  WSYNC();
  random_bits(k0, k1, n, bits, lane);
  WSYNC();
  return lane < n ? uniform_from_bits(bits[lane], lo, hi) : 0.0f;
}
// jax.random.split(key, N) in registers: the 2N output words are threefry(key, (j, N + j)) of lanes j < N -- word t is the first
// output of lane t for t < N and the second output of lane t - N otherwise -- fetched with v_readlane: no LDS, no barrier.
template <int N>
__device__ __forceinline__ void tf_split_reg(uint32_t k0, uint32_t k1, int lane, uint32_t (&out)[N][2]) {
  uint32_t o0, o1;
  threefry2x32(k0, k1, (uint32_t)lane, (uint32_t)(N + lane), o0, o1);
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int t = 2 * r + w;
      out[r][w] = (uint32_t)(t < N ? rdlane_i((int)o0, t) : rdlane_i((int)o1, t - N));
    }
}
// One lane's share of a batch of jax.random.uniform draws evaluated together: this lane is word pair `idx` of a draw of n
// elements with key (k0, k1), whose bits go to bits[off .. off + n) (same split-halves layout as random_bits).
__device__ __forceinline__ void tf_bits_batched(uint32_t k0, uint32_t k1, int n, int idx, int off, bool on, uint32_t* bits) {
  const int half = (n + 1) / 2;
  const bool two = half + idx < n;
  uint32_t o0, o1;
  threefry2x32(k0, k1, (uint32_t)idx, two ? (uint32_t)(half + idx) : 0u, o0, o1);
  if (on) { bits[off + idx] = o0; if (two) bits[off + half + idx] = o1; }
}

// Go2 info block (Layout::go2_info)
// ginfo layout = oracle enum G2_* ; env_go2f / env_go2i / env_ids as documented in rsr_mjx_amd/envs/config.py
enum { G2_CMD = 0, G2_STEPS_CMD = 3, G2_LAST_ACT = 4, G2_LAST_LAST_ACT = 16, G2_AIR = 28, G2_CONTACT_T = 32, G2_LAST_CONTACT = 36,
       G2_SWING = 40, G2_ACT_BUF = 44, G2_GYRO_BUF = 92, G2_LINVEL_BUF = 104, G2_GRAV_BUF = 116, G2_STEPS_PERT = 128,
       G2_PERT_DUR_S = 129, G2_PERT_DUR = 130, G2_SINCE_PERT = 131, G2_PERT_STEPS = 132, G2_PERT_DIR = 133, G2_PERT_MAG = 136,
       G2_RNG = 137, G2_XFRC = 139 /* data.xfrc_applied[torso, :3] */ };
constexpr int GO2_PRIV = 123;    // obs['privileged_state'], joystick.py:341-366

// ---------------------------------------------------------------- record I/O
template <class C>
__device__ void load_overrides(const DModel& m, Smem<C>& s, const StepArgs& a, int e, int lane) {
  if (lane < 4) s.rw[C::NEFC + lane] = 0.0f;                 // zero weight of the null row
  // Per-env leaf or the model's own: the source POINTER is selected, then every value is read in one batch of global loads and
  // stored to LDS after one wait.  (A branch per leaf -- `dr ? dr[..] : m.x[..]` -- made each leaf's load wait on its own: up
  // to nine global round trips in a row at the start of every work unit.)
  auto src = [&](const float* dr, gp_f own, int per_env) { return dr ? (gp_f)(dr + (size_t)e * per_env) : own; };
  const gp_f p_fric = src(a.dr_geom_friction, m.geom_friction, C::NG * 3), p_mass = src(a.dr_body_mass, m.body_mass, C::NB);
  const gp_f p_damp = src(a.dr_dof_damping, m.dof_damping, C::NV), p_floss = src(a.dr_dof_frictionloss, m.dof_frictionloss, C::NV);
  constexpr int NFR = (C::NGA * 3 + 63) / 64;
  float v_fric[NFR];
#pragma unroll
  for (int k = 0; k < NFR; ++k) {                             // friction of the geom slots (geoms of the contact pairs)
    const int t = lane + 64 * k, tt = t < C::NGA * 3 ? t : 0;
    const int sidx = C::NGA == C::NG ? tt : 3 * m.geom_slot_ids[tt / 3] + tt % 3;
    v_fric[k] = p_fric[sidx];
  }
  const float v_mass = p_mass[lane < C::NB ? lane : 0];
  const int dl = lane < C::NV ? lane : 0;
  const float v_damp = p_damp[dl], v_floss = p_floss[dl];
  float v_ipos[2] = {0, 0}, v_q0 = 0, v_arma = 0, v_gain = 0, v_bias = 0;
  if constexpr (C::DREX) {
    static_assert(C::NB * 3 <= 64 && C::NQ <= 64 && C::NU * 3 <= 64, "one lane per extended leaf entry");
    const gp_f p_ipos = src(a.dr_body_ipos, m.body_ipos, C::NB * 3), p_q0 = src(a.dr_qpos0, m.qpos0, C::NQ);
    const gp_f p_arma = src(a.dr_dof_armature, m.dof_armature, C::NV);
    const gp_f p_gain = src(a.dr_gainprm, m.actuator_gainprm, C::NU * 3), p_bias = src(a.dr_biasprm, m.actuator_biasprm, C::NU * 3);
    v_ipos[0] = p_ipos[lane < C::NB * 3 ? lane : 0]; v_q0 = p_q0[lane < C::NQ ? lane : 0]; v_arma = p_arma[dl];
    v_gain = p_gain[lane < C::NU * 3 ? lane : 0]; v_bias = p_bias[lane < C::NU * 3 ? lane : 0];
  }
#pragma unroll
  for (int k = 0; k < NFR; ++k) { const int t = lane + 64 * k; if (t < C::NGA * 3) s.fric[t] = v_fric[k]; }
  if (lane < C::NB) s.mass[lane] = v_mass;
  if (lane < C::NV) { s.damp[lane] = v_damp; s.floss[lane] = v_floss; }
  if constexpr (C::DREX) {
    if (lane < C::NB * 3) s.dx_ipos[lane] = v_ipos[0];
    if (lane < C::NQ) s.dx_qpos0[lane] = v_q0;
    if (lane < C::NV) s.dx_arma[lane] = v_arma;
    if (lane < C::NU * 3) { s.dx_gain[lane] = v_gain; s.dx_bias[lane] = v_bias; }
  }
}

// the pipeline state of the record: qpos, qvel, the solver's warm start (this lane's dof) and time
template <class C>
__device__ __forceinline__ void load_pipeline(Smem<C>& s, const float* rec, const Layout& L, int lane, float& warm, float& time) {
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  time = rec[L.time];
}

template <class C>
__device__ void store_pipeline(Smem<C>& s, float* rec, const Layout& L, int lane, float warm, float time) {
  for (int t = lane; t < C::NQ; t += 64) rec[L.qpos + t] = s.qpos[t];
  if (lane < C::NV) { rec[L.qvel + lane] = s.qvel[lane]; rec[L.warm + lane] = warm; }
  if (lane < C::NU) rec[L.ctrl + lane] = s.ctrl[lane];
  if (lane == 0) rec[L.time] = time;
  for (int t = lane; t < C::NB * 3; t += 64) rec[L.xpos + t] = s.xpos[t];
  for (int t = lane; t < C::NS * 3; t += 64) rec[L.site_xpos + t] = s.spos[t];
}

// AutoResetWrapper.reset: cache first_pipeline_state (same field order as the live block).  f_time is the caller's: the Go2 resets
// store it with the lane-0 outputs.
template <class C>
__device__ __forceinline__ void store_first_state(const Smem<C>& s, float* rec, const Layout& L, int lane, float warm, bool f_time) {
  for (int t = lane; t < C::NQ; t += 64) rec[L.f_qpos + t] = s.qpos[t];
  if (lane < C::NV) { rec[L.f_qvel + lane] = s.qvel[lane]; rec[L.f_warm + lane] = warm; }
  if (lane < C::NU) rec[L.f_ctrl + lane] = s.ctrl[lane];
  if (f_time && lane == 0) rec[L.f_time] = 0.0f;
  for (int t = lane; t < C::NB * 3; t += 64) rec[L.f_xpos + t] = s.xpos[t];
  for (int t = lane; t < C::NS * 3; t += 64) rec[L.f_site_xpos + t] = s.spos[t];
}

// lane 0 of a reset: reward, done, metrics and the wrappers' counters and sums start at zero; stats of the reset's forward pass
template <class C>
__device__ __forceinline__ void store_reset_outputs(const Smem<C>& s, const FwdOut<C>& f, float* rec, const Layout& L) {
  rec[L.reward] = 0.0f; rec[L.done] = 0.0f;
  for (int i = 0; i < C::NMET; ++i) rec[L.metrics + i] = 0.0f;
  rec[L.steps] = 0.0f; rec[L.truncation] = 0.0f; rec[L.episode_done] = 0.0f;
  for (int i = 0; i < 2 + C::NMET; ++i) rec[L.episode_metrics + i] = 0.0f;
  int* st = reinterpret_cast<int*>(rec + L.stats);
  st[0] = f.st.niter; st[1] = f.st.ls_total; st[2] = s.ncon; st[3] = s.ncon_drop;
}

}  // namespace rsr
