// rsr_physics.hip -- the library's translation units: the env kernels and C ABI of ../rsr_mjx.hip, plus the physics-level API
// (include/rsr_physics.h: rsr_physics_step / rsr_physics_forward / rsr_physics_rollout / rsr_physics_view, the sensor stage of
// rsr_sensors.hpp).  rsr_mjx_amd/build.py compiles this file
// once per unit, with the macros of rsr_mjx.hip (RSR_TU_TSHAPE: the T-shape kernels; RSR_TU_GO2: the Go2 family; neither: the cube
// kernels and the host code); each unit adds its family's physics kernels to the env kernels it already holds.
// The env sources are included unchanged: their hash (bench.py csrc_sha16) pins the parity envelopes measured on them, and the
// env kernels' device code is the same with or without what follows.
#include "../rsr_mjx.hip"
#include "../../../include/rsr_physics.h"
#include "rsr_sensors.hpp"

namespace rsr {

// ================================================================ physics-only kernels (rsr_physics_step / rsr_physics_forward)
// mjx_env.step(model, data, ctrl, n_substeps) and mjx_env.init's mjx.forward (reference _src/mjx_env.py:30-73) on the record's
// pipeline state: no env prologue / epilogue, no wrappers, no PRNG.  The per-env model leaves of the batch apply.  One wave per env,
// a plain launch.  Each family's physics kernels are built in the unit of its env kernels (same flags, same inlined stages): the
// substeps compile to the same arithmetic as inside rsr_step, and a physics step is bit-identical to the env step it stands in for
// (tests/test_physics_gpu.py).
//
// Side buffer (rsr_physics_view), per env, floats: qacc [nv] | actuator_force [nu] | xquat [nbody*4] | ncon | contacts [ncon_max][9]
// (dist, pos[3], normal[3], geom1, geom2) | ncon_dropped, padded to 16 floats.  Filled by these kernels only (rsr_step leaves it).
struct PhysLayout { int qacc, aforce, xquat, ncon, con, ncon_drop, stride; };
__host__ __device__ inline PhysLayout phys_layout(int nv, int nu, int nbody, int ncon_max) {
  PhysLayout p;
  p.qacc = 0; p.aforce = nv; p.xquat = nv + nu; p.ncon = p.xquat + 4 * nbody; p.con = p.ncon + 1; p.ncon_drop = p.con + 9 * ncon_max;
  p.stride = (p.ncon_drop + 1 + 15) & ~15;
  return p;
}
struct PhysArgs {
  const float* ctrl;    // [N][nu] or null (keep the record's ctrl)
  float* out;           // side buffer [N][PhysLayout::stride] or null
  const int* ids;       // [grid] the envs to run (rsr_physics_forward_envs), or null: env = workgroup index
  int nsteps;           // substeps (the step kernel)
  float* sd;            // sensordata [N][RSR_MAX_SENSORDATA], written when sens.nsd > 0
  SensArgs sens;
};
// rsr_physics_rollout: ctrl [N][T][nu]; trajectory rows [N][T][w], each pointer null = not recorded
struct RollArgs {
  const float* ctrl;
  int T;
  float *qpos, *qvel, *time, *aforce, *ncon, *sd;
};

// the side buffer row of env e from the last forward pass (qacc_i: this lane's qacc of that pass)
template <class C>
__device__ __forceinline__ void store_side(const DModel& m, const Smem<C>& s, float* out, int e, int lane, float qacc_i) {
  const PhysLayout PL = phys_layout(C::NV, C::NU, C::NB, C::NCON);
  float* o = out + (size_t)e * PL.stride;
  if (lane < C::NV) o[PL.qacc + lane] = qacc_i;
  if (lane < C::NU) o[PL.aforce + lane] = s.aforce[lane];
  for (int t = lane; t < C::NB * 4; t += 64) o[PL.xquat + t] = s.xquat[t];
  const int nc = s.ncon;
  for (int c = lane; c < C::NCON; c += 64) {
    float* w = o + PL.con + 9 * c;
    const bool on = c < nc;
    const int pr = on ? s.cpair[c] : 0;
    w[0] = on ? s.cdist[c] : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { w[1 + k] = on ? s.cpos[3 * c + k] : 0.0f; w[4 + k] = on ? s.cnrm[3 * c + k] : 0.0f; }
    w[7] = on ? (float)m.pair_geom1[pr] : -1.0f; w[8] = on ? (float)m.pair_geom2[pr] : -1.0f;
  }
  if (lane == 0) { o[PL.ncon] = (float)nc; o[PL.ncon_drop] = (float)s.ncon_drop; }
}

// STEP: nsteps x (forward, integrate); otherwise one forward.  Position-dependent outputs (xpos, xquat, site_xpos, contacts) are
// those of the last forward pass, i.e. before the final integration (MJX Data semantics, as in the record after rsr_step).
template <class C, bool STEP, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void physics_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = p.ids ? p.ids[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  if (e < 0 || e >= a.n) return;                                // (an id out of range runs nothing)
  float* rec = a.state + (size_t)e * L.rec;
  PROF_DECL
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float warm = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  float time = rec[L.time];
  load_overrides<C>(m, s, a, e, lane);
  if (lane < C::NU) s.ctrl[lane] = p.ctrl ? p.ctrl[(size_t)e * C::NU + lane] : rec[L.ctrl + lane];
  if constexpr (C::XFRC) {        // data.xfrc_applied = 0 (the Go2 joystick's kick is env logic); the accelerometer's body as in the env kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  WSYNC();
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsteps = STEP ? p.nsteps : 1;
  for (int fr = 0; fr < nsteps; ++fr) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS);
    if constexpr (STEP) {
      integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
      time += hot.timestep;
    }
  }
  WSYNC();
  if (p.sens.nsd > 0) {                                          // (wave-uniform; no table: the stage is skipped)
    const float v = sensor_stage<C>(m, s, lane, f.qacc, p.sens);
    if (lane < p.sens.nsd) p.sd[(size_t)e * RSR_MAX_SENSORDATA + lane] = v;
  }
  if constexpr (STEP) store_pipeline<C>(s, rec, L, lane, warm, time);
  else {                          // mjx.forward leaves qpos as it was (kinematics normalises the quaternions in LDS only)
    if (lane < C::NV) rec[L.warm + lane] = warm;
    for (int t = lane; t < C::NB * 3; t += 64) rec[L.xpos + t] = s.xpos[t];
    for (int t = lane; t < C::NS * 3; t += 64) rec[L.site_xpos + t] = s.spos[t];
  }
  if (p.out) store_side<C>(m, s, p.out, e, lane, f.qacc);
}

// rsr_physics_rollout: T control steps of physics_kernel<C, true> in one launch.  The state stays in LDS and the warm start in its
// register from one control step to the next (in physics_kernel both make a round trip through the record, which is exact), so
// the trajectory is bit-identical to T step launches.  After control step t the wave writes its rows t of the requested
// trajectories: per env the rows are contiguous in time ([N][T][w]).  The record, the side buffer and the sensordata row are
// written once, at the end, as physics_kernel<C, true> writes them.
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void rollout_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, RollArgs r) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = (int)blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  float* rec = a.state + (size_t)e * L.rec;
  PROF_DECL
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float warm = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  float time = rec[L.time];
  load_overrides<C>(m, s, a, e, lane);
  if constexpr (C::XFRC) {
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  float Mrow[C::NV];
  FwdOut<C> f;
  const int nsd = p.sens.nsd;
  // one loop over the T * nsteps substeps, as in physics_kernel, the control-step boundary a wave-uniform branch (a loop over
  // control steps around the substep loop spills 19 VGPRs of the Go2 kernels at their 128-register budget, this 13: DESIGN.md 4c)
  if (lane < C::NU) s.ctrl[lane] = r.ctrl[(size_t)e * r.T * C::NU + lane];
  WSYNC();
  const int total = r.T * p.nsteps;
  int t = 0, fr = 0;
  for (int k = 0; k < total; ++k) {
    const int lane_s = lrec_lane(lane);        // see step_kernel
    forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS);
    integrate<C>(m, hot, s, lane_s, Mrow, f PROF_PASS);
    time += hot.timestep;
    if (++fr < p.nsteps) continue;
    fr = 0;
    WSYNC();
    const size_t row = (size_t)e * r.T + t;
    float sv = 0.0f;
    if (nsd > 0) {
      sv = sensor_stage<C>(m, s, lane, f.qacc, p.sens);
      if (t == r.T - 1 && lane < nsd) p.sd[(size_t)e * RSR_MAX_SENSORDATA + lane] = sv;      // the view: the last control step's
    }
    if (r.qpos) for (int q = lane; q < C::NQ; q += 64) r.qpos[row * C::NQ + q] = s.qpos[q];
    if (r.qvel && lane < C::NV) r.qvel[row * C::NV + lane] = s.qvel[lane];
    if (r.time && lane == 0) r.time[row] = time;
    if (r.aforce && lane < C::NU) r.aforce[row * C::NU + lane] = s.aforce[lane];
    if (r.ncon && lane == 0) r.ncon[row] = (float)s.ncon;
    if (r.sd && lane < nsd) r.sd[row * nsd + lane] = sv;
    if (++t < r.T) {
      if (lane < C::NU) s.ctrl[lane] = r.ctrl[(row + 1) * C::NU + lane];
      WSYNC();
    }
  }
  store_pipeline<C>(s, rec, L, lane, warm, time);
  if (p.out) store_side<C>(m, s, p.out, e, lane, f.qacc);
}

// launchers, one per unit (the family's env kernels live there too); Go2 kind: 2 joystick on a plane, 3 joystick on a height field,
// 4 handstand / footstand.  mode: PHYS_FORWARD, PHYS_STEP, PHYS_ROLLOUT (r is read by the last only).
enum { PHYS_FORWARD = 0, PHYS_STEP = 1, PHYS_ROLLOUT = 2 };
void launch_physics_cube(int mode, int n, hipStream_t st, const DModel* dm, Layout L, StepArgs a, PhysArgs p, RollArgs r);
void launch_physics_tshape(int mode, int n, hipStream_t st, const DModel* dm, Layout L, StepArgs a, PhysArgs p, RollArgs r);
void launch_physics_go2(int kind, int mode, int n, hipStream_t st, const DModel* dm, Layout L, StepArgs a, PhysArgs p, RollArgs r);
template <class C, int WAVES>
static void launch_phys(int mode, int n, hipStream_t st, const DModel* dm, Layout L, StepArgs a, PhysArgs p, RollArgs r) {
  if (mode == PHYS_STEP) hipLaunchKernelGGL((physics_kernel<C, true, WAVES>), dim3(n), dim3(64), sizeof(Smem<C>), st, dm, L, a, p);
  else if (mode == PHYS_FORWARD) hipLaunchKernelGGL((physics_kernel<C, false, WAVES>), dim3(n), dim3(64), sizeof(Smem<C>), st, dm, L, a, p);
  else hipLaunchKernelGGL((rollout_kernel<C, WAVES>), dim3(n), dim3(64), sizeof(Smem<C>), st, dm, L, a, p, r);
}
#if defined(RSR_TU_TSHAPE)
void launch_physics_tshape(int mode, int n, hipStream_t st, const DModel* dm, Layout L, StepArgs a, PhysArgs p, RollArgs r) {
  launch_phys<TShapeDims, RSR_WAVES_PER_EU>(mode, n, st, dm, L, a, p, r);
}
#elif defined(RSR_TU_GO2)
void launch_physics_go2(int kind, int mode, int n, hipStream_t st, const DModel* dm, Layout L, StepArgs a, PhysArgs p, RollArgs r) {
  if (kind == 4) launch_phys<HandDims, RSR_HS_WAVES_PER_EU>(mode, n, st, dm, L, a, p, r);
  else if (kind == 3) launch_phys<Go2Dims, RSR_GO2_WAVES_PER_EU>(mode, n, st, dm, L, a, p, r);
  else launch_phys<Go2FlatDims, RSR_GO2_WAVES_PER_EU>(mode, n, st, dm, L, a, p, r);
}
#else
void launch_physics_cube(int mode, int n, hipStream_t st, const DModel* dm, Layout L, StepArgs a, PhysArgs p, RollArgs r) {
  launch_phys<CubeDims, RSR_WAVES_PER_EU>(mode, n, st, dm, L, a, p, r);
}
#endif

}  // namespace rsr

#if !defined(RSR_TU_GO2) && !defined(RSR_TU_TSHAPE)
// ---------------------------------------------------------------- host side: the physics handle
// The side buffer belongs to a handle of its own (the batch struct is part of the env sources, see the top of this file).
struct rsr_physics {
  rsr_batch* b;         // borrowed
  float* out;           // [n][PhysLayout::stride]
  rsr::PhysLayout PL;
  float* sd;            // sensordata [n][RSR_MAX_SENSORDATA]
  int4* sens_el;        // [RSR_MAX_SENSORDATA] the sensor table, one entry per output element (rsr::SensArgs)
  int nsd = 0, acc_site = -1;
};

extern "C" int rsr_physics_create(rsr_batch* b, rsr_physics** out) {
  if (!b || !out) return fail(RSR_ERR_ARG, "rsr_physics_create: null argument");
  const int kind = b->model->dims.env_kind;
  if (kind != rsr::ENV_CUBE && kind != rsr::ENV_AIRBOT_SF && kind != rsr::ENV_TSHAPE && kind != rsr::ENV_GO2 && kind != rsr::ENV_GO2_HANDSTAND)
    return fail(RSR_ERR_UNSUPPORTED, "rsr_physics_create: no physics kernel for this env kind");
  HIPCHK(hipSetDevice(b->device));
  const rsr_dims& d = b->model->dims;
  rsr_physics* p = new rsr_physics();
  p->b = b;
  p->PL = rsr::phys_layout(d.nv, d.nu, d.nbody, d.ncon_max);
  const size_t bytes = (size_t)b->n * p->PL.stride * sizeof(float);
  if (hipMalloc(&p->out, bytes) != hipSuccess) { delete p; return fail(RSR_ERR_NOMEM, "rsr_physics_create: hipMalloc(side buffer)"); }
  if (hipMemset(p->out, 0, bytes) != hipSuccess) { (void)hipFree(p->out); delete p; return fail(RSR_ERR_HIP, "rsr_physics_create: hipMemset"); }
  const size_t sd_bytes = (size_t)b->n * RSR_MAX_SENSORDATA * sizeof(float);
  if (hipMalloc(&p->sd, sd_bytes) != hipSuccess) { (void)hipFree(p->out); delete p; return fail(RSR_ERR_NOMEM, "rsr_physics_create: hipMalloc(sensordata)"); }
  if (hipMalloc(&p->sens_el, RSR_MAX_SENSORDATA * sizeof(int4)) != hipSuccess) {
    (void)hipFree(p->sd); (void)hipFree(p->out); delete p; return fail(RSR_ERR_NOMEM, "rsr_physics_create: hipMalloc(sensor table)");
  }
  if (hipMemset(p->sd, 0, sd_bytes) != hipSuccess) {
    (void)hipFree(p->sens_el); (void)hipFree(p->sd); (void)hipFree(p->out); delete p; return fail(RSR_ERR_HIP, "rsr_physics_create: hipMemset");
  }
  *out = p;
  return RSR_OK;
}

extern "C" void rsr_physics_destroy(rsr_physics* p) {
  if (!p) return;
  (void)hipSetDevice(p->b->device);
  if (p->out) (void)hipFree(p->out);
  if (p->sd) (void)hipFree(p->sd);
  if (p->sens_el) (void)hipFree(p->sens_el);
  delete p;
}

static int physics_launch(rsr_physics* ph, const float* ctrl, const int* ids, int grid, int nsteps, int mode, void* hip_stream, const char* who,
                          const rsr::RollArgs& r = rsr::RollArgs{}) {
  rsr_batch* b = ph->b;
  HIPCHK(hipSetDevice(b->device));
  rsr::StepArgs a = make_args(b);
  a.debug = nullptr;
  const rsr::PhysArgs p{ctrl, ph->out, ids, nsteps, ph->sd, rsr::SensArgs{ph->sens_el, ph->nsd, ph->acc_site}};
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const Layout& LY = b->model->layout;
  switch (b->model->dims.env_kind) {
    case rsr::ENV_GO2: rsr::launch_physics_go2(b->model->has_hfield ? 3 : 2, mode, grid, st, b->dmodel, LY, a, p, r); break;
    case rsr::ENV_GO2_HANDSTAND: rsr::launch_physics_go2(4, mode, grid, st, b->dmodel, LY, a, p, r); break;
    case rsr::ENV_TSHAPE: rsr::launch_physics_tshape(mode, grid, st, b->dmodel, LY, a, p, r); break;
    default: rsr::launch_physics_cube(mode, grid, st, b->dmodel, LY, a, p, r); break;
  }
  { hipError_t le = hipGetLastError(); if (le != hipSuccess) return fail(RSR_ERR_HIP, std::string(who) + ": launch: " + hipGetErrorString(le)); }
  return RSR_OK;
}

extern "C" int rsr_physics_step(rsr_physics* p, const float* ctrl, int nsteps, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_step: null handle");
  if (nsteps < 1) return fail(RSR_ERR_ARG, "rsr_physics_step: nsteps must be >= 1");
  const int rc = physics_launch(p, ctrl, nullptr, p->b->n, nsteps, rsr::PHYS_STEP, hip_stream, "rsr_physics_step");
  if (rc == RSR_OK && p->b->timing) p->b->launches++;
  return rc;
}

extern "C" int rsr_physics_forward(rsr_physics* p, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_forward: null handle");
  return physics_launch(p, nullptr, nullptr, p->b->n, 1, rsr::PHYS_FORWARD, hip_stream, "rsr_physics_forward");
}

extern "C" int rsr_physics_forward_envs(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream) {
  if (!p || !env_ids || count < 1) return fail(RSR_ERR_ARG, "rsr_physics_forward_envs: null handle / ids or count < 1");
  return physics_launch(p, nullptr, env_ids, count, 1, rsr::PHYS_FORWARD, hip_stream, "rsr_physics_forward_envs");
}

extern "C" int rsr_physics_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  if (!p || !dev_ptr || !shape || !stride) return fail(RSR_ERR_ARG, "rsr_physics_view: null argument");
  const rsr_dims& d = p->b->model->dims;
  const rsr::PhysLayout& PL = p->PL;
  int off = -1, w = 0;
  switch (field) {
    case RSR_P_QACC: off = PL.qacc; w = d.nv; break;
    case RSR_P_ACTUATOR_FORCE: off = PL.aforce; w = d.nu; break;
    case RSR_P_XQUAT: off = PL.xquat; w = 4 * d.nbody; break;
    case RSR_P_NCON: off = PL.ncon; w = 1; break;
    case RSR_P_CONTACT: off = PL.con; w = 9 * d.ncon_max; break;
    case RSR_P_NCON_DROPPED: off = PL.ncon_drop; w = 1; break;
    case RSR_P_SENSORDATA:
      *dev_ptr = p->sd;
      shape[0] = p->b->n; shape[1] = p->nsd;
      stride[0] = RSR_MAX_SENSORDATA; stride[1] = 1;
      return RSR_OK;
    default: return fail(RSR_ERR_ARG, "rsr_physics_view: unknown field id");
  }
  *dev_ptr = p->out + off;
  shape[0] = p->b->n; shape[1] = w;
  stride[0] = PL.stride; stride[1] = 1;
  return RSR_OK;
}

extern "C" int rsr_physics_set_sensors(rsr_physics* p, const int32_t* table, int nsensor) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_set_sensors: null handle");
  if (nsensor < 0 || nsensor > RSR_MAX_SENSORDATA || (nsensor > 0 && !table))
    return fail(RSR_ERR_ARG, "rsr_physics_set_sensors: nsensor must lie in [0, 64] and the table must not be null");
  static const int width[RSR_S_COUNT] = {3, 3, 3, 3, 3, 3, 4, 3, 3};
  const rsr_model* md = p->b->model;
  const int nsite = md->dims.nsite, kind = md->dims.env_kind;
  const int32_t* site_body = static_cast<const int32_t*>(md->find("site_bodyid"));
  const int32_t* env_ids = static_cast<const int32_t*>(md->find("env_ids"));
  std::vector<int4> el;
  int acc_site = -1;
  for (int i = 0; i < nsensor; ++i) {
    const int32_t type = table[4 * i], site = table[4 * i + 1], ref = table[4 * i + 2], adr = table[4 * i + 3];
    const std::string at = "rsr_physics_set_sensors: sensor " + std::to_string(i) + ": ";
    if (type < 0 || type >= RSR_S_COUNT) return fail(RSR_ERR_ARG, at + "unknown type");
    if (site < 0 || site >= nsite) return fail(RSR_ERR_ARG, at + "site id out of range");
    if (ref != -1 && (type != RSR_S_FRAMEPOS || ref < 0 || ref >= nsite)) return fail(RSR_ERR_ARG, at + "bad ref site (framepos only)");
    if (adr != (int)el.size()) return fail(RSR_ERR_ARG, at + "address must follow the previous sensor");
    if ((int)el.size() + width[type] > RSR_MAX_SENSORDATA) return fail(RSR_ERR_ARG, at + "more than 64 sensordata floats");
    if (type == RSR_S_ACCELEROMETER) {
      // the kernels track the acceleration bias of one body: the Go2 IMU site's (env_ids[0])
      const bool go2 = kind == rsr::ENV_GO2 || kind == rsr::ENV_GO2_HANDSTAND;
      if (!go2 || !site_body || !env_ids || site_body[site] != site_body[env_ids[0]])
        return fail(RSR_ERR_UNSUPPORTED, at + "accelerometer only on a site of the Go2 IMU's body");
      if (acc_site >= 0 && acc_site != site) return fail(RSR_ERR_UNSUPPORTED, at + "accelerometers on more than one site");
      acc_site = site;
    }
    for (int c = 0; c < width[type]; ++c) el.push_back(int4{type, site, ref, c});
  }
  HIPCHK(hipSetDevice(p->b->device));
  if (!el.empty()) {
    HIPCHK(hipDeviceSynchronize());               // launches in flight read the table
    HIPCHK(hipMemcpy(p->sens_el, el.data(), el.size() * sizeof(int4), hipMemcpyHostToDevice));
  }
  p->nsd = (int)el.size();
  p->acc_site = acc_site;
  return RSR_OK;
}

extern "C" int rsr_physics_rollout(rsr_physics* p, const float* ctrl, int T, int nsteps, const rsr_rollout_out* out, void* hip_stream) {
  if (!p || !ctrl) return fail(RSR_ERR_ARG, "rsr_physics_rollout: null handle or ctrl");
  if (T < 1 || nsteps < 1 || (int64_t)T * nsteps > INT32_MAX) return fail(RSR_ERR_ARG, "rsr_physics_rollout: T and nsteps must be >= 1 (T * nsteps < 2^31)");
  rsr::RollArgs r{ctrl, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (out) {
    if (out->sensordata && p->nsd == 0) return fail(RSR_ERR_ARG, "rsr_physics_rollout: sensordata requested with no sensor table set");
    r.qpos = out->qpos; r.qvel = out->qvel; r.time = out->time; r.aforce = out->actuator_force; r.ncon = out->ncon; r.sd = out->sensordata;
  }
  const int rc = physics_launch(p, nullptr, nullptr, p->b->n, nsteps, rsr::PHYS_ROLLOUT, hip_stream, "rsr_physics_rollout", r);
  if (rc == RSR_OK && p->b->timing) p->b->launches++;
  return rc;
}
#endif  // the host unit
