// rsr_physics.hip -- the C ABI of the physics layer (include/rsr_physics.h): rsr_physics_step / rsr_physics_forward /
// rsr_physics_rollout / rsr_physics_view, the sensor table of rsr_sensors.hpp, the applied forces (rsr_physics_set_applied) and
// the dynamics terms (rsr_physics_dynamics), the constraint and contact forces (rsr_physics_constraint) and the transition Jacobians
// (rsr_physics_transition_fd), inverse dynamics (rsr_physics_inverse), sampled rollouts (rsr_physics_sample_rollouts), parameter
// rollouts (rsr_physics_param_rollouts), closed-loop rollouts (rsr_physics_feedback_rollouts), cost rollouts (rsr_physics_cost_rollouts), the transition Jacobians along a
// trajectory (rsr_physics_trajectory_fd), the LQR backward pass (rsr_physics_lqr_backward) and its control-limited form (rsr_physics_lqr_box), inverse kinematics on site pose
// targets (rsr_physics_ik), the Kalman filter and smoother (rsr_physics_kalman) and the cost expansion (rsr_physics_cost_expand).  Every launch is a physics op
// (rsr::PhysOp) sent through physics_launch; the kernels are in the family units (physics/rsr_physics_kernels.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../rsr_host.hpp"
#include "../rsr_launch.hpp"

// The side buffer belongs to a handle of its own, on a batch it borrows.
struct rsr_physics {
  rsr_batch* b;         // borrowed
  float* out = nullptr;  // [n][PhysLayout::stride]
  rsr::PhysLayout PL;
  float* sd = nullptr;   // sensordata [n][RSR_MAX_SENSORDATA]
  int4* sens_el = nullptr;  // [RSR_MAX_SENSORDATA] the sensor table, one entry per output element (rsr::SensArgs)
  int nsd = 0, acc_site = -1;
  float* xfrc = nullptr;  // data.xfrc_applied [n][nbody*6], allocated on the first rsr_physics_set_applied(p, 1)
  float* qfrc = nullptr;  // data.qfrc_applied [n][nv]
  bool applied = false;   // launches take the applied kernels
  float* dyn = nullptr;   // the dynamics buffer [n][DynLayout::stride], allocated on first use (dyn_buffers)
  int* jac_sites = nullptr;  // [RSR_MAX_JAC_SITES] the Jacobian sites (device)
  int njac = 0;
  float* con = nullptr;   // the constraint buffer [n][ConLayout::stride], allocated on first use (con_buffer)
  float* fd = nullptr;    // the transition buffer [n][FdLayout::env], allocated on first use (fd_buffers)
  float* fd_states = nullptr;  // the states buffer of RSR_FD_STATES, allocated on first request (fd_buffers)
  float* inv = nullptr;   // the inverse buffer [n][InvLayout::stride], allocated on first use (inv_buffer)
  float* nominal = nullptr;  // the nominal scratch of rsr_physics_trajectory_fd [M][T][nq + 2 nv], grown on demand (nominal_scratch)
  size_t nominal_floats = 0;
};

// `*slot`, a buffer of the handle, on first use: `bytes` of device memory, zeroed; once there it never moves.  A failure is reported
// as `who`'s, with the buffer's name `what`, and leaves the slot null.
template <class T>
static int zeroed_once(rsr_physics* p, T** slot, size_t bytes, const char* what, const char* who) {
  if (*slot) return RSR_OK;
  HIPCHK(hipSetDevice(p->b->device));
  T* buf = nullptr;
  if (hipMalloc(&buf, bytes) != hipSuccess) return fail(RSR_ERR_NOMEM, std::string(who) + ": hipMalloc(" + what + ")");
  if (hipMemset(buf, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(buf); return fail(RSR_ERR_HIP, std::string(who) + ": hipMemset");
  }
  *slot = buf;
  return RSR_OK;
}

extern "C" int rsr_physics_create(rsr_batch* b, rsr_physics** out) {
  if (!b || !out) return fail(RSR_ERR_ARG, "rsr_physics_create: null argument");
  HIPCHK(hipSetDevice(b->device));
  const rsr_dims& d = b->model->dims;
  rsr_physics* p = new rsr_physics();
  p->b = b;
  p->PL = rsr::phys_layout(d.nv, d.nu, d.nbody, d.ncon_max);
  const char* who = "rsr_physics_create";
  int rc = zeroed_once(p, &p->out, (size_t)b->n * p->PL.stride * sizeof(float), "side buffer", who);
  if (!rc) rc = zeroed_once(p, &p->sd, (size_t)b->n * RSR_MAX_SENSORDATA * sizeof(float), "sensordata", who);
  if (!rc) rc = zeroed_once(p, &p->sens_el, RSR_MAX_SENSORDATA * sizeof(int4), "sensor table", who);
  if (rc) { rsr_physics_destroy(p); return rc; }
  *out = p;
  return RSR_OK;
}

extern "C" void rsr_physics_destroy(rsr_physics* p) {
  if (!p) return;
  (void)hipSetDevice(p->b->device);
  if (p->out) (void)hipFree(p->out);
  if (p->sd) (void)hipFree(p->sd);
  if (p->sens_el) (void)hipFree(p->sens_el);
  if (p->xfrc) (void)hipFree(p->xfrc);
  if (p->qfrc) (void)hipFree(p->qfrc);
  if (p->dyn) (void)hipFree(p->dyn);
  if (p->jac_sites) (void)hipFree(p->jac_sites);
  if (p->con) (void)hipFree(p->con);
  if (p->fd) (void)hipFree(p->fd);
  if (p->fd_states) (void)hipFree(p->fd_states);
  if (p->inv) (void)hipFree(p->inv);
  if (p->nominal) (void)hipFree(p->nominal);
  delete p;
}

// The arguments of a physics op on `grid` envs (ids: which, or null: the first `grid`): the handle's buffers as every op's; the
// caller adds what its op owns (r, fd, inv, K, sw).
static rsr::Launch physics_args(rsr_physics* ph, const float* ctrl, const int* ids, int grid, int nsteps, void* hip_stream) {
  rsr::Launch x = launch_args(ph->b, hip_stream);
  x.grid = grid;
  x.a.debug = nullptr;
  x.ph.p = rsr::PhysArgs{ctrl, ph->out, ids, nsteps, ph->sd, rsr::SensArgs{ph->sens_el, ph->nsd, ph->acc_site}};
  x.ph.d = rsr::DynArgs{ph->dyn, ids, ph->jac_sites, ph->njac};
  x.ph.c = rsr::ConArgs{ph->con, ids};
  if (ph->applied) x.ph.ap = rsr::Applied{ph->xfrc, ph->qfrc};
  return x;
}

// sends one physics op (rsr::PhysOp); reports the launch error as `who`
static int physics_launch(rsr_physics* ph, int op, const rsr::Launch& x, const char* who) {
  HIPCHK(hipSetDevice(ph->b->device));
  if (launch(ph->b, op, x) < 0) return fail(RSR_ERR_UNSUPPORTED, std::string(who) + ": the model's kernels have no such op");
  { hipError_t le = hipGetLastError(); if (le != hipSuccess) return fail(RSR_ERR_HIP, std::string(who) + ": launch: " + hipGetErrorString(le)); }
  return RSR_OK;
}

// a launch that advances the state, for the batch's timing: counted when it was sent
static int counted(rsr_physics* p, int rc) {
  if (rc == RSR_OK && p->b->timing) p->b->launches++;
  return rc;
}

// the envs an env-list entry point runs, *n: the `count` listed ones, or with env_ids null every env of the batch
static int env_count(const rsr_physics* p, const int32_t* env_ids, int count, const char* who, int* n) {
  if (env_ids && count < 1) return fail(RSR_ERR_ARG, std::string(who) + ": count < 1 with env_ids");
  *n = env_ids ? count : p->b->n;
  return RSR_OK;
}

extern "C" int rsr_physics_step(rsr_physics* p, const float* ctrl, int nsteps, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_step: null handle");
  if (nsteps < 1) return fail(RSR_ERR_ARG, "rsr_physics_step: nsteps must be >= 1");
  return counted(p, physics_launch(p, rsr::OP_PHYS_STEP, physics_args(p, ctrl, nullptr, p->b->n, nsteps, hip_stream), "rsr_physics_step"));
}

extern "C" int rsr_physics_forward(rsr_physics* p, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_forward: null handle");
  return physics_launch(p, rsr::OP_PHYS_FORWARD, physics_args(p, nullptr, nullptr, p->b->n, 1, hip_stream), "rsr_physics_forward");
}

extern "C" int rsr_physics_forward_envs(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream) {
  if (!p || !env_ids || count < 1) return fail(RSR_ERR_ARG, "rsr_physics_forward_envs: null handle / ids or count < 1");
  return physics_launch(p, rsr::OP_PHYS_FORWARD, physics_args(p, nullptr, env_ids, count, 1, hip_stream), "rsr_physics_forward_envs");
}

// a view's answer: `w` floats per env from `ptr`, the envs `row` floats apart
static int view_out(const rsr_physics* p, float* ptr, int w, int row, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  *dev_ptr = ptr;
  shape[0] = p->b->n; shape[1] = w;
  stride[0] = row; stride[1] = 1;
  return RSR_OK;
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
    case RSR_P_SENSORDATA: return view_out(p, p->sd, p->nsd, RSR_MAX_SENSORDATA, dev_ptr, shape, stride);
    default: return fail(RSR_ERR_ARG, "rsr_physics_view: unknown field id");
  }
  return view_out(p, p->out + off, w, PL.stride, dev_ptr, shape, stride);
}

extern "C" int rsr_physics_set_sensors(rsr_physics* p, const int32_t* table, int nsensor) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_set_sensors: null handle");
  if (nsensor < 0 || nsensor > RSR_MAX_SENSORDATA || (nsensor > 0 && !table))
    return fail(RSR_ERR_ARG, "rsr_physics_set_sensors: nsensor must lie in [0, 64] and the table must not be null");
  static const int width[RSR_S_COUNT] = {3, 3, 3, 3, 3, 3, 4, 3, 3};
  const rsr_model* md = p->b->model;
  const int nsite = md->dims.nsite;
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
      if (md->spec->family != rsr::FAMILY_GO2 || !site_body || !env_ids || site_body[site] != site_body[env_ids[0]])
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
  rsr::Launch x = physics_args(p, nullptr, nullptr, p->b->n, nsteps, hip_stream);
  rsr::RollArgs& r = x.ph.r = rsr::RollArgs{ctrl, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (out) {
    if (out->sensordata && p->nsd == 0) return fail(RSR_ERR_ARG, "rsr_physics_rollout: sensordata requested with no sensor table set");
    r.qpos = out->qpos; r.qvel = out->qvel; r.time = out->time; r.aforce = out->actuator_force; r.ncon = out->ncon; r.sd = out->sensordata;
  }
  return counted(p, physics_launch(p, rsr::OP_PHYS_ROLLOUT, x, "rsr_physics_rollout"));
}

// The refusals the three (slot, sample) rollouts share, after each entry's own argument checks and in `who`'s name; *waves: the
// launch's workgroups.  Only reads.
static int sample_grid(const rsr_physics* p, const int32_t* env_ids, int count, int K, int T, int nsteps, const rsr_rollout_out* out,
                       const char* who, int* waves) {
  int n;
  if (const int rc = env_count(p, env_ids, count, who, &n)) return rc;
  if (out->sensordata && p->nsd == 0) return fail(RSR_ERR_ARG, std::string(who) + ": sensordata requested with no sensor table set");
  const int64_t grid = (int64_t)n * K;           // one wave per (slot, sample)
  if (grid > INT32_MAX || (int64_t)T * nsteps > INT32_MAX)
    return fail(RSR_ERR_ARG, std::string(who) + ": envs x K and T x nsteps must stay below 2^31");
  *waves = (int)grid;
  return RSR_OK;
}

extern "C" int rsr_physics_sample_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, int K, int T, int nsteps,
                                           const rsr_rollout_out* out, void* hip_stream) {
  const char* who = "rsr_physics_sample_rollouts";
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_sample_rollouts: null handle");
  if (!ctrl) return fail(RSR_ERR_ARG, "rsr_physics_sample_rollouts: null ctrl");
  if (!out || !(out->qpos || out->qvel || out->time || out->actuator_force || out->ncon || out->sensordata))
    return fail(RSR_ERR_ARG, "rsr_physics_sample_rollouts: null out, or nothing to record");
  if (K < 1 || T < 1 || nsteps < 1) return fail(RSR_ERR_ARG, "rsr_physics_sample_rollouts: K, T and nsteps must be >= 1");
  int grid;
  if (const int rc = sample_grid(p, env_ids, count, K, T, nsteps, out, who, &grid)) return rc;
  rsr::Launch x = physics_args(p, nullptr, env_ids, grid, nsteps, hip_stream);
  x.ph.r = rsr::RollArgs{ctrl, T, out->qpos, out->qvel, out->time, out->actuator_force, out->ncon, out->sensordata};
  x.ph.K = K;
  return counted(p, physics_launch(p, rsr::OP_PHYS_SAMPLE, x, who));
}

// The tail of the two sweep entries (parameter and closed-loop rollouts), after each entry's own argument checks: sample_grid's
// refusals and the leaves', then the one launch of sw.K samples per listed env.  The entry has filled what it owns of `sw` (K, the
// flags, the feedback rows); `params` null: no leaf is sampled.
static int sweep_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, const rsr_param_samples* params,
                          rsr::SweepArgs sw, int T, int nsteps, const rsr_rollout_out* out, void* hip_stream, const char* who) {
  int grid;
  if (const int rc = sample_grid(p, env_ids, count, sw.K, T, nsteps, out, who, &grid)) return rc;
  for (int f = 0; params && f < RSR_DR_COUNT; ++f) {
    if (params->leaf[f] && f >= RSR_DR_BODY_IPOS && p->b->model->spec->family != rsr::FAMILY_GO2)
      return fail(RSR_ERR_UNSUPPORTED, std::string(who) + ": this leaf is per-env only in the Go2 kernels (rsr_batch_set_dr_field); the Airbot kernels take the first four");
    sw.leaf[f] = params->leaf[f];
  }
  rsr::Launch x = physics_args(p, nullptr, env_ids, grid, nsteps, hip_stream);
  x.ph.r = rsr::RollArgs{ctrl, T, out->qpos, out->qvel, out->time, out->actuator_force, out->ncon, out->sensordata};
  x.ph.sw = sw;
  return counted(p, physics_launch(p, rsr::OP_PHYS_SWEEP, x, who));
}

extern "C" int rsr_physics_param_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, const rsr_param_samples* params,
                                          int K, int T, int nsteps, int flags, const rsr_rollout_out* out, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_param_rollouts: null handle");
  if (!ctrl) return fail(RSR_ERR_ARG, "rsr_physics_param_rollouts: null ctrl");
  if (!out || !(out->qpos || out->qvel || out->time || out->actuator_force || out->ncon || out->sensordata))
    return fail(RSR_ERR_ARG, "rsr_physics_param_rollouts: null out, or nothing to record");
  if (K < 1 || T < 1 || nsteps < 1) return fail(RSR_ERR_ARG, "rsr_physics_param_rollouts: K, T and nsteps must be >= 1");
  if (flags & ~RSR_PR_CTRL_PER_SAMPLE) return fail(RSR_ERR_ARG, "rsr_physics_param_rollouts: unknown flag bits");
  rsr::SweepArgs sw{};
  sw.K = K;
  sw.ctrl_per_sample = (flags & RSR_PR_CTRL_PER_SAMPLE) != 0;
  return sweep_rollouts(p, env_ids, count, ctrl, params, sw, T, nsteps, out, hip_stream, "rsr_physics_param_rollouts");
}

// Closed-loop rollouts: the parameter rollout's launch with the feedback rows set (rsr_feedback.hpp).
extern "C" int rsr_physics_feedback_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, const rsr_feedback* fb,
                                             const rsr_param_samples* params, int K, int T, int nsteps, int flags, const rsr_rollout_out* out,
                                             float* ctrl_out, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_feedback_rollouts: null handle");
  if (!ctrl) return fail(RSR_ERR_ARG, "rsr_physics_feedback_rollouts: null ctrl");
  if (!fb || !fb->gain || !fb->qpos_ref || !fb->qvel_ref) return fail(RSR_ERR_ARG, "rsr_physics_feedback_rollouts: null fb, or a null member of it");
  if (!out) return fail(RSR_ERR_ARG, "rsr_physics_feedback_rollouts: null out");
  if (!ctrl_out && !(out->qpos || out->qvel || out->time || out->actuator_force || out->ncon || out->sensordata))
    return fail(RSR_ERR_ARG, "rsr_physics_feedback_rollouts: nothing to record and null ctrl_out");
  if (K < 1 || T < 1 || nsteps < 1) return fail(RSR_ERR_ARG, "rsr_physics_feedback_rollouts: K, T and nsteps must be >= 1");
  if (flags & ~(RSR_FB_CTRL_PER_SAMPLE | RSR_FB_PER_SAMPLE | RSR_FB_CLAMP)) return fail(RSR_ERR_ARG, "rsr_physics_feedback_rollouts: unknown flag bits");
  rsr::SweepArgs sw{};
  sw.K = K;
  sw.ctrl_per_sample = (flags & RSR_FB_CTRL_PER_SAMPLE) != 0;
  sw.fb_gain = fb->gain; sw.fb_qpos = fb->qpos_ref; sw.fb_qvel = fb->qvel_ref;
  sw.ctrl_out = ctrl_out;
  sw.fb_per_sample = (flags & RSR_FB_PER_SAMPLE) != 0;
  sw.fb_clamp = (flags & RSR_FB_CLAMP) != 0;
  return sweep_rollouts(p, env_ids, count, ctrl, params, sw, T, nsteps, out, hip_stream, "rsr_physics_feedback_rollouts");
}

// Cost rollouts: the sweep's launch shape with the cost stage (rsr_cost.hpp), an op of its own.  Its own checks, sample_grid's,
// the leaves' as sweep_rollouts makes them, then the one launch; nothing is allocated and no buffer of the handle is used.
extern "C" int rsr_physics_cost_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, const rsr_feedback* fb,
                                         const rsr_param_samples* params, const rsr_cost* cost, int K, int T, int nsteps, int flags,
                                         const rsr_rollout_out* traj, const rsr_cost_out* out, void* hip_stream) {
  const char* who = "rsr_physics_cost_rollouts";
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: null handle");
  if (!ctrl) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: null ctrl");
  if (fb && (!fb->gain || !fb->qpos_ref || !fb->qvel_ref)) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: an fb with a null member");
  if (!fb && (flags & (RSR_FB_PER_SAMPLE | RSR_FB_CLAMP))) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: RSR_FB_PER_SAMPLE or RSR_FB_CLAMP with a null fb");
  if (!cost || !out || !out->cost) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: null cost, out or out->cost");
  if (!(cost->w_qpos || cost->w_qvel || cost->w_ctrl || cost->w_sensor)) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: all four weights are null");
  if (cost->w_qpos && !cost->qpos_ref) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: w_qpos without qpos_ref");
  if (out->dx && !cost->qpos_ref) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: out->dx without qpos_ref");
  if (K < 1 || T < 1 || nsteps < 1) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: K, T and nsteps must be >= 1");
  if (flags & ~(RSR_FB_CTRL_PER_SAMPLE | RSR_FB_PER_SAMPLE | RSR_FB_CLAMP)) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: unknown flag bits");
  if ((cost->w_sensor || cost->sensor_ref) && p->nsd == 0) return fail(RSR_ERR_ARG, "rsr_physics_cost_rollouts: w_sensor or sensor_ref with no sensor table set");
  const rsr_rollout_out none{};
  const rsr_rollout_out* tr = traj ? traj : &none;
  int grid;
  if (const int rc = sample_grid(p, env_ids, count, K, T, nsteps, tr, who, &grid)) return rc;
  rsr::SweepArgs sw{};
  for (int f = 0; params && f < RSR_DR_COUNT; ++f) {
    if (params->leaf[f] && f >= RSR_DR_BODY_IPOS && p->b->model->spec->family != rsr::FAMILY_GO2)
      return fail(RSR_ERR_UNSUPPORTED, std::string(who) + ": this leaf is per-env only in the Go2 kernels (rsr_batch_set_dr_field); the Airbot kernels take the first four");
    sw.leaf[f] = params->leaf[f];
  }
  sw.K = K;
  sw.ctrl_per_sample = (flags & RSR_FB_CTRL_PER_SAMPLE) != 0;
  if (fb) { sw.fb_gain = fb->gain; sw.fb_qpos = fb->qpos_ref; sw.fb_qvel = fb->qvel_ref; }
  sw.fb_per_sample = (flags & RSR_FB_PER_SAMPLE) != 0;
  sw.fb_clamp = (flags & RSR_FB_CLAMP) != 0;
  rsr::Launch x = physics_args(p, nullptr, env_ids, grid, nsteps, hip_stream);
  x.ph.r = rsr::RollArgs{ctrl, T, tr->qpos, tr->qvel, tr->time, tr->actuator_force, tr->ncon, tr->sensordata};
  x.ph.sw = sw;                                  // (sw.ctrl_out stays null: the cost stage writes out->ctrl)
  x.ph.cs = rsr::CostArgs{cost->qpos_ref, cost->qvel_ref, cost->ctrl_ref, cost->sensor_ref, cost->w_qpos, cost->w_qvel, cost->w_ctrl, cost->w_sensor,
                          out->cost, out->step_cost, out->terms, out->dx, out->ctrl};
  return counted(p, physics_launch(p, rsr::OP_COST_ROLLOUTS, x, who));
}

// the applied-force buffers, on first use: both or neither
static int applied_buffers(rsr_physics* p, size_t xb, size_t qb, const char* who) {
  const bool had = p->xfrc != nullptr;
  if (const int rc = zeroed_once(p, &p->xfrc, xb, "xfrc", who)) return rc;
  const int rc = zeroed_once(p, &p->qfrc, qb, "qfrc", who);
  if (rc && !had) { (void)hipFree(p->xfrc); p->xfrc = nullptr; }
  return rc;
}

extern "C" int rsr_physics_set_applied(rsr_physics* p, int on) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_set_applied: null handle");
  if (on != 0 && on != 1) return fail(RSR_ERR_ARG, "rsr_physics_set_applied: on must be 0 or 1");
  if (on == (int)p->applied) return RSR_OK;                 // (on again: the values stay)
  const rsr_dims& d = p->b->model->dims;
  const size_t xb = (size_t)p->b->n * d.nbody * 6 * sizeof(float), qb = (size_t)p->b->n * d.nv * sizeof(float);
  HIPCHK(hipSetDevice(p->b->device));
  HIPCHK(hipDeviceSynchronize());               // launches in flight read the buffers (and were launched with the old choice)
  // (a failure reads "rsr_physics_set_applied: hipMalloc(xfrc)" / "(qfrc)")
  if (const int rc = applied_buffers(p, xb, qb, "rsr_physics_set_applied")) return rc;
  HIPCHK(hipMemset(p->xfrc, 0, xb));            // off: back to zero for the next time on
  HIPCHK(hipMemset(p->qfrc, 0, qb));
  HIPCHK(hipDeviceSynchronize());
  p->applied = on != 0;
  return RSR_OK;
}

extern "C" int rsr_physics_applied_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  if (!p || !dev_ptr || !shape || !stride) return fail(RSR_ERR_ARG, "rsr_physics_applied_view: null argument");
  if (!p->applied) return fail(RSR_ERR_ARG, "rsr_physics_applied_view: applied forces are off (rsr_physics_set_applied)");
  const rsr_dims& d = p->b->model->dims;
  switch (field) {
    case RSR_A_XFRC_APPLIED: return view_out(p, p->xfrc, 6 * d.nbody, 6 * d.nbody, dev_ptr, shape, stride);
    case RSR_A_QFRC_APPLIED: return view_out(p, p->qfrc, d.nv, d.nv, dev_ptr, shape, stride);
    default: return fail(RSR_ERR_ARG, "rsr_physics_applied_view: unknown field id");
  }
}

// the dynamics buffer and the site table, on first use: both or neither
static int dyn_buffers(rsr_physics* p, const char* who) {
  const bool had = p->dyn != nullptr;
  if (const int rc = zeroed_once(p, &p->dyn, (size_t)p->b->n * rsr::dyn_layout(p->b->model->dims.nv).stride * sizeof(float), "dynamics buffer", who)) return rc;
  const int rc = zeroed_once(p, &p->jac_sites, RSR_MAX_JAC_SITES * sizeof(int), "site table", who);
  if (rc && !had) { (void)hipFree(p->dyn); p->dyn = nullptr; }
  return rc;
}

extern "C" int rsr_physics_set_jac_sites(rsr_physics* p, const int32_t* site_ids, int nsite) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_set_jac_sites: null handle");
  if (nsite < 0 || nsite > RSR_MAX_JAC_SITES || (nsite > 0 && !site_ids))
    return fail(RSR_ERR_ARG, "rsr_physics_set_jac_sites: nsite must lie in [0, " + std::to_string(RSR_MAX_JAC_SITES) + "] and the table must not be null");
  for (int k = 0; k < nsite; ++k)
    if (site_ids[k] < 0 || site_ids[k] >= p->b->model->dims.nsite)
      return fail(RSR_ERR_ARG, "rsr_physics_set_jac_sites: site " + std::to_string(k) + ": site id out of range");
  if (const int rc = dyn_buffers(p, "rsr_physics_set_jac_sites")) return rc;
  HIPCHK(hipSetDevice(p->b->device));
  HIPCHK(hipDeviceSynchronize());               // launches in flight read the table
  if (nsite > 0) HIPCHK(hipMemcpy(p->jac_sites, site_ids, nsite * sizeof(int32_t), hipMemcpyHostToDevice));
  p->njac = nsite;
  return RSR_OK;
}

extern "C" int rsr_physics_dynamics(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_dynamics: null handle");
  int n;
  if (const int rc = env_count(p, env_ids, count, "rsr_physics_dynamics", &n)) return rc;
  if (const int rc = dyn_buffers(p, "rsr_physics_dynamics")) return rc;
  return physics_launch(p, rsr::OP_PHYS_DYNAMICS, physics_args(p, nullptr, env_ids, n, 1, hip_stream), "rsr_physics_dynamics");
}

extern "C" int rsr_physics_dynamics_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  if (!p || !dev_ptr || !shape || !stride) return fail(RSR_ERR_ARG, "rsr_physics_dynamics_view: null argument");
  const int nv = p->b->model->dims.nv;
  const rsr::DynLayout DL = rsr::dyn_layout(nv);
  int off = -1, w = 0;
  switch (field) {
    case RSR_D_QM: off = DL.qM; w = nv * nv; break;
    case RSR_D_QFRC_BIAS: off = DL.bias; w = nv; break;
    case RSR_D_QFRC_PASSIVE: off = DL.passive; w = nv; break;
    case RSR_D_QFRC_ACTUATOR: off = DL.actuator; w = nv; break;
    case RSR_D_JAC: off = DL.jac; w = p->njac * 6 * nv; break;
    case RSR_D_JAC_SITE_XPOS: off = DL.sxpos; w = p->njac * 3; break;
    default: return fail(RSR_ERR_ARG, "rsr_physics_dynamics_view: unknown field id");
  }
  if (const int rc = dyn_buffers(p, "rsr_physics_dynamics_view")) return rc;
  return view_out(p, p->dyn + off, w, DL.stride, dev_ptr, shape, stride);
}

// the constraint buffer, on first use
static int con_buffer(rsr_physics* p, const char* who) {
  const rsr_dims& d = p->b->model->dims;
  return zeroed_once(p, &p->con, (size_t)p->b->n * rsr::con_layout(d.nv, d.nefc_max, d.ncon_max).stride * sizeof(float), "constraint buffer", who);
}

extern "C" int rsr_physics_constraint(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_constraint: null handle");
  int n;
  if (const int rc = env_count(p, env_ids, count, "rsr_physics_constraint", &n)) return rc;
  if (const int rc = con_buffer(p, "rsr_physics_constraint")) return rc;
  return physics_launch(p, rsr::OP_PHYS_CONSTRAINT, physics_args(p, nullptr, env_ids, n, 1, hip_stream), "rsr_physics_constraint");
}

extern "C" int rsr_physics_constraint_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  if (!p || !dev_ptr || !shape || !stride) return fail(RSR_ERR_ARG, "rsr_physics_constraint_view: null argument");
  const rsr_dims& d = p->b->model->dims;
  const rsr::ConLayout CL = rsr::con_layout(d.nv, d.nefc_max, d.ncon_max);
  int off = -1, w = 0;
  switch (field) {
    case RSR_C_QFRC_CONSTRAINT: off = CL.qfc; w = d.nv; break;
    case RSR_C_QACC: off = CL.qacc; w = d.nv; break;
    case RSR_C_EFC_COUNTS: off = CL.counts; w = 4; break;
    case RSR_C_EFC_FORCE: off = CL.force; w = d.nefc_max; break;
    case RSR_C_NCON: off = CL.ncon; w = 1; break;
    case RSR_C_CONTACT: off = CL.con; w = 9 * d.ncon_max; break;
    case RSR_C_CONTACT_WRENCH: off = CL.wrench; w = 7 * d.ncon_max; break;
    default: return fail(RSR_ERR_ARG, "rsr_physics_constraint_view: unknown field id");
  }
  if (const int rc = con_buffer(p, "rsr_physics_constraint_view")) return rc;
  return view_out(p, p->con + off, w, CL.stride, dev_ptr, shape, stride);
}

// the transition buffer and, with `states`, the states buffer, each on first use
static int fd_buffers(rsr_physics* p, const rsr::FdLayout& FL, bool states, const char* who) {
  if (const int rc = zeroed_once(p, &p->fd, (size_t)p->b->n * FL.env * sizeof(float), "transition buffer", who)) return rc;
  return states ? zeroed_once(p, &p->fd_states, (size_t)p->b->n * FL.ncol * 2 * (FL.xw + FL.yw) * sizeof(float), "states buffer", who) : RSR_OK;
}

extern "C" int rsr_physics_transition_fd(rsr_physics* p, const int32_t* env_ids, int count, int nsteps, float eps, int flags, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_transition_fd: null handle");
  if (nsteps < 1 || nsteps > INT32_MAX / 2) return fail(RSR_ERR_ARG, "rsr_physics_transition_fd: nsteps must lie in [1, 2^30)");
  if (!std::isfinite(eps) || !(eps > 0.0f)) return fail(RSR_ERR_ARG, "rsr_physics_transition_fd: eps must be finite and > 0");
  if (flags & ~(RSR_FD_CENTERED | RSR_FD_STATES)) return fail(RSR_ERR_ARG, "rsr_physics_transition_fd: unknown flag bits");
  int n;
  if (const int rc = env_count(p, env_ids, count, "rsr_physics_transition_fd", &n)) return rc;
  const rsr_dims& d = p->b->model->dims;
  const rsr::FdLayout FL = rsr::fd_layout(d.nq, d.nv, d.nu);
  const int64_t grid = (int64_t)n * FL.ncol;      // one wave per (env, column)
  if (grid > INT32_MAX) return fail(RSR_ERR_ARG, "rsr_physics_transition_fd: envs x columns must stay below 2^31");
  const bool states = (flags & RSR_FD_STATES) != 0;
  if (const int rc = fd_buffers(p, FL, states, "rsr_physics_transition_fd")) return rc;
  rsr::Launch x = physics_args(p, nullptr, nullptr, (int)grid, nsteps, hip_stream);
  x.ph.fd = rsr::FdArgs{p->fd, states ? p->fd_states : nullptr, env_ids, eps, flags};
  return physics_launch(p, rsr::OP_PHYS_TRANSITION, x, "rsr_physics_transition_fd");
}

extern "C" int rsr_physics_transition_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  if (!p || !dev_ptr || !shape || !stride) return fail(RSR_ERR_ARG, "rsr_physics_transition_view: null argument");
  const rsr_dims& d = p->b->model->dims;
  const rsr::FdLayout FL = rsr::fd_layout(d.nq, d.nv, d.nu);
  const int xrow = FL.ncol * 2 * FL.xw, yrow = FL.ncol * 2 * FL.yw;
  switch (field) {
    case RSR_T_COLUMNS: case RSR_T_STATES_X: case RSR_T_STATES_Y: break;
    default: return fail(RSR_ERR_ARG, "rsr_physics_transition_view: unknown field id");
  }
  if (const int rc = fd_buffers(p, FL, field != RSR_T_COLUMNS, "rsr_physics_transition_view")) return rc;
  if (field == RSR_T_COLUMNS) return view_out(p, p->fd, FL.env, FL.env, dev_ptr, shape, stride);
  if (field == RSR_T_STATES_X) return view_out(p, p->fd_states, xrow, xrow, dev_ptr, shape, stride);
  return view_out(p, p->fd_states + (size_t)p->b->n * xrow, yrow, yrow, dev_ptr, shape, stride);
}

// The nominal scratch, at least `floats` long: allocated by the first call that needs it, and replaced only by a call that needs
// more, after a wait for the device (launches in flight read the one there).  Not zeroed: every row read was written by the same call.
static int nominal_scratch(rsr_physics* p, size_t floats, const char* who) {
  if (floats <= p->nominal_floats) return RSR_OK;
  HIPCHK(hipSetDevice(p->b->device));
  if (p->nominal) HIPCHK(hipDeviceSynchronize());
  float* buf = nullptr;
  if (hipMalloc(&buf, floats * sizeof(float)) != hipSuccess) return fail(RSR_ERR_NOMEM, std::string(who) + ": hipMalloc(nominal scratch)");
  if (p->nominal) (void)hipFree(p->nominal);
  p->nominal = buf;
  p->nominal_floats = floats;
  return RSR_OK;
}

// Two launches on the caller's stream: the nominal trajectory, one wave per slot, then every column of every control step.
extern "C" int rsr_physics_trajectory_fd(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, int T, int nsteps,
                                         float eps, int flags, const rsr_trajectory_fd_out* out, void* hip_stream) {
  const char* who = "rsr_physics_trajectory_fd";
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: null handle");
  if (!ctrl) return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: null ctrl");
  if (!out || !out->columns) return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: null out, or null out->columns");
  if (T < 1) return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: T must be >= 1");
  if (nsteps < 1 || nsteps > INT32_MAX / 2) return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: nsteps must lie in [1, 2^30)");
  if (!std::isfinite(eps) || !(eps > 0.0f)) return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: eps must be finite and > 0");
  if (flags & ~RSR_FD_CENTERED) return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: only RSR_FD_CENTERED is accepted");
  int n;
  if (const int rc = env_count(p, env_ids, count, who, &n)) return rc;
  const rsr_dims& d = p->b->model->dims;
  const rsr::FdLayout FL = rsr::fd_layout(d.nq, d.nv, d.nu);
  const int64_t cells = (int64_t)n * T;           // (slot, t): one row of the scratch each; one wave per (slot, t, column)
  if ((int64_t)T * nsteps > INT32_MAX || cells > INT32_MAX || cells * FL.ncol > INT32_MAX)
    return fail(RSR_ERR_ARG, "rsr_physics_trajectory_fd: T x nsteps and envs x T x columns must stay below 2^31");
  if (const int rc = nominal_scratch(p, (size_t)cells * (d.nq + 2 * d.nv), who)) return rc;
  rsr::Launch x = physics_args(p, nullptr, env_ids, n, nsteps, hip_stream);
  x.ph.tj = rsr::TrajArgs{ctrl, T, p->nominal, out->qpos, out->qvel, out->columns, eps, flags};
  if (const int rc = physics_launch(p, rsr::OP_TRAJ_NOMINAL, x, who)) return rc;
  x.grid = (int)(cells * FL.ncol);
  return physics_launch(p, rsr::OP_TRAJ_FD, x, who);
}

// One launch, one wave per slot (rsr_lqr.hpp).  The handle gives nv, nu, the device and the family's entry; none of its buffers is used.
extern "C" int rsr_physics_lqr_backward(rsr_physics* p, int M, int T, const float* columns, int row_stride, const rsr_lqr_cost* cost,
                                        const float* mu, int flags, const rsr_lqr_out* out, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: null handle");
  if (!columns || !cost || !mu || !out) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: null columns, cost, mu or out");
  if (!cost->lx || !cost->lu || !cost->lxx || !cost->luu) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: cost needs lx, lu, lxx and luu (only lux may be null)");
  if (!out->gain || !out->k || !out->dv || !out->status) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: out needs gain, k, dv and status (only vx and vxx may be null)");
  if (M < 1 || T < 1) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: M and T must be >= 1");
  const rsr_dims& d = p->b->model->dims;
  if (row_stride < 2 * d.nv) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: row_stride must be >= 2 nv");
  if (flags & ~RSR_LQR_REG_STATE) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: unknown flag bits");
  if ((int64_t)M * ((int64_t)T + 1) > INT32_MAX) return fail(RSR_ERR_ARG, "rsr_physics_lqr_backward: M x (T + 1) must stay below 2^31");
  rsr::Launch x = physics_args(p, nullptr, nullptr, M, 1, hip_stream);
  x.ph.lq = rsr::LqrArgs{columns, row_stride, T, cost->lx, cost->lu, cost->lxx, cost->luu, cost->lux, mu, flags,
                         out->gain, out->k, out->dv, out->status, out->vx, out->vxx};
  return physics_launch(p, rsr::OP_LQR_BACKWARD, x, "rsr_physics_lqr_backward");
}

// The same launch with the bounds on k_t (box_backward_kernel, rsr_lqr.hpp).  None of the handle's buffers is used.
extern "C" int rsr_physics_lqr_box(rsr_physics* p, int M, int T, const float* columns, int row_stride, const rsr_lqr_cost* cost,
                                   const rsr_lqr_box* box, const float* mu, int max_iter, int flags, const rsr_lqr_out* out, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: null handle");
  if (!columns || !cost || !box || !mu || !out) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: null columns, cost, box, mu or out");
  if (!cost->lx || !cost->lu || !cost->lxx || !cost->luu) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: cost needs lx, lu, lxx and luu (only lux may be null)");
  if (!box->lo || !box->hi) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: box needs lo and hi (only clamped and qp may be null)");
  if (!out->gain || !out->k || !out->dv || !out->status) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: out needs gain, k, dv and status (only vx and vxx may be null)");
  if (M < 1 || T < 1) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: M and T must be >= 1");
  const rsr_dims& d = p->b->model->dims;
  if (row_stride < 2 * d.nv) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: row_stride must be >= 2 nv");
  if (max_iter < 1 || max_iter > 64) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: max_iter must lie in [1, 64]");
  if (flags & ~RSR_LQR_REG_STATE) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: unknown flag bits");
  if ((int64_t)M * ((int64_t)T + 1) > INT32_MAX) return fail(RSR_ERR_ARG, "rsr_physics_lqr_box: M x (T + 1) must stay below 2^31");
  rsr::Launch x = physics_args(p, nullptr, nullptr, M, 1, hip_stream);
  x.ph.bx = rsr::BoxArgs{rsr::LqrArgs{columns, row_stride, T, cost->lx, cost->lu, cost->lxx, cost->luu, cost->lux, mu, flags,
                                      out->gain, out->k, out->dv, out->status, out->vx, out->vxx},
                         box->lo, box->hi, box->clamped, box->qp, max_iter};
  return physics_launch(p, rsr::OP_BOX_BACKWARD, x, "rsr_physics_lqr_box");
}

// One launch, one wave per slot (rsr_kalman.hpp).  The handle gives nv, nu, the device and the family's entry; none of its buffers is used.
extern "C" int rsr_physics_kalman(rsr_physics* p, int M, int T, const float* columns, int row_stride, int ny, const rsr_kalman_in* in,
                                  int flags, const rsr_kalman_out* out, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_kalman: null handle");
  if (!columns || !in || !out) return fail(RSR_ERR_ARG, "rsr_physics_kalman: null columns, in or out");
  if (!in->dy || !in->r || !in->q || !in->P0) return fail(RSR_ERR_ARG, "rsr_physics_kalman: in needs dy, r, q and P0 (only x0 may be null)");
  if (!out->xf || !out->status) return fail(RSR_ERR_ARG, "rsr_physics_kalman: out needs xf and status");
  if ((out->xs || out->ps) && !out->pf) return fail(RSR_ERR_ARG, "rsr_physics_kalman: xs and ps need pf");
  if (out->ps && !out->xs) return fail(RSR_ERR_ARG, "rsr_physics_kalman: ps needs xs");
  if (M < 1 || T < 1) return fail(RSR_ERR_ARG, "rsr_physics_kalman: M and T must be >= 1");
  const rsr_dims& d = p->b->model->dims;
  if (ny < 1 || ny > RSR_MAX_SENSORDATA) return fail(RSR_ERR_ARG, "rsr_physics_kalman: ny must lie in [1, " + std::to_string(RSR_MAX_SENSORDATA) + "]");
  if (row_stride < 2 * d.nv + ny) return fail(RSR_ERR_ARG, "rsr_physics_kalman: row_stride must be >= 2 nv + ny");
  if (flags != 0) return fail(RSR_ERR_ARG, "rsr_physics_kalman: unknown flag bits");
  if ((int64_t)M * ((int64_t)T + 1) > INT32_MAX) return fail(RSR_ERR_ARG, "rsr_physics_kalman: M x (T + 1) must stay below 2^31");
  rsr::Launch x = physics_args(p, nullptr, nullptr, M, 1, hip_stream);
  x.ph.kf = rsr::KalmanArgs{columns, row_stride, T, ny, in->dy, in->r, in->q, in->x0, in->P0, out->xf, out->pf, out->xs, out->ps,
                            out->nll, out->status};
  return physics_launch(p, rsr::OP_KALMAN, x, "rsr_physics_kalman");
}

// One launch, one wave per (slot, t'), t' = 0 .. T (rsr_expand.hpp).  The handle gives nv, nu, the device and the family's entry; none of its buffers is used.
extern "C" int rsr_physics_cost_expand(rsr_physics* p, int M, int T, const float* columns, int row_stride, int ny, const rsr_cost* cost,
                                       const rsr_cost_nominal* nominal, const rsr_cost_expansion* out, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: null handle");
  if (!cost || !nominal || !out) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: null cost, nominal or out");
  if (!out->lx || !out->lu || !out->lxx || !out->luu || !out->lux) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: out needs lx, lu, lxx, luu and lux");
  if (M < 1 || T < 1) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: M and T must be >= 1");
  if (ny < 0 || ny > RSR_MAX_SENSORDATA) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: ny must lie in [0, " + std::to_string(RSR_MAX_SENSORDATA) + "]");
  if (!(cost->w_qpos || cost->w_qvel || cost->w_ctrl || cost->w_sensor)) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: no weight is given");
  if ((cost->w_qpos || cost->w_qvel) && !nominal->dx) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: w_qpos and w_qvel need nominal->dx");
  if (cost->w_ctrl && !nominal->ctrl) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: w_ctrl needs nominal->ctrl");
  if (cost->w_sensor && ny == 0) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: w_sensor given with ny == 0");
  if (cost->w_sensor && (!nominal->sensordata || !columns)) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: w_sensor needs nominal->sensordata and columns");
  const rsr_dims& d = p->b->model->dims;
  if (cost->w_sensor && row_stride < 2 * d.nv + ny) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: row_stride must be >= 2 nv + ny");
  if ((int64_t)M * ((int64_t)T + 1) > INT32_MAX) return fail(RSR_ERR_ARG, "rsr_physics_cost_expand: M x (T + 1) must stay below 2^31");
  rsr::Launch x = physics_args(p, nullptr, nullptr, M * (T + 1), 1, hip_stream);
  x.ph.ex = rsr::ExpandArgs{columns, row_stride, T, ny, cost->ctrl_ref, cost->sensor_ref, cost->w_qpos, cost->w_qvel, cost->w_ctrl, cost->w_sensor,
                            nominal->dx, nominal->ctrl, nominal->sensordata, out->lx, out->lu, out->lxx, out->luu, out->lux};
  return physics_launch(p, rsr::OP_EXPAND, x, "rsr_physics_cost_expand");
}

// One launch, one wave per slot (rsr_ik.hpp).  The task table goes by value; none of the handle's buffers is used.
extern "C" int rsr_physics_ik(rsr_physics* p, const int32_t* env_ids, int count, const rsr_ik_task* task, const rsr_ik_in* in,
                              const rsr_ik_opt* opt, const rsr_ik_out* out, void* hip_stream) {
  const char* who = "rsr_physics_ik";
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_ik: null handle");
  if (!task || !in || !opt || !out) return fail(RSR_ERR_ARG, "rsr_physics_ik: null task, in, opt or out");
  if (!in->target_pos || !in->damping) return fail(RSR_ERR_ARG, "rsr_physics_ik: in needs target_pos and damping (target_quat and qpos0 may be null)");
  if (!out->qpos || !out->err || !out->info) return fail(RSR_ERR_ARG, "rsr_physics_ik: out needs qpos, err and info");
  int n;
  if (const int rc = env_count(p, env_ids, count, who, &n)) return rc;
  const rsr_dims& d = p->b->model->dims;
  if (task->nsite < 1 || task->nsite > RSR_MAX_JAC_SITES)
    return fail(RSR_ERR_ARG, "rsr_physics_ik: nsite must lie in [1, " + std::to_string(RSR_MAX_JAC_SITES) + "]");
  bool any = false, rot = false;
  for (int k = 0; k < task->nsite; ++k) {
    if (task->sites[k] < 0 || task->sites[k] >= d.nsite) return fail(RSR_ERR_ARG, "rsr_physics_ik: site " + std::to_string(k) + ": site id out of range");
    const float wp = task->pos_weight[k], wr = task->rot_weight[k];
    if (!std::isfinite(wp) || !std::isfinite(wr) || wp < 0.0f || wr < 0.0f) return fail(RSR_ERR_ARG, "rsr_physics_ik: site " + std::to_string(k) + ": weights must be finite and >= 0");
    any = any || wp > 0.0f || wr > 0.0f;
    rot = rot || wr > 0.0f;
  }
  if (!any) return fail(RSR_ERR_ARG, "rsr_physics_ik: every weight is zero");
  if (rot && !in->target_quat) return fail(RSR_ERR_ARG, "rsr_physics_ik: a positive rot_weight needs target_quat");
  if (d.nv < 32 && (task->dofs >> d.nv) != 0u) return fail(RSR_ERR_ARG, "rsr_physics_ik: dofs has a bit at or above nv");
  if (opt->iters < 0) return fail(RSR_ERR_ARG, "rsr_physics_ik: iters must be >= 0");
  if (!std::isfinite(opt->tol_pos) || !std::isfinite(opt->tol_rot) || !std::isfinite(opt->max_step) || opt->tol_pos < 0.0f || opt->tol_rot < 0.0f || opt->max_step < 0.0f)
    return fail(RSR_ERR_ARG, "rsr_physics_ik: tol_pos, tol_rot and max_step must be finite and >= 0");
  if (opt->limits != 0 && opt->limits != 1) return fail(RSR_ERR_ARG, "rsr_physics_ik: limits must be 0 or 1");
  rsr::Launch x = physics_args(p, nullptr, nullptr, n, 1, hip_stream);
  rsr::IkArgs& q = x.ph.ik = rsr::IkArgs{};
  q.target_pos = in->target_pos; q.target_quat = in->target_quat; q.qpos0 = in->qpos0; q.damping = in->damping; q.ids = env_ids;
  q.qpos = out->qpos; q.err = out->err; q.info = out->info;
  for (int k = 0; k < task->nsite; ++k) { q.sites[k] = task->sites[k]; q.wp[k] = task->pos_weight[k]; q.wr[k] = task->rot_weight[k]; }
  q.dofs = task->dofs; q.nsite = task->nsite; q.iters = opt->iters; q.limits = opt->limits;
  q.tol_pos = opt->tol_pos; q.tol_rot = opt->tol_rot; q.max_step = opt->max_step;
  return physics_launch(p, rsr::OP_IK, x, who);
}

// the inverse buffer, on first use
static int inv_buffer(rsr_physics* p, const char* who) {
  const rsr_dims& d = p->b->model->dims;
  return zeroed_once(p, &p->inv, (size_t)p->b->n * rsr::inv_layout(d.nv, d.nefc_max).stride * sizeof(float), "inverse buffer", who);
}

extern "C" int rsr_physics_inverse(rsr_physics* p, const float* qacc, const int32_t* env_ids, int count, int flags, void* hip_stream) {
  if (!p) return fail(RSR_ERR_ARG, "rsr_physics_inverse: null handle");
  if (!qacc) return fail(RSR_ERR_ARG, "rsr_physics_inverse: null qacc");
  if (flags & ~RSR_INV_DISCRETE) return fail(RSR_ERR_ARG, "rsr_physics_inverse: unknown flag bits");
  int n;
  if (const int rc = env_count(p, env_ids, count, "rsr_physics_inverse", &n)) return rc;
  if (const int rc = inv_buffer(p, "rsr_physics_inverse")) return rc;
  rsr::Launch x = physics_args(p, nullptr, env_ids, n, 1, hip_stream);
  x.ph.inv = rsr::InvArgs{p->inv, env_ids, qacc, flags};
  return physics_launch(p, rsr::OP_PHYS_INVERSE, x, "rsr_physics_inverse");
}

extern "C" int rsr_physics_inverse_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  if (!p || !dev_ptr || !shape || !stride) return fail(RSR_ERR_ARG, "rsr_physics_inverse_view: null argument");
  const rsr_dims& d = p->b->model->dims;
  const rsr::InvLayout IL = rsr::inv_layout(d.nv, d.nefc_max);
  int off = -1, w = 0;
  switch (field) {
    case RSR_I_QFRC_INVERSE: off = IL.qfi; w = d.nv; break;
    case RSR_I_QFRC_CONSTRAINT: off = IL.qfc; w = d.nv; break;
    case RSR_I_QACC: off = IL.qacc; w = d.nv; break;
    case RSR_I_QFRC_ACTUATOR: off = IL.act; w = d.nv; break;
    case RSR_I_EFC_COUNTS: off = IL.counts; w = 4; break;
    case RSR_I_EFC_FORCE: off = IL.force; w = d.nefc_max; break;
    default: return fail(RSR_ERR_ARG, "rsr_physics_inverse_view: unknown field id");
  }
  if (const int rc = inv_buffer(p, "rsr_physics_inverse_view")) return rc;
  return view_out(p, p->inv + off, w, IL.stride, dev_ptr, shape, stride);
}
