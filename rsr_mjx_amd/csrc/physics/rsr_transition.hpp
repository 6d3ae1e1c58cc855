// rsr_transition.hpp -- rsr_physics_transition_fd (include/rsr_physics.h): finite-difference Jacobians of the physics step, MuJoCo's
// mjd_transitionFD.  With x = (qpos, qvel), u = ctrl of the record and F = rsr_physics_step(u, nsteps), column k of
// [A B; C D] is (F(x (+) eps e_k) (-) F(x (-) eps e_k)) / (2 eps), or (F(x (+) eps e_k) (-) F(x)) / eps when not centred, with
// (+) and (-) taken in the tangent space of qpos (mj_integratePos / mj_differentiatePos).  No ctrl-range handling: ctrl is moved
// by +-eps wherever it stands (MuJoCo nudges it back into the range).
//
// One wave per (env, column): the grid is count x ncol, so a few dozen envs already fill the machine, and no replica batch is
// needed.  The wave makes its two runs one after the other from LDS, each exactly the run of physics_kernel<C, true> on the
// perturbed record -- the same written-out load, load_overrides, forward<C> / integrate<C> per substep with the warm start
// carried in its register from the record's, sensor_stage<C> after the last pass -- so each run is bit for bit the step it stands
// for (tests/test_transition_gpu.py).  Between the runs the first end state (qpos, qvel, sensordata) waits in a few words of LDS
// behind Smem<C> that the launch adds (fd_lds_bytes): held in three registers across the second run's solver it spills in the
// Go2 joystick kernels, which have none to spare.  Nothing but the transition buffer (and the states buffer, when asked for) is
// written.
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_sensors.hpp"
#include "rsr_applied.hpp"

namespace rsr {

// x (+) dlt e_col in LDS.  col < nv: mj_integratePos(qpos, dlt e_col): hinge / slide and free-joint translations add; a free
// joint's rotation multiplies its quaternion on the right by exp(dlt e / 2) and normalises (mju_quatIntegrate).  Then qvel, ctrl.
template <class C>
__device__ __forceinline__ void perturb_state(const Hot& h, Smem<C>& s, int lane, int col, float dlt) {
  if (col < C::NV) {                             // (wave-uniform)
    const int lr = lrec_lane(lane);
    const int4 rj_ids = lrec<C>(h, LQ_J_IDS, lr), rj_ax = lrec<C>(h, LQ_J_AX, lr);     // joint type; (axis z, qposadr, dofadr, -)
    if (lane < C::NJ) {
      const int qa = rj_ax.y, k = col - rj_ax.z;
      if (rj_ids.z == JNT_FREE) {
        if (k >= 0 && k < 3) s.qpos[qa + k] += dlt;
        else if (k >= 3 && k < 6) {
          float sn, cs;
          sincosf(0.5f * dlt, &sn, &cs);
          Q4 q = qmul(ld4(&s.qpos[qa + 3]), Q4{cs, k == 3 ? sn : 0.0f, k == 4 ? sn : 0.0f, k == 5 ? sn : 0.0f});
          const float qn = fsqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
          if (qn < RSR_MINVAL) q = Q4{1, 0, 0, 0};
          else { const float inv = frcp(qn); q = Q4{q.w * inv, q.x * inv, q.y * inv, q.z * inv}; }
          st4(&s.qpos[qa + 3], q);
        }
      } else if (k == 0) {
        s.qpos[qa] += dlt;
      }
    }
  } else if (col < 2 * C::NV) {
    if (lane == col - C::NV) s.qvel[lane] += dlt;
  } else {
    if (lane == col - 2 * C::NV) s.ctrl[lane] += dlt;
  }
}

// mj_differentiatePos(yq, s.qpos) with dt = 1, this dof lane's component: yq (-) s.qpos in the tangent space.  yq: lane t holds
// the minuend's qpos[t]; the subtrahend is in LDS.  A free joint's rotation: the rotation vector of conj(q-) q+ (mju_subQuat,
// mju_quat2Vel), in the frame the perturbation was made in.  Called by all lanes (cross-lane reads in uniform code).
// zero_at_equal: where the two quaternions are equal bit for bit the rotation's difference is 0, as in MuJoCo.  Without it it is
// the rounding residue of the product's contracted fmas, about 1e-8, which the finite differences have always carried: their
// callers leave it off and compile to the code they had.  A caller that multiplies the difference by a gain and closes a loop
// on it asks for the exact zero.
template <class C>
__device__ __forceinline__ float differentiate_pos(const Hot& h, const Smem<C>& s, int lane, float yq, bool zero_at_equal = false) {
  const int lr = lrec_lane(lane);
  const int4 rd_ids = lrec<C>(h, LQ_D_IDS, lr), rd_act = lrec<C>(h, LQ_D_ACT, lr);     // (-, -, joint type, k); (-, -, qposadr, -)
  const bool fr = lane < C::NV && rd_ids.z == JNT_FREE, rot = fr && rd_ids.w >= 3;
  const int qa = lane < C::NV ? rd_act.z + (rot ? 3 : (fr ? rd_ids.w : 0)) : 0;
  float pq[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) pq[c] = __shfl(yq, qa + c < 64 ? qa + c : 63);
  if (!rot) return pq[0] - s.qpos[qa];
  const Q4 qm = ld4(&s.qpos[qa]);
  if (zero_at_equal && qm.w == pq[0] && qm.x == pq[1] && qm.y == pq[2] && qm.z == pq[3]) return 0.0f;
  const Q4 dq = qmul(Q4{qm.w, -qm.x, -qm.y, -qm.z}, Q4{pq[0], pq[1], pq[2], pq[3]});
  const float sn = fsqrt(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z);
  float speed = 2.0f * atan2f(sn, dq.w);
  if (speed > 3.14159265358979f) speed -= 6.28318530717959f;         // the short way round
  const float v = rd_ids.w == 3 ? dq.x : (rd_ids.w == 4 ? dq.y : dq.z);
  return sn > 0.0f ? v * (speed / sn) : 0.0f;
}

// LDS of a transition_kernel workgroup: Smem<C>, then the waiting end state qpos [NQ] | qvel [NV] | sensordata [RSR_MAX_SENSORDATA]
template <class C>
constexpr size_t fd_park_offset() { return (sizeof(Smem<C>) + 15) & ~size_t(15); }
template <class C>
constexpr size_t fd_lds_bytes() { return fd_park_offset<C>() + (C::NQ + C::NV + RSR_MAX_SENSORDATA) * sizeof(float); }

// Workgroup b: env d.ids[b / ncol] (or b / ncol), column b % ncol.  p: the handle's PhysArgs (nsteps and the sensor table; its
// buffers are not written).  Ap: none, or Applied: the applied forces enter every pass as in the applied physics kernels.
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void transition_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, FdArgs d, Ap... ap) {
  static_assert(C::NQ <= 64 && C::NV <= 64 && C::NU <= 64 && RSR_MAX_SENSORDATA <= 64, "one lane per entry of the kept end state");
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  float* park = reinterpret_cast<float*>(smem_raw + fd_park_offset<C>());
  const FdLayout FL = fd_layout(C::NQ, C::NV, C::NU);
  const int slot = (int)blockIdx.x / FL.ncol, col = (int)blockIdx.x - slot * FL.ncol, lane = threadIdx.x;
  const int e = d.ids ? d.ids[slot] : slot;
  if (e < 0 || e >= a.n) return;                                // (an id out of range runs nothing)
  const float* rec = a.state + (size_t)e * L.rec;
  const auto stage = force_stage<C>(e, ap.xfrc..., ap.qfrc...);
  PROF_DECL
  const int nsd = p.sens.nsd;
  const size_t cell = (size_t)e * FL.ncol + col;
  float* sx = d.states ? d.states + cell * 2 * FL.xw : nullptr;
  float* sy = d.states ? d.states + (size_t)a.n * FL.ncol * 2 * FL.xw + cell * 2 * FL.yw : nullptr;
  // a run's start: the record load of physics_kernel, written out (the record's ctrl and warm start), then the perturbation
  float warm = 0.0f;
  auto begin_run = [&](int run, float dlt) {
    const int ln = lrec_lane(lane);             // opaque, so that no address of the first run's load stays live across the solver for the second
    for (int t = ln; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
    if (ln < C::NV) { s.qvel[ln] = rec[L.qvel + ln]; warm = rec[L.warm + ln]; }
    load_overrides<C>(m, s, a, e, ln);
    if (ln < C::NU) s.ctrl[ln] = rec[L.ctrl + ln];
    if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
      if (ln == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
    }
    WSYNC();
    // dlt through the opaque zero of ln: the second run's -eps, and the sine and cosine of its half, are otherwise formed at the
    // kernel's start and held (spilled, in the Go2 joystick kernels) across both runs' solvers
    const float dl = asf(__builtin_bit_cast(int, dlt) + (ln - lane));
    if (dlt != 0.0f) perturb_state<C>(hot, s, ln, col, dl);      // (wave-uniform; not centred: the second run is the record's own state)
    WSYNC();
    if (sx) {
      float* o = sx + run * FL.xw;
      for (int t = ln; t < C::NQ; t += 64) o[t] = s.qpos[t];
      if (ln < C::NV) o[C::NQ + ln] = s.qvel[ln];
      if (ln < C::NU) o[C::NQ + C::NV + ln] = s.ctrl[ln];
    }
  };
  float Mrow[C::NV];
  FwdOut<C> f;
  begin_run(0, d.eps);
  // the two runs as one loop over their 2 * nsteps substeps, the end of a run a wave-uniform branch, as in rollout_kernel (a loop
  // over runs around the substep loop costs the Go2 kernels registers they do not have)
  const int total = 2 * p.nsteps;              // (nsteps < 2^30: rsr_physics_transition_fd)
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
    if (sy) {
      float* o = sy + run * FL.yw;
      for (int t = lt; t < C::NQ; t += 64) o[t] = s.qpos[t];
      if (lt < C::NV) o[C::NQ + lt] = s.qvel[lt];
    }
    const bool centered = (d.flags & RSR_FD_CENTERED) != 0;
    if (run == 0) {
      if (lt < C::NQ) park[lt] = s.qpos[lt];
      if (lt < C::NV) park[C::NQ + lt] = s.qvel[lt];
      park[C::NQ + C::NV + lt] = sv;
      WSYNC();                                   // the next run's load overwrites what was just read
      run = 1;
      begin_run(1, centered ? -d.eps : 0.0f);
    } else {
      // the column: one contiguous row of the buffer, every entry of it (past the sensordata: zeros)
      const float hstep = centered ? 2.0f * d.eps : d.eps;
      const float yq = lt < C::NQ ? park[lt] : 0.0f, yv = lt < C::NV ? park[C::NQ + lt] : 0.0f, ys = park[C::NQ + C::NV + lt];
      const float dq = differentiate_pos<C>(hot, s, lt, yq);
      float* o = d.out + cell * FL.w;
      if (lt < C::NV) { o[lt] = dq / hstep; o[C::NV + lt] = (yv - s.qvel[lt]) / hstep; }
      o[2 * C::NV + lt] = lt < nsd ? (ys - sv) / hstep : 0.0f;
    }
  }
}

}  // namespace rsr
