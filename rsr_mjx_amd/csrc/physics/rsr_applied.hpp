// rsr_applied.hpp -- applied forces of the physics layer (rsr_physics_set_applied): data.xfrc_applied / data.qfrc_applied added to
// qfrc_smooth in every forward pass of the applied physics kernels (rsr_physics_kernels.hpp).  The env kernels' sources (csrc/*.hpp,
// the ones the parity envelopes were measured on) are not touched: the applied forward pass is its own function here, built from
// the same stages, with one stage of its own between smooth_forces and the factorisation of M.
#pragma once
#include "../rsr_launch.hpp"

namespace rsr {

// data.xfrc_applied [nbody*6] (force, torque: world frame, at the body's COM) and data.qfrc_applied [nv]: the handle's buffers
// ([N][...], as a kernel argument) or one env's rows (forward_applied)
struct Applied {
  const float* xfrc;
  const float* qfrc;
};

// The launch of an applied op: the op carries OP_APPLIED and the Launch is an AppliedLaunch (rsr_physics.hip builds it; the
// family units pass the reference on to launch_physics untouched).
constexpr int OP_APPLIED = 1 << 8;
struct AppliedLaunch : Launch {
  Applied ap;
};

// qfrc_smooth += qfrc_applied + sum over bodies b >= 1 of J_b(xipos_b)^T [f_b; tau_b]   (mj_xfrcAccumulate / support.xfrc_accumulate)
// Each body's wrench, moved to its tree's subtree COM like cdof and cinert, is summed over subtrees as smooth_forces sums cfrc;
// then J^T w for dof i is cdof_i . (sum over the subtree of body_i).  Runs right after smooth_forces: its cfrc / cfrcsum are dead
// then, and hold the wrenches and their sums (the factorisation of M reuses phase A only after this).  fs: this dof lane's
// qfrc_smooth; returns it with the applied forces added.
template <class C>
__device__ __forceinline__ float applied_forces(const Hot& h, Smem<C>& s, int lane, const Applied& ap, float fs) {
  const int lr = lrec_lane(lane);
  const int4 rb_misc = lrec<C>(h, LQ_B_MISC, lr), rd_ids = lrec<C>(h, LQ_D_IDS, lr);
  const int qb = lane >> 2;            // four lanes per body, as in smooth_forces
  const bool body_lane = (lane & 3) == 0 && qb < C::NB;
  float w[6] = {0, 0, 0, 0, 0, 0}, qfrc_i = 0.0f;
  if (body_lane && qb > 0) {           // (the world's row is never read: its wrench stays zero)
#pragma unroll
    for (int c = 0; c < 6; ++c) w[c] = ap.xfrc[6 * qb + c];
  }
  if (lane < C::NV) qfrc_i = ap.qfrc[lane];
  // cross-lane reads in uniform code (source lanes active)
  const unsigned sub_mask_q = (unsigned)__shfl(rb_misc.z, qb < C::NB ? qb : 0);
  const int root_q = __shfl(rb_misc.y, qb < C::NB ? qb : 0);
  WSYNC();                             // smooth_forces' last reads of cfrcsum
  if (body_lane) {
    const V3 f = v3(w[0], w[1], w[2]);
    const V3 t = v3(w[3], w[4], w[5]) + cross(ld3(&s.x.a.xipos[3 * qb]) - ld3(&s.com[3 * root_q]), f);
    float* o = &s.x.a.cfrc[6 * qb];
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = f.x; o[4] = f.y; o[5] = f.z;
  }
  WSYNC();
  subtree_sum_quad<C, 6>(s.x.a.cfrc, s.x.a.cfrcsum, qb >= C::NB ? 0u : sub_mask_q, lane);
  WSYNC();
  if (lane < C::NV) {
    const int i = lane, b = rd_ids.y;
    float jw = 0.0f;
#pragma unroll
    for (int c = 0; c < 6; ++c) jw += s.cdof[6 * i + c] * s.x.a.cfrcsum[6 * b + c];
    fs += jw + qfrc_i;
  }
  return fs;
}

// forward<C> (rsr_solver.hpp) with applied_forces after smooth_forces; no parity dump.  ap: this env's rows.
template <class C>
__device__ __forceinline__ void forward_applied(const DModel& m, const Hot& h, Smem<C>& s, int lane, float (&Mrow)[C::NV], float& warm,
                                                FwdOut<C>& out, const Applied& ap PROF_ARG) {
  kinematics<C>(m, h, s, lane PROF_PASS);
  PROF(PS_KIN)
  com_crb_mass<C>(m, h, s, lane PROF_PASS);
  load_mrow<C>(s, lane, Mrow);
  PROF(PS_COMCRB)
  float qvel_i = lane < C::NV ? s.qvel[lane] : 0.0f;
  float fs = smooth_forces<C>(m, h, s, lane, qvel_i, 0.0f PROF_PASS);
  fs = applied_forces<C>(h, s, lane, ap, fs);
  PROF(PS_SMOOTH)
  // qacc_smooth = M^-1 qfrc_smooth
  float a[C::NCH], lt[C::NCH];
  float a0;
  if constexpr (C::ROWTREE) {
    const float dinv_m = rowtree_factor<C>(s.M, 0.0f, a, lt, s.scratch_a(), lane);
    a0 = rowtree_solve<C>(a, lt, dinv_m, fs, lane);
    a0 = lane < C::NV ? a0 : 0.0f;
  } else if constexpr (C::ROWCHOL) {
    const float dinv_m = rowchol_factor<C, true>(s.M, 0.0f, a, lt, s.scratch_a(), lane);
    a0 = rowchol_solve<C>(a, lt, dinv_m, fs, lane);
    a0 = lane < C::NV ? a0 : 0.0f;
  } else if constexpr (C::ARROW) {
    const float dinv_m = arrow_factor<C>(s.M, 0.0f, a, lt, s.scratch_a(), lane);
    a0 = arrow_solve<C>(a, lt, dinv_m, fs, lane);
    a0 = lane < C::NV ? a0 : 0.0f;
  } else {
#pragma unroll
    for (int j = 0; j < C::NV; ++j) a[j] = Mrow[j];
    const float dinv_m = chol_factor<C, true>(a, lt, s.scratch_a(), lane);
    a0 = lane < C::NV ? chol_solve<C>(a, lt, dinv_m, fs, lane) : 0.0f;
  }
  PROF(PS_CHOLM)
  collision<C>(m, h, s, lane PROF_PASS);
  PROF(PS_COLL)
  RowRegs rr[C::NCHUNK];
  float bcoef[C::NCHUNK], jqv[C::NCHUNK];
  int nbase;
  int nefc = make_constraint<C>(m, h, s, lane, rr, bcoef, nbase PROF_PASS);
  {
    float qb[NVP<C>];
    vec_bcast<C>(s, lane, qvel_i, qb);
    jdot<C>(s, lane, nefc, nbase, rr, qb, jqv);
  }
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) rr[ch].aref -= bcoef[ch] * jqv[ch];
  PROF(PS_ROWS)
  out.fsmooth = fs; out.nefc = nefc;
  const bool need_force = implicit_integration<C>(h, s, lane);
  solve<C>(h, s, lane, nefc, nbase, rr, Mrow, fs, a0, warm, need_force, out.qacc, out.qfc, out.st, nullptr PROF_PASS);
  warm = out.qacc;
}

}  // namespace rsr
