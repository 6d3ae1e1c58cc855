// rsr_applied.hpp -- applied forces of the physics layer (rsr_physics_set_applied): data.xfrc_applied / data.qfrc_applied added to
// qfrc_smooth in every forward pass of the applied physics kernels (rsr_physics_kernels.hpp).  They enter as forward<C>'s force
// stage (AppliedStage), between smooth_forces and the factorisation of M; the rows are the Applied struct of rsr_physics.hpp.
#pragma once
#include "../rsr_launch.hpp"

namespace rsr {

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

// forward<C>'s force stage (rsr_solver.hpp) in the applied physics kernels.  ap: this env's rows.
template <class C>
struct AppliedStage {
  Applied ap;
  __device__ __forceinline__ float operator()(const Hot& h, Smem<C>& s, int lane, float fs) const { return applied_forces<C>(h, s, lane, ap, fs); }
};

// forward<C>'s force stage of env e: none, or its rows of the applied forces (the handle's buffers xfrc / qfrc)
template <class C>
__device__ __forceinline__ NoForceStage force_stage(int) { return {}; }
template <class C>
__device__ __forceinline__ AppliedStage<C> force_stage(int e, const float* xfrc, const float* qfrc) {
  return {{xfrc + (size_t)e * (C::NB * 6), qfrc + (size_t)e * C::NV}};
}

}  // namespace rsr
