// rsr_ik.hpp -- rsr_physics_ik (include/rsr_physics.h): damped least squares on site pose targets, M independent problems in one
// launch.  One wave per slot keeps the problem in LDS and runs every iteration without returning to the host: the kinematics
// stage of forward<C> at the iterate, the pose errors of up to RSR_MAX_JAC_SITES sites, the stop test, com_crb_mass for cdof and
// com, the site Jacobians of rsr_physics_dynamics (site_jac, rsr_dynamics.hpp), J^T J + lambda I and J^T b with lane = dof, the
// in-register L D L^T the family takes for its mass matrix (two dofs share a site's chain only inside one kinematic tree, and a
// chain holds the trunk and at most one leg: C::same_tree, the per-tree rows and the block arrow each cover the pattern of J^T J
// and its fill-in), the step cap, mj_integratePos and the joint-range clamp.  The site table, the weights and the dof mask come by value in IkArgs; nothing but the caller's three output rows of the
// slot is written: not the record and no buffer of the handle.
//
// LDS: Smem<C> as every physics kernel has it (the stages write their usual fields; x.a's dead arrays are the factor's transpose
// scratch, scratch_a()), then IkDims<C>: J [48][NV] (row 6 k + c: site k, c < 3 the weighted jacp rows, c >= 3 the weighted jacr
// rows; lane i reads its column with stride 1 and every lane the same word of column j: a broadcast), the unweighted errors
// EV [48], the weighted right-hand side BW [48] and the step DQ [32].  Rows of weight 0 are neither written nor read.
// Every decision that ends or continues the loop is taken on values that all lanes computed from the same LDS words in the same
// order, and is made scalar with a readfirstlane: the wave leaves the loop as one.
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_dynamics.hpp"

namespace rsr {

template <class C>
struct IkDims {
  static constexpr int ROWS = 6 * RSR_MAX_JAC_SITES, LD = C::NV;
  static constexpr int J = 0, EV = J + ROWS * LD, BW = EV + ROWS, DQ = BW + ROWS, FLOATS = DQ + 32;   // offsets, floats
  static_assert(ROWS <= 64 && C::NV <= 32 && C::NJ <= 64, "one lane per row, per dof and per joint");
};
template <class C>
constexpr size_t ik_offset() { return (sizeof(Smem<C>) + 15) & ~size_t(15); }
template <class C>
constexpr size_t ik_lds_bytes() { return ik_offset<C>() + sizeof(float) * IkDims<C>::FLOATS; }

// the unit quaternion of q as kinematics takes a free joint's
__device__ __forceinline__ Q4 ik_unit(Q4 q) {
  const float n = fsqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  if (n < RSR_MINVAL) return Q4{1, 0, 0, 0};
  const float inv = frcp(n);
  return Q4{q.w * inv, q.x * inv, q.y * inv, q.z * inv};
}

// Workgroup s: slot s, env q.ids[s] (or s); an id out of range runs nothing.  WAVES: the family's waves per SIMD, an upper bound.
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WAVES)))
void ik_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, IkArgs q) {
  using D = IkDims<C>;
  static_assert(ik_lds_bytes<C>() <= 64 * 1024, "a workgroup's LDS");
  constexpr int NV = C::NV, LD = D::LD;
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  float* const xs = reinterpret_cast<float*>(smem_raw + ik_offset<C>());
  float *const J = xs + D::J, *const EV = xs + D::EV, *const BW = xs + D::BW, *const DQ = xs + D::DQ;
  const int lane = threadIdx.x, K = q.nsite;
  const size_t slot = blockIdx.x;
  const int e = q.ids ? q.ids[slot] : (int)slot;
  if (e < 0 || e >= a.n) return;
  PROF_DECL
  const float* start = q.qpos0 ? q.qpos0 + slot * C::NQ : a.state + (size_t)e * L.rec + L.qpos;
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = start[t];
  load_overrides<C>(m, s, a, e, lane);        // mass, and where the family has them per env: qpos0, body_ipos, armature
  const float lambda = q.damping[slot];
  // lane k < K: site k's target; lane r < 6 K: row r's weight (the table is indexed with constants: it stays in scalar registers)
  int site = 0;
  float wrow = 0.0f;
#pragma unroll
  for (int k = 0; k < RSR_MAX_JAC_SITES; ++k) {
    if (lane == k) site = q.sites[k];
    if (lane >= 6 * k && lane < 6 * k + 3) wrow = q.wp[k];
    if (lane >= 6 * k + 3 && lane < 6 * k + 6) wrow = q.wr[k];
  }
  const bool task = lane < K;
  V3 tp = v3(0, 0, 0);
  M33 Rt;
#pragma unroll
  for (int c = 0; c < 9; ++c) Rt.m[c] = (c % 4 == 0) ? 1.0f : 0.0f;
  if (task) {
    tp = ld3(q.target_pos + (slot * K + lane) * 3);
    if (q.target_quat) Rt = q2m(ik_unit(ld4(q.target_quat + (slot * K + lane) * 4)));
  }
  // lane j < NJ: joint j's addresses and range
  const int lane_j = lrec_lane(lane);
  const int4 rj_ids = lrec<C>(hot, LQ_J_IDS, lane_j), rj_ax = lrec<C>(hot, LQ_J_AX, lane_j);     // joint type; (axis z, qposadr, dofadr, -)
  const bool jn = lane < C::NJ;
  const int jt = jn ? rj_ids.z : -1, qa = rj_ax.y, da = rj_ax.z;
  const bool lim = jn && q.limits != 0 && (jt == JNT_HINGE || jt == JNT_SLIDE) && m.jnt_limited[jn ? lane : 0] != 0;
  const float lo = lim ? m.jnt_range[2 * lane] : 0.0f, hi = lim ? m.jnt_range[2 * lane + 1] : 0.0f;
  const int dl = lane < NV ? lane : 0;
  const bool moves = lane < NV && ((q.dofs >> lane) & 1u);
  WSYNC();

  int it = 0, status = 0;
  float perr = 0.0f, rerr = 0.0f;
  for (;;) {
    const int lane_s = lrec_lane(lane);
    kinematics<C>(m, hot, s, lane_s PROF_PASS);
    // e_k = p*_k - p_k and r_k = the rotation vector of R*_k R_k^T, world frame: with E = R* R^T, (E - E^T) / 2 is sin(angle) [axis]x
    // and (tr E - 1) / 2 is cos(angle); the angle lies in [0, pi], the short way round
    if (task) {
      st3(&EV[6 * lane], tp - ld3(&s.spos[3 * site]));
      V3 rv = v3(0, 0, 0);
      if (q.target_quat) {
        const float* R = &s.smat[9 * site];
        float E[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) E[3 * i + j] = Rt.m[3 * i] * R[3 * j] + Rt.m[3 * i + 1] * R[3 * j + 1] + Rt.m[3 * i + 2] * R[3 * j + 2];
        const V3 sv = v3(0.5f * (E[7] - E[5]), 0.5f * (E[2] - E[6]), 0.5f * (E[3] - E[1]));
        const float cs = 0.5f * (E[0] + E[4] + E[8] - 1.0f), sn = fsqrt(dot(sv, sv));
        if (sn > 0.0f) rv = sv * (atan2f(sn, cs) / sn);
      }
      st3(&EV[6 * lane + 3], rv);
    }
    WSYNC();
    perr = 0.0f; rerr = 0.0f;                      // (a NaN norm is kept: !(n <= x))
    for (int k = 0; k < K; ++k) {
      const V3 pe = ld3(&EV[6 * k]), re = ld3(&EV[6 * k + 3]);
      const float pn = fsqrt(dot(pe, pe)), rn = fsqrt(dot(re, re));
      if (q.wp[k] > 0.0f && !(pn <= perr)) perr = pn;
      if (q.wr[k] > 0.0f && !(rn <= rerr)) rerr = rn;
    }
    const bool conv = perr <= q.tol_pos && rerr <= q.tol_rot;
    if (uniform_i(it == q.iters || conv)) { status = conv ? 0 : 1; break; }
    if (!(lambda > 0.0f) || !(lambda < __builtin_inff())) { status = 2; break; }
    com_crb_mass<C>(m, hot, s, lane_s PROF_PASS);
    // J: the weighted rows, the columns of dofs outside the mask zero; b = the weighted errors
    for (int k = 0; k < K; ++k) {
      const int st = q.sites[k], b = m.site_bodyid[st];
      const float wp = q.wp[k], wr = q.wr[k];
      if (lane < NV) {
        const SiteJac sj = site_jac<C>(m, s, st, b, lane);
        float* j = J + 6 * k * LD + lane;
        if (wp != 0.0f) { j[0] = moves ? wp * sj.p.x : 0.0f; j[LD] = moves ? wp * sj.p.y : 0.0f; j[2 * LD] = moves ? wp * sj.p.z : 0.0f; }
        if (wr != 0.0f) { j[3 * LD] = moves ? wr * sj.r.x : 0.0f; j[4 * LD] = moves ? wr * sj.r.y : 0.0f; j[5 * LD] = moves ? wr * sj.r.z : 0.0f; }
      }
    }
    if (lane < 6 * K) BW[lane] = wrow * EV[lane];
    WSYNC();
    // lane i: row i of J^T J + lambda I and entry i of J^T b, the rows of J in ascending order, one fma per term
    float arow[NV], g = 0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) arow[j] = 0.0f;
    for (int k = 0; k < K; ++k) {
      for (int h = 0; h < 2; ++h) {
        if ((h ? q.wr[k] : q.wp[k]) == 0.0f) continue;       // (wave-uniform)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* row = J + (6 * k + 3 * h + c) * LD;
          const float ji = lane < NV ? row[dl] : 0.0f;
          g = __builtin_fmaf(ji, BW[6 * k + 3 * h + c], g);
#pragma unroll
          for (int j = 0; j < NV; ++j) arow[j] = __builtin_fmaf(ji, row[j], arow[j]);
        }
      }
    }
    // the family's factorisation, as integrate<C> takes M + h D: the layouts that read their rows from a natural-order matrix in
    // LDS find J^T J where com_crb_mass left the mass matrix, which nothing here reads, and take lambda as the diagonal term
    float x;
    if constexpr (C::ROWTREE || C::ROWCHOL || C::ARROW) {
      if (lane < NV) {
#pragma unroll
        for (int j = 0; j < NV; ++j) s.M[lane * C::LD + j] = arow[j];
      }
      WSYNC();
      float a[C::NCH], lt[C::NCH];
      if constexpr (C::ROWTREE) {
        const float dd = rowtree_dof<C>(lane) >= 0 ? lambda : 0.0f;
        const float dinv = rowtree_factor<C, true>(s.M, dd, a, lt, s.scratch_a(), lane);
        x = rowtree_solve<C>(a, lt, dinv, g, lane);
      } else if constexpr (C::ROWCHOL) {
        const float dd = rowchol_dof<C>(lane) >= 0 ? lambda : 0.0f;
        const float dinv = rowchol_factor<C, true, true>(s.M, dd, a, lt, s.scratch_a(), lane);
        x = rowchol_solve<C>(a, lt, dinv, g, lane);
      } else {
        const float dd = arrow_dof<C>(lane) >= 0 ? lambda : 0.0f;
        const float dinv = arrow_factor<C, true>(s.M, dd, a, lt, s.scratch_a(), lane);
        x = arrow_solve<C>(a, lt, dinv, g, lane);
      }
    } else {
      float lt[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) if (j == lane) arow[j] += lambda;
      const float dinv = chol_factor<C, true>(arow, lt, s.scratch_a(), lane);
      x = chol_solve<C>(arow, lt, dinv, g, lane);
    }
    if (lane < NV) DQ[lane] = x;
    WSYNC();
    float mx = 0.0f;
    bool finite = true;
    for (int j = 0; j < NV; ++j) {
      const float v = fabsf(DQ[j]);
      finite = finite && v < __builtin_inff();
      mx = v > mx ? v : mx;
    }
    if (!uniform_i(finite)) { status = 2; break; }
    const float sc = (q.max_step > 0.0f && mx > q.max_step) ? q.max_step / mx : 1.0f;
    // mj_integratePos, lane = joint; a dof outside the mask is not touched (its dq is an exact 0); then the clamp
    if (jn) {
      if (jt == JNT_FREE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) if ((q.dofs >> (da + c)) & 1u) s.qpos[qa + c] += sc * DQ[da + c];
        if ((q.dofs >> (da + 3)) & 7u) {
          const V3 v = ld3(&DQ[da + 3]) * sc;
          const float ang = fsqrt(dot(v, v));
          if (ang > 0.0f) {
            float sn, cs;
            sincosf(0.5f * ang, &sn, &cs);
            const float f = sn / ang;
            st4(&s.qpos[qa + 3], ik_unit(qmul(ld4(&s.qpos[qa + 3]), Q4{cs, v.x * f, v.y * f, v.z * f})));
          }
        }
      } else if ((q.dofs >> da) & 1u) {
        s.qpos[qa] += sc * DQ[da];
      }
      if (lim) s.qpos[qa] = clampf(s.qpos[qa], lo, hi);
    }
    WSYNC();
    ++it;
  }
  for (int t = lane; t < C::NQ; t += 64) q.qpos[slot * C::NQ + t] = s.qpos[t];
  if (lane == 0) {
    q.err[2 * slot] = perr; q.err[2 * slot + 1] = rerr;
    q.info[2 * slot] = it; q.info[2 * slot + 1] = status;
  }
}

}  // namespace rsr
