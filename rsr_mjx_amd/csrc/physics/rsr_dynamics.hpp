// rsr_dynamics.hpp -- rsr_physics_dynamics (include/rsr_physics.h): the model at the record's current state.  The first three
// stages of forward<C> (kinematics, com_crb_mass, smooth_forces) and then the terms they leave in LDS, written to the handle's
// dynamics buffer (DynLayout, rsr_physics.hpp): mj_fullM, data.qfrc_bias / qfrc_passive / qfrc_actuator and mj_jacSite of a table
// of sites.  No factorisation, collision, constraint rows or solve; nothing but that buffer is written.
#pragma once
#include "../rsr_launch.hpp"

namespace rsr {

// Column `dof` of mj_jacSite for a site of body b (rsr_physics_dynamics and rsr_physics_ik), after kinematics and com_crb_mass:
// cdof_i is dof i's spatial velocity about the subtree COM of its tree's root (ang, lin), so at the site jacr = ang and
// jacp = lin + ang x (site - com[root]), as smooth_forces takes slinvel from cvel; zero off the body's chain.  dof < NV.
struct SiteJac { V3 p, r; };
template <class C>
__device__ __forceinline__ SiteJac site_jac(const DModel& m, const Smem<C>& s, int site, int b, int dof) {
  const bool on = (m.body_dofmask[b] >> dof) & 1;
  const V3 dif = ld3(&s.spos[3 * site]) - ld3(&s.com[3 * m.body_rootid[b]]);
  const V3 ang = ld3(&s.cdof[6 * dof]), lin = ld3(&s.cdof[6 * dof + 3]) + cross(ang, dif);
  return SiteJac{V3{on ? lin.x : 0.0f, on ? lin.y : 0.0f, on ? lin.z : 0.0f}, V3{on ? ang.x : 0.0f, on ? ang.y : 0.0f, on ? ang.z : 0.0f}};
}

// One wave per env, a plain launch.  d.ids: the envs to run or null (env = workgroup index); an id out of range runs nothing.
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void dynamics_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, DynArgs d) {
  static_assert(C::NV <= 32, "dof masks are 32 bits; lane = dof");
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = d.ids ? d.ids[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  if (e < 0 || e >= a.n) return;
  const float* rec = a.state + (size_t)e * L.rec;
  PROF_DECL
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  if (lane < C::NV) s.qvel[lane] = rec[L.qvel + lane];
  load_overrides<C>(m, s, a, e, lane);
  if (lane < C::NU) s.ctrl[lane] = rec[L.ctrl + lane];
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  WSYNC();
  const int lane_s = lrec_lane(lane);
  kinematics<C>(m, hot, s, lane_s PROF_PASS);
  com_crb_mass<C>(m, hot, s, lane_s PROF_PASS);
  const float qvel_i = lane < C::NV ? s.qvel[lane] : 0.0f;
  (void)smooth_forces<C>(m, hot, s, lane_s, qvel_i, 0.0f PROF_PASS);
  WSYNC();
  // live now: M (both triangles, armature on the diagonal), cdof, com, the site frames, damp, aforce and smooth_forces' cfrcsum
  const DynLayout DL = dyn_layout(C::NV);
  float* o = d.out + (size_t)e * DL.stride;
  for (int t = lane; t < C::NV * C::NV; t += 64) o[DL.qM + t] = s.M[(t / C::NV) * C::LD + (t % C::NV)];
  if (lane < C::NV) {
    // the three terms of smooth_forces' qfrc_smooth = passive - bias + actuator, expression for expression
    const int4 rd_ids = lrec<C>(hot, LQ_D_IDS, lane_s), rd_act = lrec<C>(hot, LQ_D_ACT, lane_s), rd_frc = lrec<C>(hot, LQ_D_FRC, lane_s);
    const int i = lane, b = rd_ids.y;
    float bias = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) bias += s.cdof[6 * i + c] * s.x.a.cfrcsum[6 * b + c];
    const float passive = -s.damp[i] * qvel_i;
    float act = 0;
    const int u = rd_act.x;
    if (u >= 0) act = asf(rd_act.y) * s.aforce[u];       // gear * actuator_force (ctrl and force clamps are in aforce)
    if (rd_frc.y) act = clampf(act, asf(rd_frc.z), asf(rd_frc.w));      // the joint's actfrcrange
    o[DL.bias + i] = bias; o[DL.passive + i] = passive; o[DL.actuator + i] = act;
  }
  // mj_jacSite (site_jac)
  const int nsite = d.nsite;
  if (lane < 3 * nsite) o[DL.sxpos + lane] = s.spos[3 * d.sites[lane / 3] + lane % 3];
  for (int k = 0; k < nsite; ++k) {
    const int site = d.sites[k], b = m.site_bodyid[site];
    if (lane < C::NV) {
      const SiteJac J = site_jac<C>(m, s, site, b, lane);
      float* j = o + DL.jac + k * 6 * C::NV + lane;
      j[0] = J.p.x; j[C::NV] = J.p.y; j[2 * C::NV] = J.p.z;
      j[3 * C::NV] = J.r.x; j[4 * C::NV] = J.r.y; j[5 * C::NV] = J.r.z;
    }
  }
}

}  // namespace rsr
