// rsr_constraint.hpp -- rsr_physics_constraint (include/rsr_physics.h): the constraint side of one mjx.forward pass at the record's
// current state, written to the handle's constraint buffer (ConLayout, rsr_physics.hpp): data.efc_force, data.qfrc_constraint, the
// pass's qacc and contact list, and the wrench of every contact (mj_contactForce, rotated to the world frame).  Nothing but that
// buffer is written: the record keeps its qacc_warmstart, xpos and site_xpos.
//
// The pass is forward<C> (rsr_solver.hpp), called once with the force stage of the physics kernels and a rows tail (RowForces):
// the tail sees the per-row registers of make_constraint and the solver's qacc and does what MJX's _update_constraint does after
// the last iteration: jaref = J qacc - aref, the row forces (rows_cost), J^T force (jt_force).  solve()'s own qfrc_constraint is
// not used: a single-iteration solve that nobody asks for the force (the Go2 models) never forms it.  qacc and the contact list
// are bit-identical to what rsr_physics_forward gives on the same record (tests/test_constraint_gpu.py).
#pragma once
#include "../rsr_launch.hpp"
#include "rsr_applied.hpp"

namespace rsr {

// One wave per env, a plain launch.  d.ids: the envs to run or null (env = workgroup index); an id out of range runs nothing.
// d.out: the constraint buffer.  Ap: none, or Applied: the applied forces enter the pass as in the applied physics kernels.
template <class C, int WAVES, class... Ap>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void constraint_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, ConArgs d, Ap... ap) {
  static_assert(C::NBC == 3 || C::NBC == 4, "contact wrench: frictional contacts with or without torsion");
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = d.ids ? d.ids[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  if (e < 0 || e >= a.n) return;
  const float* rec = a.state + (size_t)e * L.rec;
  const auto stage = force_stage<C>(e, ap.xfrc..., ap.qfrc...);
  PROF_DECL
  // the record load of physics_kernel (the record's ctrl)
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float warm = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; warm = rec[L.warm + lane]; }
  load_overrides<C>(m, s, a, e, lane);
  if (lane < C::NU) s.ctrl[lane] = rec[L.ctrl + lane];
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  WSYNC();
  const int lane_s = lrec_lane(lane);
  float Mrow[C::NV], force[C::NCHUNK], qfc;
  FwdOut<C> f;
  // The rows tail: the rows at the solver's qacc, each row's force (force[ch]: row lane + 64 ch) and this lane's qfrc_constraint.
  // Live in LDS after the solve: the base rows J, bmu, sdof, the contact list with its normalised normals.  Dead: M under
  // Dims::TALIAS (the Hessian's scratch), the tangents the rows' construction staged in rw, and whatever the last factorisation
  // left in jtp | bval | wc | rw; jdot and jt_force rewrite every word of bval and rw that they read, as inside the solver's loop.
  forward<C>(m, hot, s, lane_s, Mrow, warm, f, nullptr PROF_PASS, stage,      // (warm dies here: the record keeps its own)
             [&](Smem<C>& s, int lane_s, int nefc, int nbase, const RowRegs (&rr)[C::NCHUNK], float qacc) {
    if constexpr (!C::ARROW) __builtin_amdgcn_s_setprio(0);       // (raised at the top of the solver)
    float hw[C::NCHUNK], jaref[C::NCHUNK];
    {
      float vb[NVP<C>];
      vec_bcast<C>(s, lane_s, qacc, vb);
      jdot<C>(s, lane_s, nefc, nbase, rr, vb, jaref);
    }
#pragma unroll
    for (int ch = 0; ch < C::NCHUNK; ++ch) jaref[ch] -= rr[ch].aref;
    (void)rows_cost<C, false>(lane_s, nefc, jaref, rr, force, hw);
    qfc = jt_force<C>(s, lane_s, nefc, nbase, force);      // leaves the contact rows' forces in rw[rcon .. nefc)
  });
  const int nefc = f.nefc;
  WSYNC();
  const ConLayout CL = con_layout(C::NV, C::NEFC, C::NCON);
  float* o = d.out + (size_t)e * CL.stride;
  if (lane < C::NV) { o[CL.qfc + lane] = qfc; o[CL.qacc + lane] = f.qacc; }
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) {
    const int r = lane + 64 * ch;
    if (r < C::NEFC) o[CL.force + r] = r < nefc ? force[ch] : 0.0f;
  }
  const int nc = s.ncon, rcon = nefc - C::NPYR * nc;
  if (lane == 0) {
    o[CL.counts] = (float)nefc; o[CL.counts + 1] = (float)C::NEQ; o[CL.counts + 2] = (float)C::NF; o[CL.counts + 3] = (float)s.nlim_act;
    o[CL.ncon] = (float)nc;
  }
  // one lane per contact slot: the slot as store_side writes it, and the wrench from the slot's pyramid rows
  for (int c = lane; c < C::NCON; c += 64) {
    float* w = o + CL.con + 9 * c;
    const bool on = c < nc;
    const int pr = on ? s.cpair[c] : 0;
    w[0] = on ? s.cdist[c] : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { w[1 + k] = on ? s.cpos[3 * c + k] : 0.0f; w[4 + k] = on ? s.cnrm[3 * c + k] : 0.0f; }
    w[7] = on ? (float)m.pair_geom1[pr] : -1.0f; w[8] = on ? (float)m.pair_geom2[pr] : -1.0f;
    // mj_contactForce in the contact frame: normal = sum of the edges, direction k = mu_k (f_k+ - f_k-), folded as jt_force folds
    // them; then to the world frame with the frame the rows were built on (make_constraint)
    float fn = 0.0f;
    V3 fw = v3(0, 0, 0), tw = v3(0, 0, 0);
    if (on) {
      const int r0 = rcon + C::NPYR * c, b0 = rcon + C::NBC * c;
#pragma unroll
      for (int ed = 0; ed < C::NPYR; ed += 2) fn += s.rw[r0 + ed] + s.rw[r0 + ed + 1];
      float ft[C::NBC - 1];
#pragma unroll
      for (int k = 1; k < C::NBC; ++k) ft[k - 1] = s.bmu[b0 + k] * (s.rw[r0 + 2 * (k - 1)] - s.rw[r0 + 2 * (k - 1) + 1]);
      V3 nn, t1, t2;
      make_frame(ld3(&s.cnrm[3 * c]), nn, t1, t2);
      if constexpr (C::CAPS) {
        const V3 b = ld3(&s.ctan[3 * c]);
        if (b.x != 0.0f || b.y != 0.0f || b.z != 0.0f) { nn = ld3(&s.cnrm[3 * c]); t1 = b; t2 = cross(nn, b); }
      }
      fw = nn * fn + t1 * ft[0] + t2 * ft[1];
      if constexpr (C::NBC > 3) tw = nn * ft[2];
    }
    float* q = o + CL.wrench + 7 * c;
    q[0] = fn; q[1] = fw.x; q[2] = fw.y; q[3] = fw.z; q[4] = tw.x; q[5] = tw.y; q[6] = tw.z;
  }
}

}  // namespace rsr
