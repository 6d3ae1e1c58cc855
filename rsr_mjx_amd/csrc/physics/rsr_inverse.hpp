// rsr_inverse.hpp -- rsr_physics_inverse (include/rsr_physics.h): mj_inverse at the record's current state and a caller-given
// acceleration, written to the handle's inverse buffer (InvLayout, rsr_physics.hpp): the constraint row forces of MJX's
// _update_constraint at jaref = J a - aref, qfrc_constraint = J^T force, qfrc_actuator and
// qfrc_inverse = M a + qfrc_bias - qfrc_passive - qfrc_constraint.  Nothing but that buffer is written.
//
// The pass restates the stages of forward<C> (rsr_solver.hpp) up to the rows' final aref, as dynamics_kernel restates its first
// three: kinematics, com_crb_mass, smooth_forces, collision, make_constraint, aref -= b (J qvel).  The factorisation of M for
// qacc_smooth and the Newton solve are left out; forward<C> itself is not touched (a trait on its rows tail would state the pass
// once, and would move the hash of the env kernels' sources: an edit to forward<C>'s stage order needs its mirror here).  The
// tail is the one of constraint_kernel (rsr_constraint.hpp) at the given acceleration instead of the solver's.  The handle's
// applied forces are not read: the rows do not depend on them, and qfrc_inverse is what they would have to sum to.
//
// What the tail finds in LDS with no solver before it: make_constraint zeroes the null words bval[NBASE ..] and the null row of J
// and sets bmu / sdof for every row it makes; the J.qvel before it has already run jdot on that state.  jdot writes bval[0 .. nbase)
// before it reads bval[bn], bval[bk] (both < nbase, or the null word for the rows >= nefc); jt_force writes rw[rcon .. nefc), dgw,
// bval[rcon .. nbase) and every word of jtp before it reads them; vec_bcast's buffer, the head of rw, holds the contact tangents
// of make_constraint, dead since the base rows were filled.  M is intact (nothing before the Hessian reuses it, Dims::TALIAS
// included), so Dims::MROW_LDS models reload their row from it.
#pragma once
#include "../rsr_launch.hpp"

namespace rsr {

// RSR_INV_DISCRETE: where integrate<C> solves (M + h D) qacc' = M qacc (implicit_integration), acc is that qacc' and becomes
// qacc = acc + h M^-1 (damp * acc) (mj_discreteAcc), with the factorisation of M that forward<C> takes for qacc_smooth.  Runs
// where that one runs, right after smooth_forces: the transposes' scratch (phase A's dead arrays) is free there and not after the
// rows are built.
template <class C>
__device__ __forceinline__ float discrete_acc(const Hot& h, Smem<C>& s, int lane, float (&Mrow)[C::NV], float acc) {
  if (!implicit_integration<C>(h, s, lane)) return acc;               // (wave-uniform)
  const float rhs = lane < C::NV ? h.timestep * s.damp[lane] * acc : 0.0f;
  float a[C::NCH], lt[C::NCH], x;
  WSYNC();
  if constexpr (C::ROWTREE) {
    const float dinv_m = rowtree_factor<C>(s.M, 0.0f, a, lt, s.scratch_a(), lane);
    x = rowtree_solve<C>(a, lt, dinv_m, rhs, lane);
  } else if constexpr (C::ROWCHOL) {
    const float dinv_m = rowchol_factor<C, true>(s.M, 0.0f, a, lt, s.scratch_a(), lane);
    x = rowchol_solve<C>(a, lt, dinv_m, rhs, lane);
  } else if constexpr (C::ARROW) {
    const float dinv_m = arrow_factor<C>(s.M, 0.0f, a, lt, s.scratch_a(), lane);
    x = arrow_solve<C>(a, lt, dinv_m, rhs, lane);
  } else {
    if constexpr (C::MROW_LDS) load_mrow<C>(s, lane, Mrow);
#pragma unroll
    for (int j = 0; j < C::NV; ++j) a[j] = Mrow[j];
    const float dinv_m = chol_factor<C, true>(a, lt, s.scratch_a(), lane);
    x = chol_solve<C>(a, lt, dinv_m, rhs, lane);
  }
  WSYNC();
  return lane < C::NV ? acc + x : 0.0f;
}

// One wave per env, a plain launch.  v.ids: the envs to run or null (env = workgroup index); an id out of range runs nothing.
// v.qacc: [N][nv], row e is env e's whether or not ids is given.  v.out: the inverse buffer.
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void inverse_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, InvArgs v) {
  const DModel& m = *mp;
  const Hot hot = make_hot(m);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int e = v.ids ? v.ids[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  if (e < 0 || e >= a.n) return;
  const float* rec = a.state + (size_t)e * L.rec;
  PROF_DECL
  // the record load of constraint_kernel (the warm start has no reader)
  for (int t = lane; t < C::NQ; t += 64) s.qpos[t] = rec[L.qpos + t];
  float acc = 0.0f;
  if (lane < C::NV) { s.qvel[lane] = rec[L.qvel + lane]; acc = v.qacc[(size_t)e * C::NV + lane]; }
  load_overrides<C>(m, s, a, e, lane);
  if (lane < C::NU) s.ctrl[lane] = rec[L.ctrl + lane];
  if constexpr (C::XFRC) {        // the Go2 single-body kick path idle, as in the physics kernels
    if (lane == 0) { s.acc_body = m.site_bodyid[m.env_ids[0]]; s.xfrc_body = 0; s.xfrc[0] = s.xfrc[1] = s.xfrc[2] = 0.0f; }
  }
  WSYNC();
  const int lane_s = lrec_lane(lane);
  float Mrow[C::NV], force[C::NCHUNK];
  // forward<C>'s stages up to the rows' final aref
  kinematics<C>(m, hot, s, lane_s PROF_PASS);
  com_crb_mass<C>(m, hot, s, lane_s PROF_PASS);
  load_mrow<C>(s, lane_s, Mrow);
  const float qvel_i = lane_s < C::NV ? s.qvel[lane_s] : 0.0f;
  const float fs = smooth_forces<C>(m, hot, s, lane_s, qvel_i, 0.0f PROF_PASS);
  if (v.flags & RSR_INV_DISCRETE) acc = discrete_acc<C>(hot, s, lane_s, Mrow, acc);
  collision<C>(m, hot, s, lane_s PROF_PASS);
  RowRegs rr[C::NCHUNK];
  float bcoef[C::NCHUNK], jqv[C::NCHUNK];
  int nbase;
  const int nefc = make_constraint<C>(m, hot, s, lane_s, rr, bcoef, nbase PROF_PASS);
  {
    float qb[NVP<C>];
    vec_bcast<C>(s, lane_s, qvel_i, qb);
    jdot<C>(s, lane_s, nefc, nbase, rr, qb, jqv);                   // aref = -b (J.qvel) - k imp pos
  }
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) rr[ch].aref -= bcoef[ch] * jqv[ch];
  // constraint_kernel's rows tail at acc; M acc from the same broadcast
  float hw[C::NCHUNK], jaref[C::NCHUNK], Ma;
  {
    float vb[NVP<C>];
    vec_bcast<C>(s, lane_s, acc, vb);
    if constexpr (C::MROW_LDS) load_mrow<C>(s, lane_s, Mrow);
    Ma = lane_s < C::NV ? row_dot<C>(Mrow, vb) : 0.0f;
    jdot<C>(s, lane_s, nefc, nbase, rr, vb, jaref);
  }
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) jaref[ch] -= rr[ch].aref;
  (void)rows_cost<C, false>(lane_s, nefc, jaref, rr, force, hw);
  const float qfc = jt_force<C>(s, lane_s, nefc, nbase, force);      // leaves the contact rows' forces in rw[rcon .. nefc)
  WSYNC();
  const InvLayout IL = inv_layout(C::NV, C::NEFC);
  float* o = v.out + (size_t)e * IL.stride;
  if (lane < C::NV) {
    // qfrc_actuator: dynamics_kernel's expression (gear * actuator_force, then the joint's actfrcrange)
    const int4 rd_act = lrec<C>(hot, LQ_D_ACT, lane_s), rd_frc = lrec<C>(hot, LQ_D_FRC, lane_s);
    float act = 0;
    const int u = rd_act.x;
    if (u >= 0) act = asf(rd_act.y) * s.aforce[u];
    if (rd_frc.y) act = clampf(act, asf(rd_frc.z), asf(rd_frc.w));
    // M a + qfrc_bias - qfrc_passive - qfrc_constraint, with qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator (the bias
    // scratch is dead by now)
    o[IL.qfi + lane] = Ma - fs + act - qfc;
    o[IL.qfc + lane] = qfc; o[IL.qacc + lane] = acc; o[IL.act + lane] = act;
  }
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) {
    const int r = lane + 64 * ch;
    if (r < C::NEFC) o[IL.force + r] = r < nefc ? force[ch] : 0.0f;
  }
  if (lane == 0) {
    o[IL.counts] = (float)nefc; o[IL.counts + 1] = (float)C::NEQ; o[IL.counts + 2] = (float)C::NF; o[IL.counts + 3] = (float)s.nlim_act;
  }
}

}  // namespace rsr
