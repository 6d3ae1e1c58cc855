// solver_rows.hip -- TEST ONLY: one-wave kernels around the leaf functions of the Newton solver (rsr_solver.hpp): the row costs
// (rows_cost), the line search's 1-D model (ls_prepare, ls_point, ls_eval<3>, ls_costs) and the two Jacobian products (jdot,
// jt_force), for tests/test_solver_rows*.py (loader: tests/device_harness.py).  One wave runs one problem; nothing here decodes or
// restates the functions: the kernels load per-lane registers from global arrays laid out [n][NCHUNK][64] (row = lane + 64 * chunk),
// call the product's functions as solve() does and dump what they return.  Built into tests/device/_build/, never into the product
// library.
//
// What the two Jacobian products read of the LDS image (Smem<C>), and what make_constraint (rsr_device.hpp) guarantees about it.
// With rcon = nefc - NPYR * ncon (first contact row: pyramid and base numbering agree below it) and nbase = rcon + NBC * ncon:
//   jdot      J[b * LDJ .. + NV) of the base rows b < nbase (the LDJ - NV padding columns are loaded and never used); in a chunk of
//             base rows that is partly live the lanes b >= nbase load the null row NBASE and discard the product.  It WRITES
//             bval[0 .. nbase) and then reads bval[bn], bval[bk] of the lane's rows in every chunk with 64 * ch < nefc: for the rows
//             >= nefc that is bval[NBASE] (bn = bk = NBASE, mu = 0 -- make_constraint's padding), which must be 0.
//   vec_bcast writes rw[0 .. NVP) and reads it back.
//   jt_force  ncon; WRITES rw[rcon .. nefc), dgw[0 .. NV), bval[rcon .. nbase) and every word of jtp before it reads them; reads
//             sdof[r] and J[r * LDJ + sdof[r]] of the friction / limit rows NEQ <= r < rcon whose force is not zero, the whole
//             rows J[r * LDJ .. + NV) of the equality rows r < NEQ and of the contact base rows rcon <= b < nbase, bmu[b] of the
//             contact base rows that are not a normal (b - rcon not a multiple of NBC), and -- the tail of the quartet walk --
//             J[NBASE * LDJ .. + NV) and bval[NBASE], whose product must be 0: make_constraint zeroes the null row and
//             bval[NBASE .. NBASE + 4).
// Neither function reads: the base rows nbase <= b < NBASE, the columns >= NV of any row, bmu outside the contact tangents, the
// words of bval, rw, dgw, jtp it has not written, wc.  The harness (device_harness.jproducts) fills the words named above and sets
// everything else of J / bmu / bval and all of rw / jtp / wc / dgw to a poison value (NaN by default), so that a read outside the
// contract shows in the result.
#include <hip/hip_runtime.h>

#include "../../rsr_mjx_amd/csrc/rsr_env.hpp"

namespace {
using namespace rsr;

enum { D_CUBE = 0, D_TSHAPE = 1, D_GO2FLAT = 2, D_GO2 = 3, D_HAND = 4 };

// per-lane inputs, [n][NCHUNK][64] each; a null field keeps make_constraint's padding value.  nefc: [n]
struct Rows {
  const int* nefc;
  const float *jaref, *jv, *D, *R, *floss, *mu;
  const int *bn, *bk;
};

template <class C>
__device__ __forceinline__ void load_rows(const Rows& g, int e, int lane, RowRegs (&rr)[C::NCHUNK], float (&jaref)[C::NCHUNK],
                                          float (&jv)[C::NCHUNK]) {
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) {
    const size_t o = ((size_t)e * C::NCHUNK + ch) * 64 + lane;
    RowRegs r{0.0f, 0.0f, 1.0f, -1.0f, 0.0f, C::NBASE, C::NBASE};
    if (g.D) r.D = g.D[o];
    if (g.R) r.R = g.R[o];
    if (g.floss) r.floss = g.floss[o];
    if (g.mu) r.mu = g.mu[o];
    if (g.bn) r.bn = g.bn[o];
    if (g.bk) r.bk = g.bk[o];
    rr[ch] = r;
    jaref[ch] = g.jaref ? g.jaref[o] : 0.0f;
    jv[ch] = g.jv ? g.jv[o] : 0.0f;
  }
}

// cost: [n][64] (rows_cost<C, true>: the same in every lane), cost_lane: [n][64] (rows_cost<C, false>), force / hw:
// [n][2][NCHUNK][64] (of the two calls)
struct CostOut { float *cost, *cost_lane, *force, *hw; };

template <class C>
__global__ __launch_bounds__(64) void rows_cost_kernel(Rows g, CostOut o) {
  const int lane = threadIdx.x, e = blockIdx.x, nefc = uniform_i(g.nefc[e]);
  RowRegs rr[C::NCHUNK];
  float jaref[C::NCHUNK], jv[C::NCHUNK], f0[C::NCHUNK], h0[C::NCHUNK], f1[C::NCHUNK], h1[C::NCHUNK];
  load_rows<C>(g, e, lane, rr, jaref, jv);
  const float c = rows_cost<C, true>(lane, nefc, jaref, rr, f0, h0);
  const float cl = rows_cost<C, false>(lane, nefc, jaref, rr, f1, h1);
  o.cost[(size_t)e * 64 + lane] = c;
  o.cost_lane[(size_t)e * 64 + lane] = cl;
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) {
    const size_t a = (((size_t)e * 2 + 0) * C::NCHUNK + ch) * 64 + lane, b = (((size_t)e * 2 + 1) * C::NCHUNK + ch) * 64 + lane;
    o.force[a] = f0[ch]; o.hw[a] = h0[ch];
    o.force[b] = f1[ch]; o.hw[b] = h1[ch];
  }
}

// g: [n][3] (g0, g1, g2), alpha: [n][3].  pt / ev: [n][3][4] = (q1, q2, d0(), d1()) of ls_point at each alpha / of ls_eval<C, 3>
// at the three together; cost: [n][2][3] = ls_costs on ls_point's three points, on ls_eval's
struct LsArgs { const float *g, *alpha; float *pt, *ev, *cost; };

__device__ __forceinline__ void dump_point(float* o, const LSPoint& p) { o[0] = p.q1; o[1] = p.q2; o[2] = p.d0(); o[3] = p.d1(); }

template <class C>
__global__ __launch_bounds__(64) void linesearch_kernel(Rows g, LsArgs a) {
  const int lane = threadIdx.x, e = blockIdx.x, nefc = uniform_i(g.nefc[e]);
  RowRegs rr[C::NCHUNK];
  float jaref[C::NCHUNK], jv[C::NCHUNK];
  load_rows<C>(g, e, lane, rr, jaref, jv);
  const float g0 = a.g[3 * e], g1 = a.g[3 * e + 1], g2 = a.g[3 * e + 2];
  const float al[3] = {a.alpha[3 * e], a.alpha[3 * e + 1], a.alpha[3 * e + 2]};
  LSRows<C> lw;
  ls_prepare<C>(lane, nefc, jaref, jv, rr, lw);
  LSPoint p[3], q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = ls_point<C>(nefc, al[k], lw, g1, g2);
  ls_eval<C, 3>(nefc, al, lw, g1, g2, q);
  float cp[3], cq[3];
  ls_costs<C>(nefc, lw, g0, p[0], p[1], p[2], cp[0], cp[1], cp[2]);
  ls_costs<C>(nefc, lw, g0, q[0], q[1], q[2], cq[0], cq[1], cq[2]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dump_point(&a.pt[((size_t)e * 3 + k) * 4], p[k]);
      dump_point(&a.ev[((size_t)e * 3 + k) * 4], q[k]);
      a.cost[(size_t)e * 6 + k] = cp[k]; a.cost[(size_t)e * 6 + 3 + k] = cq[k];
    }
  }
}

// LDS images as the harness built them: J [n][(NBASE + 1) * LDJ], bmu / bval [n][NBASE + 4], sdof [n][NSP + 1], ncon [n];
// poison: the value of every word of rw, jtp, wc and dgw.  v: [n][NV] (the dof vector of jdot), force: [n][NCHUNK][64].
// jd: [n][NCHUNK][64] (jdot's out), qfc: [n][64] (jt_force's return value)
struct JArgs {
  const float *J, *bmu, *bval;
  const int *sdof, *ncon;
  float poison;
  const float *v, *force;
  float *jd, *qfc;
};

template <class C>
__global__ __launch_bounds__(64) void jproducts_kernel(Rows g, JArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Smem<C>& s = *reinterpret_cast<Smem<C>*>(smem_raw);
  const int lane = threadIdx.x, e = blockIdx.x, nefc = uniform_i(g.nefc[e]), ncon = uniform_i(a.ncon[e]);
  constexpr int NJ = (C::NBASE + 1) * C::LDJ, NJTP = C::NBC * C::NCON > 16 ? 64 : 1;
  for (int t = lane; t < NJ; t += 64) s.x.b.J[t] = a.J[(size_t)e * NJ + t];
  for (int t = lane; t < C::NBASE + 4; t += 64) { s.bmu[t] = a.bmu[(size_t)e * (C::NBASE + 4) + t]; s.bval[t] = a.bval[(size_t)e * (C::NBASE + 4) + t]; }
  for (int t = lane; t < C::NSP + 1; t += 64) s.sdof[t] = a.sdof[(size_t)e * (C::NSP + 1) + t];
  for (int t = lane; t < C::NEFC + 4; t += 64) s.rw[t] = a.poison;
  for (int t = lane; t < C::NCON * 8; t += 64) s.wc[t] = a.poison;
  for (int t = lane; t < NJTP; t += 64) s.jtp[t] = a.poison;
  if (lane < C::NV) s.dgw[lane] = a.poison;
  if (lane == 0) s.ncon = ncon;
  WSYNC();
  const int nbase = nefc - C::NPYR * ncon + C::NBC * ncon;
  RowRegs rr[C::NCHUNK];
  float jaref[C::NCHUNK], jv[C::NCHUNK], out[C::NCHUNK], force[C::NCHUNK];
  load_rows<C>(g, e, lane, rr, jaref, jv);
  {
    float vb[NVP<C>];
    vec_bcast<C>(s, lane, lane < C::NV ? a.v[(size_t)e * C::NV + lane] : 0.0f, vb);
    jdot<C>(s, lane, nefc, nbase, rr, vb, out);
  }
#pragma unroll
  for (int ch = 0; ch < C::NCHUNK; ++ch) {
    const size_t o = ((size_t)e * C::NCHUNK + ch) * 64 + lane;
    a.jd[o] = out[ch];
    force[ch] = a.force[o];
  }
  a.qfc[(size_t)e * 64 + lane] = jt_force<C>(s, lane, nefc, nbase, force);
}

int finish() {
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return (int)err;
}
template <class C> int launch_rows_cost(int n, const Rows& g, const CostOut& o) {
  hipLaunchKernelGGL(rows_cost_kernel<C>, dim3(n), dim3(64), 0, 0, g, o);
  return finish();
}
template <class C> int launch_linesearch(int n, const Rows& g, const LsArgs& a) {
  hipLaunchKernelGGL(linesearch_kernel<C>, dim3(n), dim3(64), 0, 0, g, a);
  return finish();
}
template <class C> int launch_jproducts(int n, const Rows& g, const JArgs& a) {
  static_assert(sizeof(Smem<C>) <= 65536, "the LDS image fits a plain dynamic-LDS launch, as in the product");
  hipLaunchKernelGGL(jproducts_kernel<C>, dim3(n), dim3(64), sizeof(Smem<C>), 0, g, a);
  return finish();
}

template <class C> void fill_dims(int* out) {
  const int v[11] = {C::NV, C::NEQ, C::NF, C::NL, C::NCON, C::NPYR, C::NBC, C::NEFC, C::NCHUNK, C::NBASE, C::LDJ};
  for (int i = 0; i < 11; ++i) out[i] = v[i];
}
}  // namespace

// (Go2Dims shares Go2FlatDims' row constants and every function here: not instantiated)
#define RSR_SR_DISPATCH(dims, call, otherwise)                      \
  switch (dims) {                                                   \
    case D_CUBE: { using C = rsr::CubeDims; call; }                 \
    case D_TSHAPE: { using C = rsr::TShapeDims; call; }             \
    case D_GO2FLAT: { using C = rsr::Go2FlatDims; call; }           \
    case D_HAND: { using C = rsr::HandDims; call; }                 \
    default: otherwise;                                             \
  }

extern "C" {

// out[11] = NV, NEQ, NF, NL, NCON, NPYR, NBC, NEFC, NCHUNK, NBASE, LDJ of Dims `dims` (host call)
int rsr_sr_dims(int dims, int* out) {
  RSR_SR_DISPATCH(dims, fill_dims<C>(out); return 0, return -1)
}

// Device pointers throughout; every call returns 0, a hipError_t, or -1 for no such Dims / n <= 0.
int rsr_sr_rows_cost(int dims, int n, const int* nefc, const float* jaref, const float* D, const float* R, const float* floss,
                     float* cost, float* cost_lane, float* force, float* hw) {
  if (n <= 0) return -1;
  const Rows g{nefc, jaref, nullptr, D, R, floss, nullptr, nullptr, nullptr};
  const CostOut o{cost, cost_lane, force, hw};
  RSR_SR_DISPATCH(dims, return launch_rows_cost<C>(n, g, o), return -1)
}

int rsr_sr_linesearch(int dims, int n, const int* nefc, const float* jaref, const float* jv, const float* D, const float* R,
                      const float* floss, const float* g012, const float* alpha, float* pt, float* ev, float* cost) {
  if (n <= 0) return -1;
  const Rows g{nefc, jaref, jv, D, R, floss, nullptr, nullptr, nullptr};
  const LsArgs a{g012, alpha, pt, ev, cost};
  RSR_SR_DISPATCH(dims, return launch_linesearch<C>(n, g, a), return -1)
}

int rsr_sr_jproducts(int dims, int n, const int* nefc, const int* ncon, const float* J, const float* bmu, const float* bval,
                     const int* sdof, float poison, const float* mu, const int* bn, const int* bk, const float* v,
                     const float* force, float* jd, float* qfc) {
  if (n <= 0) return -1;
  const Rows g{nefc, nullptr, nullptr, nullptr, nullptr, nullptr, mu, bn, bk};
  const JArgs a{J, bmu, bval, sdof, ncon, poison, v, force, jd, qfc};
  RSR_SR_DISPATCH(dims, return launch_jproducts<C>(n, g, a), return -1)
}

}  // extern "C"
