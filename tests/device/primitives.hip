// primitives.hip -- TEST ONLY: one-wave kernels around the in-register L D L^T layouts, the wave sums and the reciprocals of
// rsr_device.hpp, for tests/test_device_primitives*.py (loader: tests/device_harness.py).  Nothing here decodes a layout: the
// factor kernels copy a natural-order matrix into LDS, call the product's factor / solve exactly as rsr_solver.hpp does and
// dump the raw registers of all 64 lanes.  Built into tests/device/_build/, never into the product library.
#include <hip/hip_runtime.h>

#include "../../rsr_mjx_amd/csrc/rsr_env.hpp"

namespace {
using namespace rsr;

enum { K_NATURAL = 0, K_ROWCHOL = 1, K_ROWTREE = 2, K_ARROW = 3 };
enum { D_CUBE = 0, D_TSHAPE = 1, D_GO2FLAT = 2, D_GO2 = 3, D_HAND = 4, D_COUNT = 5 };
enum { M_MASS_ONLY = 1, M_HAS_DIAG = 2 };      // bits of `mode`

// floats of the transpose scratch each layout documents
template <class C, int KIND> constexpr int scratch_floats() {
  return KIND == K_NATURAL ? C::NV * C::LD : KIND == K_ROWCHOL ? C::NCH * 22 : KIND == K_ROWTREE ? 3 * C::NCT * C::NCT : 4 * 81;
}

struct FactorArgs {
  const float *H, *diag, *b;      // [n][NV][LD] (padding word included), [n][NV], [n][NV]
  int alias;                      // 1: the matrix itself is the scratch T (hessian_factor), 0: a scratch of its own
  float *a, *lt, *dinv, *x;       // [n][64][NREG] x 2, [n][64] x 2
};

template <class C, int KIND, bool MASS_ONLY, bool HAS_DIAG>
__global__ __launch_bounds__(64) void factor_kernel(FactorArgs g) {
  constexpr int NV = C::NV, LD = C::LD, NREG = KIND == K_NATURAL ? NV : C::NCH;
  constexpr int NSCR = scratch_floats<C, KIND>();
  // aliased, the matrix's storage must hold the scratch as well (the product's scratch_b() regions do); the words past the
  // matrix and the whole separate scratch start as NaN: no layout may read a scratch word it has not written
  constexpr int NMAT = NV * LD > NSCR ? NV * LD : NSCR;
  __shared__ float Hs[NMAT];
  __shared__ float Ts[NSCR];
  const int lane = threadIdx.x, e = blockIdx.x;
  const float qnan = __builtin_nanf("");
  for (int t = lane; t < NMAT; t += 64) Hs[t] = t < NV * LD ? g.H[(size_t)e * NV * LD + t] : qnan;
  for (int t = lane; t < NSCR; t += 64) Ts[t] = qnan;
  WSYNC();
  float* T = g.alias ? Hs : Ts;
  const float bl = lane < NV ? g.b[e * NV + lane] : 0.0f;
  float a[NREG], lt[NREG], dinv, x;
  if constexpr (KIND == K_NATURAL) {
    const float* row = &Hs[(lane < NV ? lane : 0) * LD];      // as hessian_factor: unmasked, lanes >= NV read row 0
    const float dd = (HAS_DIAG && lane < NV) ? g.diag[e * NV + lane] : 0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] = HAS_DIAG ? row[j] + (j == lane ? dd : 0.0f) : row[j];
    WSYNC();
    dinv = chol_factor<C, MASS_ONLY>(a, lt, T, lane);
    x = lane < NV ? chol_solve<C>(a, lt, dinv, bl, lane) : 0.0f;
  } else if constexpr (KIND == K_ROWCHOL) {
    const int dl = rowchol_dof<C>(lane);
    const float dd = (HAS_DIAG && dl >= 0) ? g.diag[e * NV + dl] : 0.0f;
    dinv = rowchol_factor<C, MASS_ONLY, HAS_DIAG>(Hs, dd, a, lt, T, lane);
    x = rowchol_solve<C>(a, lt, dinv, bl, lane);
  } else if constexpr (KIND == K_ROWTREE) {
    const int dl = rowtree_dof<C>(lane);
    const float dd = (HAS_DIAG && dl >= 0) ? g.diag[e * NV + dl] : 0.0f;
    dinv = rowtree_factor<C, HAS_DIAG>(Hs, dd, a, lt, T, lane);
    x = rowtree_solve<C>(a, lt, dinv, bl, lane);
  } else {
    const int dl = arrow_dof<C>(lane);
    const float dd = (HAS_DIAG && dl >= 0) ? g.diag[e * NV + dl] : 0.0f;
    dinv = arrow_factor<C, HAS_DIAG>(Hs, dd, a, lt, T, lane);
    x = arrow_solve<C>(a, lt, dinv, bl, lane);
  }
  const size_t o = (size_t)e * 64 + lane;
#pragma unroll
  for (int c = 0; c < NREG; ++c) { g.a[o * NREG + c] = a[c]; g.lt[o * NREG + c] = lt[c]; }
  g.dinv[o] = dinv; g.x[o] = x;
}

template <class C, int KIND, bool MASS_ONLY, bool HAS_DIAG>
int launch_factor(int n, const FactorArgs& g) {
  hipLaunchKernelGGL((factor_kernel<C, KIND, MASS_ONLY, HAS_DIAG>), dim3(n), dim3(64), 0, 0, g);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return (int)err;
}

// the template arguments the product instantiates (rsr_solver.hpp: hessian_factor, forward, integrate); the natural order is
// the bit reference and takes every combination
constexpr bool supported(int kind, bool rowchol, bool rowtree, bool arrow, int mode) {
  return kind == K_NATURAL ? (mode >= 0 && mode <= 3)
       : kind == K_ROWCHOL ? (rowchol && (mode == 0 || mode == M_MASS_ONLY || mode == (M_MASS_ONLY | M_HAS_DIAG)))
       : kind == K_ROWTREE ? (rowtree && (mode == 0 || mode == M_HAS_DIAG))
       : kind == K_ARROW ? (arrow && (mode == 0 || mode == M_HAS_DIAG)) : false;
}
template <class C> constexpr bool supported(int kind, int mode) { return supported(kind, C::ROWCHOL, C::ROWTREE, C::ARROW, mode); }

template <class C, int KIND, int MODE>
int factor_mode(int n, const FactorArgs& g) {
  if constexpr (supported<C>(KIND, MODE)) return launch_factor<C, KIND, (MODE & M_MASS_ONLY) != 0, (MODE & M_HAS_DIAG) != 0>(n, g);
  else return -1;
}
template <class C, int KIND>
int factor_kind(int mode, int n, const FactorArgs& g) {
  switch (mode) {
    case 0: return factor_mode<C, KIND, 0>(n, g);
    case 1: return factor_mode<C, KIND, 1>(n, g);
    case 2: return factor_mode<C, KIND, 2>(n, g);
    case 3: return factor_mode<C, KIND, 3>(n, g);
    default: return -1;
  }
}
template <class C>
int factor_dims(int kind, int mode, int n, const FactorArgs& g) {
  switch (kind) {
    case K_NATURAL: return factor_kind<C, K_NATURAL>(mode, n, g);
    case K_ROWCHOL: return factor_kind<C, K_ROWCHOL>(mode, n, g);
    case K_ROWTREE: return factor_kind<C, K_ROWTREE>(mode, n, g);
    case K_ARROW: return factor_kind<C, K_ARROW>(mode, n, g);
    default: return -1;
  }
}

// the device's own lane <-> dof maps: dof_of_lane[64], lane_of_dof[NV]
template <class C, int KIND>
__global__ __launch_bounds__(64) void lane_map_kernel(int* dof_of_lane, int* lane_of_dof) {
  const int lane = threadIdx.x, d = lane < C::NV ? lane : 0;
  int dof, ln;
  if constexpr (KIND == K_ROWCHOL) { dof = rowchol_dof<C>(lane); ln = rowchol_lane<C>(d); }
  else if constexpr (KIND == K_ROWTREE) { dof = rowtree_dof<C>(lane); ln = rowtree_lane<C>(d); }
  else if constexpr (KIND == K_ARROW) { dof = arrow_dof<C>(lane); ln = arrow_lane<C>(d); }
  else { dof = lane < C::NV ? lane : -1; ln = d; }
  dof_of_lane[lane] = dof;
  if (lane < C::NV) lane_of_dof[lane] = ln;
}
template <class C, int KIND>
int lane_map_kind(int* dof_of_lane, int* lane_of_dof) {
  if constexpr (supported<C>(KIND, 0)) {
    hipLaunchKernelGGL((lane_map_kernel<C, KIND>), dim3(1), dim3(64), 0, 0, dof_of_lane, lane_of_dof);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return (int)err;
  } else return -1;
}
template <class C>
int lane_map_dims(int kind, int* dof_of_lane, int* lane_of_dof) {
  switch (kind) {
    case K_NATURAL: return lane_map_kind<C, K_NATURAL>(dof_of_lane, lane_of_dof);
    case K_ROWCHOL: return lane_map_kind<C, K_ROWCHOL>(dof_of_lane, lane_of_dof);
    case K_ROWTREE: return lane_map_kind<C, K_ROWTREE>(dof_of_lane, lane_of_dof);
    case K_ARROW: return lane_map_kind<C, K_ARROW>(dof_of_lane, lane_of_dof);
    default: return -1;
  }
}

// v: [n][3][64].  ws / rs: wave_sum / row_sum16 of each of the three vectors on its own; ws3: wave_sum3 of the three together
__global__ __launch_bounds__(64) void sums_kernel(const float* v, float* ws, float* rs, float* ws3) {
  const int lane = threadIdx.x;
  const size_t o = (size_t)blockIdx.x * 3 * 64 + lane;
  const float v0 = v[o], v1 = v[o + 64], v2 = v[o + 128];
  ws[o] = wave_sum(v0); ws[o + 64] = wave_sum(v1); ws[o + 128] = wave_sum(v2);
  rs[o] = row_sum16(v0); rs[o + 64] = row_sum16(v1); rs[o + 128] = row_sum16(v2);
  float a = v0, b = v1, c = v2;
  wave_sum3(a, b, c);
  ws3[o] = a; ws3[o + 64] = b; ws3[o + 128] = c;
}

__global__ __launch_bounds__(64) void recips_kernel(int n, const float* x, float* rcp, float* rsq, float* sq) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) { const float v = x[i]; rcp[i] = frcp(v); rsq[i] = frsq(v); sq[i] = fsqrt(v); }
}

template <class C> void fill_dims(int* out) {
  const int v[16] = {C::NV, C::NCH, C::LD, C::ISO0, C::ISO1, C::TREE1, C::TREE2, C::NCT, C::ANT, C::ALEGN,
                     C::ALEGS, C::NA, C::NISO, C::ROWCHOL, C::ROWTREE, C::ARROW};
  for (int i = 0; i < 16; ++i) out[i] = v[i];
}
}  // namespace

#define RSR_PRIM_DISPATCH(dims, call, otherwise)                   \
  switch (dims) {                                                   \
    case D_CUBE: { using C = rsr::CubeDims; call; }                 \
    case D_TSHAPE: { using C = rsr::TShapeDims; call; }             \
    case D_GO2FLAT: { using C = rsr::Go2FlatDims; call; }           \
    case D_GO2: { using C = rsr::Go2Dims; call; }                   \
    case D_HAND: { using C = rsr::HandDims; call; }                 \
    default: otherwise;                                             \
  }

extern "C" {

// out[16] = NV, NCH, LD, ISO0, ISO1, TREE1, TREE2, NCT, ANT, ALEGN, ALEGS, NA, NISO, ROWCHOL, ROWTREE, ARROW of Dims `dims`
int rsr_prim_dims(int dims, int* out) {
  RSR_PRIM_DISPATCH(dims, fill_dims<C>(out); return 0, return -1)
}

// 1 when (kind, dims, mode) is a combination the product instantiates (natural order: always), else 0
int rsr_prim_supported(int kind, int dims, int mode) {
  RSR_PRIM_DISPATCH(dims, return supported<C>(kind, mode) ? 1 : 0, return 0)
}

// float registers a lane dumps per array for (kind, dims): NV in natural order, NCH otherwise; -1 = no such Dims
int rsr_prim_nreg(int kind, int dims) {
  RSR_PRIM_DISPATCH(dims, return kind == K_NATURAL ? C::NV : C::NCH, return -1)
}

// factor + solve of n matrices, one wave each.  Device pointers; returns 0, a hipError_t, or -1 for an unsupported combination.
int rsr_prim_factor(int kind, int dims, int mode, int n, const float* H, const float* diag, const float* b, int alias,
                    float* a, float* lt, float* dinv, float* x) {
  if (n <= 0) return -1;
  const FactorArgs g{H, diag, b, alias, a, lt, dinv, x};
  RSR_PRIM_DISPATCH(dims, return factor_dims<C>(kind, mode, n, g), return -1)
}

int rsr_prim_lane_map(int kind, int dims, int* dof_of_lane, int* lane_of_dof) {
  RSR_PRIM_DISPATCH(dims, return lane_map_dims<C>(kind, dof_of_lane, lane_of_dof), return -1)
}

int rsr_prim_sums(int n, const float* v, float* ws, float* rs, float* ws3) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(sums_kernel, dim3(n), dim3(64), 0, 0, v, ws, rs, ws3);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return (int)err;
}

int rsr_prim_recips(int n, const float* x, float* rcp, float* rsq, float* sq) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(recips_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, x, rcp, rsq, sq);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return (int)err;
}

}  // extern "C"
