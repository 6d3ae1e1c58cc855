// rsr_kalman.hpp -- rsr_physics_kalman (include/rsr_physics.h): a linear time-varying Kalman filter and Rauch-Tung-Striebel smoother
// on the columns rsr_physics_trajectory_fd writes (A_t and the sensor Jacobian C_t), the dual of the Riccati pass of rsr_lqr.hpp.  One
// wave per slot runs all T filter steps and then, if asked, the T smoother steps in one launch.  The kernel reads neither the model
// nor the record: C gives NV and NU, i.e. static LDS offsets, loop bounds and register tiles, and the first three kernel arguments are
// there only because every physics op is sent by the one launch lambda.
//
// Layout.  nx = 2 NV.  Every matrix is NX rows of LD floats, LD the padded pitch of rsr_lqr.hpp (LD / 4 odd: lanes that read rows LD
// apart 16 bytes at a time hit different slots of the bank row).  F[j][i] = A_t[i][j] is a row of `columns` as it lies in memory;
// CS[r][j] = C_t[r][j] is the one transposed load (sensor entry r is a row, so an update reads its c_r four floats at a time).  All
// nx^2-sized products have the one form out[a][b] = sum_j X[j][a] Y[j][b] (prod): both operands are read along rows, a lane holds a
// 4 x (4 NB) register tile and adds ascending j.  A P A^T is prod(prod(P, F), F) because P is symmetric; the smoother's G D G^T is
// prod(GT, prod(D, GT)) with GT the transposed gain, which the solve writes as it goes.  The dots of two rows (row_dot_n) sum the
// indices i mod 4 apart and add the four at the end: the order is fixed, an output element is one lane's own sums, and the chain a
// lone wave has to wait out is a quarter as long.
//
// Measurement update.  R_t is diagonal, so the entries are taken one at a time, ascending: lane i owns row i of P, forms w_i =
// P[i] . c, every lane forms s = c . w + r and nu = dy - c . x from LDS (the same bits in every lane), and lane i writes x_i +=
// w_i (nu / s) and P[i][k] = fma(-(w_i w_k), 1 / s, P[i][k]): the product w_i w_k commutes, so P stays symmetric bit for bit.  An
// entry with r = +inf is skipped whole; nothing else depends on ny.  The predict symmetrises through a scratch matrix:
// P[i][k] = (S[i][k] + S[k][i]) / 2, + q_i on the diagonal.
//
// Smoother.  Pf[t] and xf[t] come back from global memory, where other lanes of this wave stored them earlier in the launch: the
// stores are drained (vmcnt(0)) between a workgroup-scope release and acquire before the first load.  Pm is the filter's own predict
// code on Pf[t], so the same bits.  Its Cholesky runs a column per trip, lane i forming L[i][j] from rows i and j of the factor so
// far (the factor is kept as L and as L^T, zeros elsewhere, so both triangular solves read rows); every lane forms the pivot.  Lane l
// then solves Pm g = (Pf A^T)[l] in its own row of LDS, no lane waiting for another.
#pragma once
#include "rsr_lqr.hpp"

namespace rsr {

template <class C>
struct KalmanDims {
  static constexpr int NX = 2 * C::NV, NCOL = NX + C::NU;
  static constexpr int IB = NX / 4;                          // tile columns: four indices each
  static constexpr int LD = LqrDims<C>::LD;                  // row pitch, LD / 4 odd
  static constexpr int GRP = 64 / IB;                        // lane groups of a product
  static constexpr int NB = (IB + GRP - 1) / GRP;            // 4-wide column blocks per lane: block g + n GRP
  static constexpr int NREG = (NX * NX + 63) / 64;
  static constexpr int MAT = NX * LD;
  // offsets, floats: the vectors, then what the filter uses (P its covariance, the smoother's Pf[t]; CS lies where the smoother's
  // matrices will), then the smoother's own.  A filter-only launch asks for the first FILTER_FLOATS alone.
  static constexpr int XV = 0, WV = XV + 64, DV = WV + 64, RV = DV + 64, YV = RV + 64, QV = YV + 64, DI = QV + 64, XS = DI + 64;
  static constexpr int P = XS + 64, F = P + MAT, W = F + MAT, S = W + MAT, PM = S + MAT, PS = PM + MAT, LF = PS + MAT, LT = LF + MAT, CS = PM;
  static constexpr int FILTER_FLOATS = CS + RSR_MAX_SENSORDATA * LD, FLOATS = LT + MAT;
  static_assert(NX % 4 == 0 && NX <= 64 && RSR_MAX_SENSORDATA <= 64, "one lane per state index and per sensor entry");
  static_assert(FILTER_FLOATS <= FLOATS, "C_t fits where the smoother's matrices will stand");
  static_assert(GRP * NB >= IB && GRP * IB <= 64, "every column block has a lane");
  static_assert(sizeof(float) * FLOATS <= 64 * 1024, "the image stays under what a plain launch may ask for");
};
// (smoothing: whether the launch's out->xs is given; the filter alone leaves room for twice the workgroups per CU)
template <class C>
constexpr size_t kalman_lds_bytes(bool smoothing) { return sizeof(float) * (smoothing ? KalmanDims<C>::FLOATS : KalmanDims<C>::FILTER_FLOATS); }

// sum over i < n (a multiple of 4) of a[i] b[i]: the indices i mod 4 summed apart, each ascending, then (s0 + s1) + (s2 + s3).
// Four short fma chains where row_dot has one long one: a wave alone on its SIMD waits out every dependent fma.
__device__ __forceinline__ void dot_step(f2 (&acc)[2], const float4& a, const float4& b) {
  acc[0] = pk_fma(f2{a.x, a.y}, f2{b.x, b.y}, acc[0]); acc[1] = pk_fma(f2{a.z, a.w}, f2{b.z, b.w}, acc[1]);
}
__device__ __forceinline__ float dot_sum(const f2 (&acc)[2]) { return (acc[0].x + acc[0].y) + (acc[1].x + acc[1].y); }
__device__ __forceinline__ float row_dot_n(const float* a, const float* b, int n) {
  f2 acc[2] = {f2{0.0f, 0.0f}, f2{0.0f, 0.0f}};
  for (int i = 0; i < n; i += 4) dot_step(acc, lds4(a + i), lds4(b + i));
  return dot_sum(acc);
}

// out[a][b] = sum_j X[j][a] Y[j][b], ascending j: lane (g, ib) holds rows 4 ib .. 4 ib + 3 of the column blocks g + n GRP
template <class D>
__device__ __forceinline__ void kalman_prod(const float* X, const float* Y, float* out, int lane) {
  constexpr int NX = D::NX, LD = D::LD, IB = D::IB, GRP = D::GRP, NB = D::NB;
  const int ib = lane % IB, g = lane / IB;
  if (g >= GRP) return;
  f2 acc[NB][4][2];
  int bb[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    bb[n] = g + n * GRP;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[n][r][0] = acc[n][r][1] = f2{0.0f, 0.0f};
  }
  for (int j = 0; j < NX; ++j) {
    const float4 x = lds4(X + j * LD + 4 * ib);
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const float4 y = lds4(Y + j * LD + 4 * (bb[n] < IB ? bb[n] : IB - 1));
      fma4(acc[n][0], x.x, y); fma4(acc[n][1], x.y, y); fma4(acc[n][2], x.z, y); fma4(acc[n][3], x.w, y);
    }
  }
#pragma unroll
  for (int n = 0; n < NB; ++n)
    if (bb[n] < IB)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4*>(out + (4 * ib + r) * LD + 4 * bb[n]) = make_float4(acc[n][r][0].x, acc[n][r][0].y, acc[n][r][1].x, acc[n][r][1].y);
}

// dst = A src A^T + diag(q), symmetrised (src symmetric; F, QV in LDS; W = src A^T stays): the filter's predict and the smoother's Pm
template <class D>
__device__ __forceinline__ void kalman_predict(float* sm, const float* src, float* dst, int lane) {
  constexpr int NX = D::NX, LD = D::LD;
  float *const F = sm + D::F, *const W = sm + D::W, *const S = sm + D::S, *const QV = sm + D::QV;
  kalman_prod<D>(src, F, W, lane);
  WSYNC();
  kalman_prod<D>(W, F, S, lane);
  WSYNC();
  for (int e = lane; e < NX * NX; e += 64) {
    const int i = e / NX, k = e - i * NX;
    const float v = 0.5f * (S[i * LD + k] + S[k * LD + i]);
    dst[i * LD + k] = i == k ? v + QV[i] : v;
  }
  WSYNC();
}

// Workgroup s: slot s.  WAVES: the family's waves per SIMD, an upper bound only (the LDS image admits fewer).
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WAVES)))
void kalman_kernel(const DModel* __restrict__, Layout, StepArgs, KalmanArgs q) {
  using D = KalmanDims<C>;
  constexpr int NX = D::NX, LD = D::LD, NREG = D::NREG;
  constexpr float LOG_2PI = 1.8378770664093453f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* const sm = reinterpret_cast<float*>(smem_raw);
  float *const P = sm + D::P, *const F = sm + D::F, *const W = sm + D::W, *const S = sm + D::S, *const PM = sm + D::PM, *const PS = sm + D::PS;
  float *const LF = sm + D::LF, *const LT = sm + D::LT, *const CS = sm + D::CS;
  float *const XV = sm + D::XV, *const WV = sm + D::WV, *const DV = sm + D::DV, *const RV = sm + D::RV, *const YV = sm + D::YV;
  float *const QV = sm + D::QV, *const DI = sm + D::DI, *const XS = sm + D::XS;
  const int lane = threadIdx.x, T = q.T, ny = q.ny;
  const size_t slot = blockIdx.x;
  const bool mine = lane < NX;                     // the lane of state index `lane`
  float* const prow = P + (mine ? lane : 0) * LD;

  auto load_step = [&](int t) {                    // A_t (rows of `columns`, row_stride apart) and q_t
    const float* src = q.columns + (slot * T + t) * D::NCOL * (size_t)q.row_stride;
#pragma unroll
    for (int n = 0; n < NREG; ++n) {
      const int e = lane + 64 * n, k = e / NX, i = e - k * NX;
      if (e < NX * NX) F[k * LD + i] = src[(size_t)k * q.row_stride + i];
    }
    if (mine) QV[lane] = q.q[(slot * T + t) * NX + lane];
  };
  auto get_mat = [&](float* dst, const float* src) {       // [nx][nx] in global memory -> rows of LD
    for (int e = lane; e < NX * NX; e += 64) { const int i = e / NX; dst[i * LD + e - i * NX] = src[e]; }
  };
  auto put_mat = [&](float* dst, const float* src) {
    for (int e = lane; e < NX * NX; e += 64) { const int i = e / NX; dst[e] = src[i * LD + e - i * NX]; }
  };
  auto a_times = [&](const float* x) {             // (A_t x)[lane], summed as row_dot_n sums
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    if (mine)
      for (int j = 0; j < NX; j += 4) {
        const float4 xj = lds4(x + j);
        a0 = __builtin_fmaf(F[(j + 0) * LD + lane], xj.x, a0); a1 = __builtin_fmaf(F[(j + 1) * LD + lane], xj.y, a1);
        a2 = __builtin_fmaf(F[(j + 2) * LD + lane], xj.z, a2); a3 = __builtin_fmaf(F[(j + 3) * LD + lane], xj.w, a3);
      }
    return (a0 + a1) + (a2 + a3);
  };

  // ---- the filter
  get_mat(P, q.P0 + slot * (size_t)(NX * NX));
  if (mine) XV[lane] = q.x0 ? q.x0[slot * NX + lane] : 0.0f;
  float nll = 0.0f;
  for (int t = 0; t < T; ++t) {
    load_step(t);
    {
      const float* src = q.columns + (slot * T + t) * D::NCOL * (size_t)q.row_stride + NX;
      if (lane < ny) {
#pragma unroll 4
        for (int j = 0; j < NX; ++j) CS[lane * LD + j] = src[(size_t)j * q.row_stride + lane];
        RV[lane] = q.r[(slot * T + t) * (size_t)ny + lane];
        YV[lane] = q.dy[(slot * T + t) * (size_t)ny + lane];
      }
    }
    WSYNC();
    for (int j = 0; j < ny; ++j) {
      const float rj = asf(uniform_i(__builtin_bit_cast(int, RV[j])));
      if (rj == __builtin_inff()) continue;        // a missing sample: skipped whole
      const float* c = CS + j * LD;
      const float w = mine ? row_dot_n(prow, c, NX) : 0.0f;
      if (mine) WV[lane] = w;
      WSYNC();
      f2 cw[2] = {f2{0.0f, 0.0f}, f2{0.0f, 0.0f}}, cx[2] = {f2{0.0f, 0.0f}, f2{0.0f, 0.0f}};
      for (int i = 0; i < NX; i += 4) { const float4 ci = lds4(c + i); dot_step(cw, ci, lds4(WV + i)); dot_step(cx, ci, lds4(XV + i)); }
      const float s = dot_sum(cw) + rj;
      const float nu = YV[j] - dot_sum(cx);
      const bool ok = rj > 0.0f && s > 0.0f && s < __builtin_inff();          // (rj is not +inf here; NaN fails every test)
      if (!uniform_i(ok)) {
        if (lane == 0) { q.status[2 * slot] = (float)t; q.status[2 * slot + 1] = -1.0f; if (q.nll) q.nll[slot] = 0.0f; }
        return;
      }
      const float sinv = 1.0f / s, g = nu / s;
      nll += 0.5f * (nu * g + logf(s) + LOG_2PI);
      if (mine) {
        XV[lane] = __builtin_fmaf(w, g, XV[lane]);
        for (int k = 0; k < NX; k += 4) {
          const float4 wk = lds4(WV + k);
          float4 p = lds4(prow + k);
          p.x = __builtin_fmaf(-(w * wk.x), sinv, p.x); p.y = __builtin_fmaf(-(w * wk.y), sinv, p.y);
          p.z = __builtin_fmaf(-(w * wk.z), sinv, p.z); p.w = __builtin_fmaf(-(w * wk.w), sinv, p.w);
          *reinterpret_cast<float4*>(prow + k) = p;
        }
      }
      WSYNC();
    }
    if (mine) q.xf[(slot * (T + 1) + t) * NX + lane] = XV[lane];
    if (q.pf) put_mat(q.pf + (slot * (T + 1) + t) * (size_t)(NX * NX), P);
    const float xn = a_times(XV);
    WSYNC();
    if (mine) XV[lane] = xn;
    kalman_predict<D>(sm, P, P, lane);
  }
  if (mine) q.xf[(slot * (T + 1) + T) * NX + lane] = XV[lane];
  if (q.pf) put_mat(q.pf + (slot * (T + 1) + T) * (size_t)(NX * NX), P);
  if (lane == 0) { q.status[2 * slot] = -1.0f; q.status[2 * slot + 1] = -1.0f; if (q.nll) q.nll[slot] = nll; }
  if (!q.xs) return;

  // ---- the smoother.  It loads rows of xf and pf that other lanes of this wave stored above: drain the stores, and keep every
  // load behind that point
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  for (int e = lane; e < NX * LD; e += 64) PS[e] = P[e];
  if (mine) { XS[lane] = XV[lane]; q.xs[(slot * (T + 1) + T) * NX + lane] = XV[lane]; }
  WSYNC();
  if (q.ps) put_mat(q.ps + (slot * (T + 1) + T) * (size_t)(NX * NX), PS);
  for (int t = T - 1; t >= 0; --t) {
    load_step(t);
    get_mat(P, q.pf + (slot * (T + 1) + t) * (size_t)(NX * NX));
    if (mine) XV[lane] = q.xf[(slot * (T + 1) + t) * NX + lane];
    for (int e = lane; e < NX * LD; e += 64) LF[e] = LT[e] = 0.0f;
    WSYNC();
    kalman_predict<D>(sm, P, PM, lane);            // W = Pf A^T, PM = Pm
    if (mine) DV[lane] = XS[lane] - a_times(XV);
    // Cholesky of Pm, a column per trip; a pivot <= 0 or not finite ends the slot's smoother
    for (int j = 0; j < NX; ++j) {
      const int j4 = (j + 3) & ~3;                 // (the factor's entries at and beyond the diagonal are zeros)
      const float d = asf(uniform_i(__builtin_bit_cast(int, PM[j * LD + j] - row_dot_n(LF + j * LD, LF + j * LD, j4))));
      if (!(d > 0.0f) || !(d < __builtin_inff())) {
        if (lane == 0) q.status[2 * slot + 1] = (float)t;
        return;
      }
      const float dinv = 1.0f / sqrtf(d);
      if (lane > j && mine) {
        const float v = (PM[lane * LD + j] - row_dot_n(LF + lane * LD, LF + j * LD, j4)) * dinv;
        LF[lane * LD + j] = v; LT[j * LD + lane] = v;
      }
      if (lane == j) DI[j] = dinv;
      WSYNC();
    }
    // G[l] = Pm^-1 (Pf A^T)[l], in lane l's own row of W; its transpose goes to S
    if (mine) {
      float* y = W + lane * LD;
      for (int c = 0; c < NX; ++c) y[c] = (y[c] - row_dot_n(LF + c * LD, y, (c + 3) & ~3)) * DI[c];
      for (int c = NX - 1; c >= 0; --c) {
        const int k0 = c & ~3;
        const float v = (y[c] - row_dot_n(LT + c * LD + k0, y + k0, NX - k0)) * DI[c];
        y[c] = v; S[c * LD + lane] = v;
      }
    }
    WSYNC();
    if (mine) {
      const float v = XV[lane] + row_dot<NX>(W + lane * LD, DV, 0.0f);
      XS[lane] = v;
      q.xs[(slot * (T + 1) + t) * NX + lane] = v;
    }
    for (int e = lane; e < NX * NX; e += 64) { const int i = e / NX, o = i * LD + e - i * NX; PM[o] = PS[o] - PM[o]; }
    WSYNC();
    kalman_prod<D>(PM, S, LF, lane);               // U = D G^T
    WSYNC();
    kalman_prod<D>(S, LF, LT, lane);               // G U
    WSYNC();
    for (int e = lane; e < NX * NX; e += 64) {
      const int i = e / NX, k = e - i * NX;
      PS[i * LD + k] = P[i * LD + k] + 0.5f * (LT[i * LD + k] + LT[k * LD + i]);
    }
    WSYNC();
    if (q.ps) put_mat(q.ps + (slot * (T + 1) + t) * (size_t)(NX * NX), PS);
  }
}

}  // namespace rsr
