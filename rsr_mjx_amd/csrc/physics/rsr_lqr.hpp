// rsr_lqr.hpp -- rsr_physics_lqr_backward (include/rsr_physics.h): the backward recursion of iLQR / time-varying LQR (Tassa et al.
// 2012, the unregularised Q in the value update) on the columns rsr_physics_trajectory_fd writes, with the gains in the layout
// rsr_physics_feedback_rollouts reads.  One wave per slot walks t = T-1 .. 0 in one launch with Vxx, F_t = [A_t B_t], W = Vxx F and
// the Q blocks in LDS.  The kernel reads neither the model nor the record: C gives NV and NU, i.e. static LDS offsets, loop bounds
// and register tiles, and the first three kernel arguments are there only because every physics op is sent by the one launch lambda.
//
// Layout.  nx = 2 NV, nc = nx + NU.  Every matrix is rows of LD floats with the state index contiguous: V[l][i] (symmetric),
// F[k][i] = column k of [A B] (a row of `columns` as it lies in memory, so the loader copies rows and transposes nothing), W[k][i]
// = column k of Vxx F, P[a][b] = (F^T W + cost)[a][b] for b < nx (rows a < nx: Qxx, rows a >= nx: Qux), K[j][b], G[j][b] =
// (Quu K + Qux)[j][b].  All three nx^2-sized products then read rows only, four floats at a time (ds_read_b128), and no product
// reads a matrix across its rows.  LD = nx, plus 4 where nx / 4 is even, so that LD / 4 is odd: the lanes of a tile column read rows
// that lie LD apart, a b128 read takes 16-byte slot (row LD / 4 + const) mod 16 of the 256-byte bank row, and an odd multiplier
// makes up to 16 rows hit 16 different slots (nx = 40 unpadded: rows 0 and 8 collide, 10 r mod 16; LD = 44: 11 r mod 16, none).
//
// Lanes.  A product's outputs are cut into 4 x KB register tiles, lane = kb IB + ib with IB = nx / 4: four state indices (4 ib ..
// 4 ib + 3 in W, ib + IB c in P: rows LD apart again) by the KB rows r KBLK + kb, KBLK = 64 / IB, KB = ceil(nc / KBLK) (cube 4 x 8
// on 60 lanes, Go2 4 x 7 on 63, T-shape 4 x 4 on 63).  Rows nc .. KBLK KB of F are zeros, so no tile tests a bound.  The value
// update runs on tile pairs: the lane of (ib <= jb) forms the 4 x 4 tiles (ib, jb) and (jb, ib) of Qxx + K^T G + Qux^T K, averages
// one with the other's transpose in registers and writes both, so Vxx is symmetric bit for bit and is never read across its rows.
// Every output element is one lane's fma chain in a fixed order (ascending; in F^T W the even and the odd indices apart, added at
// the end): the result depends on the slot's inputs alone.  The products' fmas are written on float pairs (v_pk_fma_f32).
// The NU x NU Cholesky runs in LDS on the wave (a column per step), the solves one right-hand side per lane (nx columns of Qux~
// and Qu) with the column in registers.  Global loads of the next step's F and of this step's cost rows are issued before the first
// product and land in registers while it runs.
//
// rsr_physics_lqr_box (box_backward_kernel) is the same body with BOX = true: between the Q blocks and the value update, k_t is the
// minimiser of the step's QP over lo <= x <= hi by projected Newton steps (the iteration is stated in include/rsr_physics.h), the
// factor is taken of Quu~ with the clamped rows and columns replaced by the identity's, and the right-hand sides of the clamped rows
// of K are zeros.  Lane j < nu holds entry j of the QP's vectors and forms its entry of H x as one fma chain; every lane runs the one
// nu x nu solve on the same LDS words, so y needs no broadcast; the clamped set is a ballot.  With no bound reached the arithmetic
// that reaches the outputs is the plain pass's, operation for operation.
#pragma once
#include "../rsr_launch.hpp"

namespace rsr {

template <class C>
struct LqrDims {
  static constexpr int NX = 2 * C::NV, NU = C::NU, NC = NX + NU;
  static constexpr int IB = NX / 4;                          // tile columns: four state indices each
  static constexpr int LD = NX + ((IB & 1) ? 0 : 4);         // row pitch, LD / 4 odd
  static constexpr int KBLK = 64 / IB;                       // tile rows
  static constexpr int KB = (NC + KBLK - 1) / KBLK;          // matrix rows per tile
  static constexpr int ROWS = KBLK * KB;                     // rows of F, W, P (>= NC; F's rows >= NC stay zero)
  static constexpr int TILES = IB * KBLK;                    // lanes with a tile
  static constexpr int PAIRS = IB * (IB + 1) / 2;            // lanes with a tile pair of the value update
  static constexpr int NREG = (NC * NX + 63) / 64;           // registers per lane that hold one [nc][nx] block in flight
  // offsets, floats (each a multiple of 4: the rows are read 16 bytes at a time)
  static constexpr int V = 0, F = V + NX * LD, W = F + ROWS * LD, P = W + ROWS * LD, K = P + ROWS * LD, G = K + NU * LD;
  static constexpr int QUU = G + NU * LD, LF = QUU + ((NU * NU + 3) & ~3);     // Quu, and the factor of Quu~
  static constexpr int VX = LF + ((NU * NU + 3) & ~3), Q = VX + NX;            // Vx [nx]; Qx | Qu [nc]
  static constexpr int KV = Q + ((NC + 3) & ~3), GV = KV + 16;                  // k [nu]; Quu k + Qu [nu]
  static constexpr int FLOATS = GV + 16;
  static_assert(NX % 4 == 0 && NU <= 16 && NC <= 64 && NX + 1 <= 64, "one lane per row of F and per right-hand side");
  static_assert(TILES <= 64 && PAIRS <= 64 && ROWS >= NC, "one tile and one tile pair per lane");
};
template <class C>
constexpr size_t lqr_lds_bytes() { return sizeof(float) * LqrDims<C>::FLOATS; }

__device__ __forceinline__ float4 lds4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// Two fp32 fmas per instruction (v_pk_fma_f32): one wave alone issues a VALU instruction every 4 cycles, packed or not, and the
// products are bound by that.  Each half is the same IEEE fma as the scalar instruction's.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// acc (four floats as two pairs) += s v
__device__ __forceinline__ void fma4(f2 (&acc)[2], float s, const float4& v) {
  acc[0] = pk_fma(f2{s, s}, f2{v.x, v.y}, acc[0]); acc[1] = pk_fma(f2{s, s}, f2{v.z, v.w}, acc[1]);
}
// acc (the sums over even and over odd indices) += a b, entry by entry
__device__ __forceinline__ f2 dot4_eo(f2 acc, const float4& a, const float4& b) {
  return pk_fma(f2{a.z, a.w}, f2{b.z, b.w}, pk_fma(f2{a.x, a.y}, f2{b.x, b.y}, acc));
}
__device__ __forceinline__ float dot4(float acc, const float4& a, const float4& b) {
  return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, __builtin_fmaf(a.x, b.x, acc))));
}
// sum over i < N of a[i] b[i], ascending, from acc (rows of LDS, N a multiple of 4)
template <int N>
__device__ __forceinline__ float row_dot(const float* a, const float* b, float acc) {
  for (int i = 0; i < N; i += 4) acc = dot4(acc, lds4(a + i), lds4(b + i));
  return acc;
}

// What rsr_physics_lqr_box adds to the image: Quu~ as it was formed (the factor is taken in place and taken again for every set of
// clamped controls), and the QP's vectors, 16 floats each: x, the gradient, the right-hand side, the trial point, H z.  The bounds
// of a step stay in the registers of the lanes j < nu.
template <class C>
struct BoxDims {
  static constexpr int NU = C::NU;
  static constexpr int H = LqrDims<C>::FLOATS, X = H + ((NU * NU + 3) & ~3), GR = X + 16, R = GR + 16, Z = R + 16, HZ = Z + 16;
  static constexpr int FLOATS = HZ + 16;
};
template <class C>
constexpr size_t box_lds_bytes() { return sizeof(float) * BoxDims<C>::FLOATS; }

// The one body of both passes.  BOX = false: the plain recursion; bx is not read and every branch on BOX folds away.
template <class C, bool BOX>
__device__ __forceinline__ void lqr_body(const LqrArgs& q, const BoxArgs& bx);

// Workgroup s: slot s.  WAVES: the family's waves per SIMD, an upper bound only (the LDS image admits fewer).
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WAVES)))
void lqr_kernel(const DModel* __restrict__, Layout, StepArgs, LqrArgs q) {
  lqr_body<C, false>(q, BoxArgs{});
}
// rsr_physics_lqr_box: the same recursion with k_t the minimiser of the step's box-constrained QP (Tassa, Mansard and Todorov 2014)
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WAVES)))
void box_backward_kernel(const DModel* __restrict__, Layout, StepArgs, BoxArgs b) {
  lqr_body<C, true>(b.lq, b);
}

template <class C, bool BOX>
__device__ __forceinline__ void lqr_body(const LqrArgs& q, const BoxArgs& bx) {
  using D = LqrDims<C>;
  using E = BoxDims<C>;
  constexpr int NX = D::NX, NU = D::NU, NC = D::NC, LD = D::LD, IB = D::IB, KBLK = D::KBLK, KB = D::KB, NREG = D::NREG;
  constexpr int NQUU = (NU * NU + 63) / 64;      // entries of Quu per lane
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* const sm = reinterpret_cast<float*>(smem_raw);
  float *const V = sm + D::V, *const F = sm + D::F, *const W = sm + D::W, *const P = sm + D::P, *const K = sm + D::K, *const G = sm + D::G;
  float *const QUU = sm + D::QUU, *const LF = sm + D::LF, *const VX = sm + D::VX, *const Q = sm + D::Q, *const KV = sm + D::KV, *const GV = sm + D::GV;
  float *const HQ = sm + E::H, *const BX = sm + E::X, *const BG = sm + E::GR, *const BR = sm + E::R, *const BZ = sm + E::Z, *const BHZ = sm + E::HZ;   // (BOX)
  const int lane = threadIdx.x, T = q.T;
  const size_t slot = blockIdx.x;
  const float mu = q.mu[slot];
  const bool state_reg = (q.flags & RSR_LQR_REG_STATE) != 0;
  const int ib = lane % IB, kb = lane / IB;
  const bool tile = lane < D::TILES, pair = lane < D::PAIRS;
  int pi = 0, pj = 0;                              // the tile pair (pi <= pj) of the value update
  { int p = pair ? lane : 0; while (p >= IB - pi) { p -= IB - pi; ++pi; } pj = pi + p; }

  // block e -> (row e / NX, entry e % NX) of an [nc][nx] block, 64 consecutive floats of a row (or of two) per load
  float freg[NREG], creg[NREG];
  auto fetch_F = [&](int t) {                      // [A_t B_t]: rows of `columns`, row_stride apart
    const float* src = q.columns + (slot * T + t) * NC * (size_t)q.row_stride;
#pragma unroll
    for (int n = 0; n < NREG; ++n) {
      const int e = lane + 64 * n, k = e / NX, i = e - k * NX;
      freg[n] = e < NC * NX ? src[(size_t)k * q.row_stride + i] : 0.0f;
    }
  };
  auto fetch_cost = [&](int t) {                   // [lxx_t; lux_t], lux null: zeros, added like any other
    const float* xx = q.lxx + (slot * (T + 1) + t) * (size_t)(NX * NX);
    const float* ux = q.lux ? q.lux + (slot * T + t) * (size_t)(NU * NX) : nullptr;
#pragma unroll
    for (int n = 0; n < NREG; ++n) {
      const int e = lane + 64 * n;
      creg[n] = e < NX * NX ? xx[e] : (ux && e < NC * NX ? ux[e - NX * NX] : 0.0f);
    }
  };
  auto put = [&](float* dst, const float (&reg)[NREG]) {
#pragma unroll
    for (int n = 0; n < NREG; ++n) {
      const int e = lane + 64 * n, k = e / NX, i = e - k * NX;
      if (e < NC * NX) dst[k * LD + i] = reg[n];
    }
  };
  auto record = [&](int t) {                       // the optional value rows of step t (T: the terminal cost)
    if (q.vx && lane < NX) q.vx[(slot * (T + 1) + t) * NX + lane] = VX[lane];
    if (q.vxx) {
      float* o = q.vxx + (slot * (T + 1) + t) * (size_t)(NX * NX);
      for (int e = lane; e < NX * NX; e += 64) { const int i = e / NX; o[e] = V[i * LD + e - i * NX]; }
    }
  };

  // the terminal cost, F's zero rows, the first step's F
  fetch_F(T - 1);
  {
    const float* xx = q.lxx + (slot * (T + 1) + T) * (size_t)(NX * NX);
    for (int e = lane; e < NX * NX; e += 64) { const int i = e / NX; V[i * LD + e - i * NX] = xx[e]; }
    if (lane < NX) VX[lane] = q.lx[(slot * (T + 1) + T) * NX + lane];
    for (int e = NC * LD + lane; e < D::ROWS * LD; e += 64) F[e] = 0.0f;
  }
  put(F, freg);
  WSYNC();
  record(T);
  float dv0 = 0.0f, dv1 = 0.0f;                    // lane NX's
  for (int t = T - 1; t >= 0; --t) {
    fetch_cost(t);
    if (t > 0) fetch_F(t - 1);
    // (and the step's small cost rows: a load where its value is used would stand in the way for a round trip to memory)
    const float lq = lane < NX ? q.lx[(slot * (T + 1) + t) * NX + lane] : (lane < NC ? q.lu[(slot * T + t) * NU + lane - NX] : 0.0f);
    const bool mine = lane < NU;                   // (BOX) lane j < nu: entry j of the QP's vectors
    float lj = 0.0f, hj = 0.0f;
    if constexpr (BOX) {
      if (mine) { lj = bx.lo[(slot * T + t) * NU + lane]; hj = bx.hi[(slot * T + t) * NU + lane]; }
    }
    float luu[NQUU];
#pragma unroll
    for (int n = 0; n < NQUU; ++n) luu[n] = lane + 64 * n < NU * NU ? q.luu[(slot * T + t) * (size_t)(NU * NU) + lane + 64 * n] : 0.0f;
    // W = Vxx F: W[k][i] = sum_l F[k][l] V[l][i], four l per trip
    if (tile) {
      f2 acc[KB][2];
#pragma unroll
      for (int r = 0; r < KB; ++r) acc[r][0] = acc[r][1] = f2{0.0f, 0.0f};
      for (int l = 0; l < NX; l += 4) {
        const float4 v0 = lds4(V + (l + 0) * LD + 4 * ib), v1 = lds4(V + (l + 1) * LD + 4 * ib);
        const float4 v2 = lds4(V + (l + 2) * LD + 4 * ib), v3 = lds4(V + (l + 3) * LD + 4 * ib);
#pragma unroll
        for (int r = 0; r < KB; ++r) {
          const float4 f = lds4(F + (r * KBLK + kb) * LD + l);
          fma4(acc[r], f.x, v0); fma4(acc[r], f.y, v1); fma4(acc[r], f.z, v2); fma4(acc[r], f.w, v3);
        }
      }
#pragma unroll
      for (int r = 0; r < KB; ++r) *reinterpret_cast<float4*>(W + (r * KBLK + kb) * LD + 4 * ib) = make_float4(acc[r][0].x, acc[r][0].y, acc[r][1].x, acc[r][1].y);
    }
    // Qx | Qu = lx_t | lu_t + F^T Vx, a lane per row of F
    if (lane < NC) Q[lane] = lq + row_dot<NX>(F + lane * LD, VX, 0.0f);
    put(P, creg);
    WSYNC();
    // P = [lxx_t; lux_t] + F^T W on the columns b < nx: P[a][b] = sum_i F[a][i] W[b][i], four i per trip, the even and the odd i
    // summed apart and added at the end
    if (tile) {
      f2 acc[KB][4];
#pragma unroll
      for (int r = 0; r < KB; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = f2{0.0f, 0.0f};
      for (int i = 0; i < NX; i += 4) {
        const float4 w0 = lds4(W + (0 * IB + ib) * LD + i), w1 = lds4(W + (1 * IB + ib) * LD + i);
        const float4 w2 = lds4(W + (2 * IB + ib) * LD + i), w3 = lds4(W + (3 * IB + ib) * LD + i);
#pragma unroll
        for (int r = 0; r < KB; ++r) {
          const float4 f = lds4(F + (r * KBLK + kb) * LD + i);
          acc[r][0] = dot4_eo(acc[r][0], f, w0); acc[r][1] = dot4_eo(acc[r][1], f, w1);
          acc[r][2] = dot4_eo(acc[r][2], f, w2); acc[r][3] = dot4_eo(acc[r][3], f, w3);
        }
      }
#pragma unroll
      for (int r = 0; r < KB; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) P[(r * KBLK + kb) * LD + c * IB + ib] += acc[r][c].x + acc[r][c].y;
    }
    // Quu = luu_t + B^T Vxx B, and Quu~ where the factor will stand
#pragma unroll
    for (int n = 0; n < NQUU; ++n) {
      const int e = lane + 64 * n, j = e / NU, j2 = e - j * NU;
      if (e >= NU * NU) continue;
      const float quu = luu[n] + row_dot<NX>(F + (NX + j) * LD, W + (NX + j2) * LD, 0.0f);
      QUU[e] = quu;
      const float quur = quu + (state_reg ? mu * row_dot<NX>(F + (NX + j) * LD, F + (NX + j2) * LD, 0.0f) : (j == j2 ? mu : 0.0f));
      LF[e] = quur;
      if constexpr (BOX) HQ[e] = quur;
    }
    WSYNC();
    // Cholesky of what LF holds, in place, a column per trip; a pivot <= 0 or not finite ends the slot (wave-uniform: one LDS
    // word).  Every lane keeps the reciprocals of the factor's diagonal: the solves multiply by them.
    float dinv[NU];
    auto chol = [&]() {
      bool ok = true;
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        const float d = asf(uniform_i(__builtin_bit_cast(int, LF[j * NU + j])));
        if (!(d > 0.0f) || !(d < __builtin_inff())) ok = false;     // (the later columns then run on for nothing: the slot ends below)
        dinv[j] = 1.0f / sqrtf(d);
        if (lane > j && lane < NU) LF[lane * NU + j] = LF[lane * NU + j] * dinv[j];
        WSYNC();
        for (int e = lane; e < NU * NU; e += 64) {
          const int i = e / NU, c = e - i * NU;
          if (c > j && i >= c) LF[e] = __builtin_fmaf(-LF[i * NU + j], LF[c * NU + j], LF[e]);
        }
        WSYNC();
      }
      return ok;
    };
    // x = -(L L^T)^-1 x with the factor in LF, the column in registers
    auto solve = [&](float (&x)[NU]) {
#pragma unroll
      for (int j = 0; j < NU; ++j) {
#pragma unroll
        for (int c = 0; c < j; ++c) x[j] = __builtin_fmaf(-LF[j * NU + c], x[c], x[j]);
        x[j] = x[j] * dinv[j];
      }
#pragma unroll
      for (int j = NU - 1; j >= 0; --j) {
#pragma unroll
        for (int c = NU - 1; c > j; --c) x[j] = __builtin_fmaf(-LF[c * NU + j], x[c], x[j]);
        x[j] = x[j] * dinv[j];
      }
#pragma unroll
      for (int j = 0; j < NU; ++j) x[j] = -x[j];
    };
    bool ok;
    unsigned cm = 0u;                              // bit j: control j is clamped (the plain pass: none)
    int code = 0, steps = 0;
    float clampj = 0.0f;
    if constexpr (!BOX) ok = chol();
    else {
      // k = argmin 1/2 x^T H x + g^T x over lo <= x <= hi, H = Quu~, g = Qu, by projected Newton steps (include/rsr_physics.h states
      // it line by line).  Lane j < nu holds entry j of x, l, h, the gradient and the step, and forms its entry of every product as
      // one fma chain over i ascending; the solve and the two scalars of the Armijo test are formed by every lane alike from LDS
      // words.  Every branch around a WSYNC is taken on a ballot, on `it`, or on a value sent through uniform_i.
      constexpr unsigned ALL = (1u << NU) - 1u, NONE = ~0u;
      const float* Hj = HQ + (mine ? lane : 0) * NU;                // row j of H
      // Armijo needs f(v) = 1/2 v^T H v + g^T v of a vector in LDS: H v a lane per row, then sum_j (1/2 (H v)_j + g_j) v_j ascending
      auto fval = [&](const float* v) {
        float hv = 0.0f;
#pragma unroll
        for (int i = 0; i < NU; ++i) hv = __builtin_fmaf(Hj[i], v[i], hv);
        WSYNC();
        if (mine) BHZ[lane] = hv;
        WSYNC();
        float f = 0.0f;
#pragma unroll
        for (int j = 0; j < NU; ++j) f = __builtin_fmaf(__builtin_fmaf(0.5f, BHZ[j], Q[NX + j]), v[j], f);
        return f;
      };
      auto factor = [&]() {                        // Hm: H with the rows and columns of cm replaced by the identity's
        WSYNC();
        for (int e = lane; e < NU * NU; e += 64) {
          const int i = e / NU, c = e - i * NU;
          LF[e] = ((cm >> i) | (cm >> c)) & 1u ? (i == c ? 1.0f : 0.0f) : HQ[e];
        }
        WSYNC();
        return chol();
      };
      ok = __ballot(mine && !(lj <= hj)) == 0ull;
      if (ok) {
        const float gj = mine ? Q[NX + lane] : 0.0f;
        float xj = 0.0f < lj ? lj : (0.0f > hj ? hj : 0.0f), grad = 0.0f;
        bool cj = false, full = false;
        unsigned cprev = NONE, cfac = NONE;
        if (mine) BX[lane] = xj;
        WSYNC();
        for (int it = 0;; ++it) {                  // (leaves at it == max_iter at the latest)
          grad = gj;
#pragma unroll
          for (int i = 0; i < NU; ++i) grad = __builtin_fmaf(Hj[i], BX[i], grad);
          cj = mine && ((xj == lj && grad > 0.0f) || (xj == hj && grad < 0.0f));
          cm = (unsigned)__ballot(cj);
          steps = it;
          if (cm == ALL) { code = 1; break; }
          if (full && cm == cprev) { code = 0; break; }
          if (it == bx.max_iter) { code = 2; break; }
          ok = factor();
          cfac = cm;
          if (!ok) break;
          float r = gj;
#pragma unroll
          for (int i = 0; i < NU; ++i) r = (cm >> i) & 1u ? __builtin_fmaf(Hj[i], BX[i], r) : r;
          if (mine) { BR[lane] = cj ? 0.0f : r; BG[lane] = grad; }
          WSYNC();
          float y[NU], yj = 0.0f;
#pragma unroll
          for (int j = 0; j < NU; ++j) y[j] = BR[j];
          solve(y);
#pragma unroll
          for (int j = 0; j < NU; ++j) yj = lane == j ? y[j] : yj;
          const float xs = cj ? xj : yj, dj = xs - xj, xn = xj + dj;
          cprev = cm;
          if (__ballot(mine && !(lj <= xn && xn <= hj)) == 0ull) {   // the full step stays inside: take it as it is
            xj = xs; full = true;
            WSYNC();
            if (mine) BX[lane] = xj;
            WSYNC();
            continue;
          }
          full = false;
          const float f0 = fval(BX);
          float a = 1.0f, zj = xj;
          bool taken = false;
          for (int n = 0; n < 20 && !taken; ++n, a *= 0.6f) {
            zj = __builtin_fmaf(a, dj, xj);
            zj = zj < lj ? lj : (zj > hj ? hj : zj);
            WSYNC();
            if (mine) BZ[lane] = zj;
            WSYNC();
            const float fz = fval(BZ);
            float gd = 0.0f;
#pragma unroll
            for (int j = 0; j < NU; ++j) gd = __builtin_fmaf(BG[j], BX[j] - BZ[j], gd);
            taken = uniform_i(f0 - fz >= 0.1f * gd) != 0;
          }
          if (!taken) { code = 3; break; }
          xj = zj;
          WSYNC();
          if (mine) BX[lane] = xj;
          WSYNC();
        }
        if (ok && code != 1 && cm != cfac) ok = factor();            // (max_iter came with another set than the last factor's)
        // a clamped control is its bound bit for bit (the sign of a zero too)
        if (cj) xj = grad > 0.0f ? lj : hj;
        clampj = cj ? (grad > 0.0f ? -1.0f : 1.0f) : 0.0f;
        WSYNC();
        if (mine) BX[lane] = xj;
        WSYNC();
      }
    }
    if (!ok) {
      if (lane == 0) { q.status[slot] = (float)t; q.dv[2 * slot] = 0.0f; q.dv[2 * slot + 1] = 0.0f; }
      return;
    }
    if constexpr (BOX) {
      if (bx.clamped && mine) bx.clamped[(slot * T + t) * NU + lane] = clampj;
      if (bx.qp && lane == 0) { bx.qp[(slot * T + t) * 2] = (float)steps; bx.qp[(slot * T + t) * 2 + 1] = (float)code; }
    }
    // K = -Quu~^-1 Qux~ and k = -Quu~^-1 Qu: lane b < nx column b, lane nx the vector; then G = Quu K + Qux, Quu k + Qu, dV.  BOX: k
    // is the QP's x, and the rows of K of the clamped controls are zeros (their right-hand sides are, and Hm's rows are the identity's)
    if (lane <= NX) {
      float x[NU];
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        if (lane == NX) x[j] = BOX ? BX[j] : Q[NX + j];
        else x[j] = P[(NX + j) * LD + lane] + (state_reg ? mu * row_dot<NX>(F + (NX + j) * LD, F + lane * LD, 0.0f) : 0.0f);
        if (BOX && lane != NX && ((cm >> j) & 1u)) x[j] = 0.0f;
      }
      if (!BOX || (lane != NX && code != 1)) solve(x);
      float g[NU];                                  // Quu x
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        g[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < NU; ++c) g[j] = __builtin_fmaf(QUU[j * NU + c], x[c], g[j]);
      }
      if (lane == NX) {
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
          a0 = __builtin_fmaf(x[j], Q[NX + j], a0); a1 = __builtin_fmaf(x[j], g[j], a1);
          KV[j] = x[j]; GV[j] = g[j] + Q[NX + j];
          q.k[(slot * T + t) * NU + j] = x[j];
        }
        dv0 += a0; dv1 += 0.5f * a1;
      } else {
        float* gain = q.gain + (slot * T + t) * (size_t)(NU * NX) + lane;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
          K[j * LD + lane] = x[j]; G[j * LD + lane] = g[j] + P[(NX + j) * LD + lane];
          gain[j * NX] = x[j];
        }
      }
    }
    WSYNC();
    // Vx = Qx + K^T (Quu k + Qu) + Qux^T k
    if (lane < NX) {
      float vx = Q[lane];
#pragma unroll
      for (int j = 0; j < NU; ++j) vx = __builtin_fmaf(P[(NX + j) * LD + lane], KV[j], __builtin_fmaf(K[j * LD + lane], GV[j], vx));
      VX[lane] = vx;
    }
    // Vxx = Qxx + K^T G + Qux^T K, symmetrised: the tiles (pi, pj) and (pj, pi), averaged in registers
    if (pair) {
      const int i0 = 4 * pi, j0 = 4 * pj;
      f2 X[4][2], Y[4][2];                          // X[r]: row r of tile (pi, pj); Y[c]: row c of tile (pj, pi); two pairs each
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 a = lds4(P + (i0 + r) * LD + j0), b = lds4(P + (j0 + r) * LD + i0);
        X[r][0] = f2{a.x, a.y}; X[r][1] = f2{a.z, a.w};
        Y[r][0] = f2{b.x, b.y}; Y[r][1] = f2{b.z, b.w};
      }
      for (int a = 0; a < NU; ++a) {
        const float4 ki = lds4(K + a * LD + i0), kj = lds4(K + a * LD + j0), gi = lds4(G + a * LD + i0), gj = lds4(G + a * LD + j0);
        const float4 ui = lds4(P + (NX + a) * LD + i0), uj = lds4(P + (NX + a) * LD + j0);
        fma4(X[0], ki.x, gj); fma4(X[1], ki.y, gj); fma4(X[2], ki.z, gj); fma4(X[3], ki.w, gj);
        fma4(X[0], ui.x, kj); fma4(X[1], ui.y, kj); fma4(X[2], ui.z, kj); fma4(X[3], ui.w, kj);
        fma4(Y[0], kj.x, gi); fma4(Y[1], kj.y, gi); fma4(Y[2], kj.z, gi); fma4(Y[3], kj.w, gi);
        fma4(Y[0], uj.x, ki); fma4(Y[1], uj.y, ki); fma4(Y[2], uj.z, ki); fma4(Y[3], uj.w, ki);
      }
      float S[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) S[r][c] = 0.5f * (X[r][c >> 1][c & 1] + Y[c][r >> 1][r & 1]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        *reinterpret_cast<float4*>(V + (i0 + r) * LD + j0) = make_float4(S[r][0], S[r][1], S[r][2], S[r][3]);
        *reinterpret_cast<float4*>(V + (j0 + r) * LD + i0) = make_float4(S[0][r], S[1][r], S[2][r], S[3][r]);
      }
    }
    if (t > 0) put(F, freg);
    WSYNC();
    record(t);
  }
  if (lane == NX) { q.dv[2 * slot] = dv0; q.dv[2 * slot + 1] = dv1; }
  if (lane == 0) q.status[slot] = -1.0f;
}

}  // namespace rsr
