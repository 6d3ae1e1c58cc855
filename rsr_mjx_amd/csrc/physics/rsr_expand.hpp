// rsr_expand.hpp -- rsr_physics_cost_expand (include/rsr_physics.h): the weighted least-squares cost of the cost rollouts expanded
// to second order (Gauss-Newton) about a nominal run, into the five operands the Riccati pass takes: lx, lu, lxx, luu, lux.  One wave
// per (slot, t'), t' = 0 .. T: index t' takes the state part of cost row t' - 1 (none at t' = 0) and the ctrl and sensor parts of
// cost row t' (none at t' = T).  The steps are independent, so there is no recursion to keep inside a wave.  The kernel reads
// neither the model nor the record: C gives NV and NU, i.e. static LDS offsets and loop bounds, and the first three kernel arguments
// are there only because every physics op is sent by the one launch lambda.
//
// Layout.  nx = 2 NV, nc = nx + NU.  The sensor part of the nc column rows of step t' (C_t | D_t as they lie in `columns`: row a
// holds at nx + j the derivative of sensor entry j by coordinate a) is staged in LDS transposed, CT[j][a] with rows of LD floats:
// lane j loads entry j of every row a (the entries of a row are contiguous in j, so a load is coalesced) and stores it at
// j LD + a.  LD = ROWS + 4 with ROWS = nc rounded up to 8, the columns nc .. ROWS - 1 zeros: a multiple of 4, so that four
// coordinates of one j are one 16-byte read or store, and LD / 4 odd, so that the 16-byte staging stores of eight neighbouring
// lanes (rows LD words apart) fall on eight different 4-bank slots of the 32 (with LD / 4 even they would share
// four).  Beside it two vectors of 64: WV[j] = w_sensor[j] and GV[j] = w_sensor[j] ds[j].
//
// Lanes.  The coordinate index runs across lanes, the sensor index j is the loop: lane b < nc owns entry b of lx | lu and column b of
// the nc x nc product G[a][b] = sum_j (CT[j][a] CT[j][b]) WV[j] (lxx = G[:nx, :nx], lux = G[nx:, :nx], luu = G[nx:, nx:]), with the
// sum of every row a in a register of its own (ROWS of them), so one walk over j serves all five outputs.  Per j a lane reads its
// own CT[j][b] (the 64 lanes read consecutive words: no bank conflict), WV[j], GV[j] and the row CT[j][0 .. ROWS - 1] sixteen bytes
// at a time (the same address in every lane: a broadcast), and every row of lxx / lux / luu is stored by consecutive lanes.  The
// arithmetic is on float pairs (v_pk_mul_f32, v_pk_add_f32), three roundings per term and no fma: the product (c_a c_b) commutes,
// so lxx and luu are symmetric bit for bit.  lx | lu: lane a < nc starts from its state or ctrl part and adds CT[j][a] GV[j], j
// ascending.  The cost and residual rows (three as a coordinate, three as a sensor entry) and the lane's entry of all nc column
// rows are loaded into registers before the first wait, so a wave pays one round trip to memory; the state and the ctrl lanes
// share one set of loads whose addresses are chosen by selects, since two branches writing the same registers would each end in a
// wait.
#pragma once
#include "../rsr_launch.hpp"

namespace rsr {

template <class C>
struct ExpandDims {
  static constexpr int NV = C::NV, NX = 2 * C::NV, NU = C::NU, NC = NX + NU;
  static constexpr int ROWS = (NC + 7) & ~7;                 // rows of the product, in blocks of eight
  static constexpr int LD = ROWS + 4;                        // pitch of CT[j]; LD / 4 odd
  static constexpr int WV = 0, GV = WV + 64, CT = GV + 64;
  static constexpr int FLOATS = CT + RSR_MAX_SENSORDATA * LD;
  static_assert(NC <= 64 && RSR_MAX_SENSORDATA <= 64, "one lane per coordinate and per sensor entry");
  static_assert(LD % 4 == 0 && (LD / 4) % 2 == 1, "16-byte reads and stores of a row; eight lanes' staging stores on eight different slots");
};
template <class C>
constexpr size_t expand_lds_bytes() { return sizeof(float) * ExpandDims<C>::FLOATS; }

// Workgroup w: slot w / (T + 1), index t' = w mod (T + 1).  WAVES: the family's waves per SIMD, an upper bound only.
template <class C, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WAVES)))
void expand_kernel(const DModel* __restrict__, Layout, StepArgs, ExpandArgs q) {
#pragma clang fp contract(off)
  using D = ExpandDims<C>;
  typedef float v2 __attribute__((ext_vector_type(2)));
  constexpr int NV = D::NV, NX = D::NX, NU = D::NU, NC = D::NC, LD = D::LD;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* const sm = reinterpret_cast<float*>(smem_raw);
  float *const WV = sm + D::WV, *const GV = sm + D::GV, *const CT = sm + D::CT;
  const int lane = threadIdx.x, T = q.T;
  const size_t slot = blockIdx.x / (unsigned)(T + 1);
  const int tp = (int)(blockIdx.x - slot * (size_t)(T + 1));
  const bool st = tp > 0, cu = tp < T;           // the state part of cost row tp - 1; the ctrl and sensor parts of cost row tp
  const size_t rs = slot * T + (st ? tp - 1 : 0), rc = slot * T + (cu ? tp : 0), ro = slot * (size_t)(T + 1) + tp;
  const int ny = cu && q.w_sensor ? q.ny : 0;

  // ---- every global load, issued before the first wait: this lane's weight, residual source and reference as a coordinate (one
  // set of addresses chosen by selects, so that the state and the ctrl lanes share the loads and no branch ends in a wait) and as
  // a sensor entry, then its entry of all nc column rows into registers
  const bool is_s = st && lane < NX, is_c = cu && lane >= NX && lane < NC;
  const float* wbase = is_s ? (lane < NV ? q.w_qpos : q.w_qvel) : is_c ? q.w_ctrl : nullptr;
  const bool on = wbase != nullptr;
  const size_t wo = is_s ? rs * NV + (lane < NV ? lane : lane - NV) : rc * NU + lane - NX;
  const float* rp = is_s ? q.dx + rs * NX + lane : q.ctrl + rc * NU + lane - NX;
  const bool has_y = is_c && on && q.ctrl_ref;
  const bool sens = lane < ny;
  float wa = 0.0f, ra = 0.0f, ya = 0.0f, ws = 0.0f, sd = 0.0f, sr = 0.0f;
  float cv[NC];
  if (on) { wa = wbase[wo]; ra = *rp; }
  if (has_y) ya = q.ctrl_ref[rc * NU + lane - NX];
  if (sens) {
    ws = q.w_sensor[rc * (size_t)q.ny + lane]; sd = q.sensordata[rc * (size_t)q.ny + lane];
    if (q.sensor_ref) sr = q.sensor_ref[rc * (size_t)q.ny + lane];
    const float* src = q.columns + rc * NC * (size_t)q.row_stride + NX + lane;
#pragma unroll
    for (int a = 0; a < NC; ++a) cv[a] = src[(size_t)a * q.row_stride];
#pragma unroll
    for (int a = 0; a < NC; ++a) CT[lane * LD + a] = cv[a];
    for (int a = NC; a < D::ROWS; ++a) CT[lane * LD + a] = 0.0f;
  }
  WV[lane] = ws; GV[lane] = ws * (sd - sr);
  WSYNC();

  // ---- one walk over j for all outputs.  Lane b owns entry b of lx | lu and column b of lxx / lux / luu, every row's sum in a
  // register.  lx | lu start from the state or ctrl part (one subtraction, one product; +0 where the term is off), the diagonal
  // from the coordinate's weight.
  constexpr int NP = D::ROWS / 8;                // row blocks of eight
  const int b = lane < NC ? lane : NC - 1;
  const float sw = on ? wa : 0.0f;
  float vec = on ? wa * (ra - ya) : 0.0f;
  v2 acc[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      acc[p][k] = v2{8 * p + 2 * k == lane ? sw : 0.0f, 8 * p + 2 * k + 1 == lane ? sw : 0.0f};
  for (int j = 0; j < ny; ++j) {
    const float* row = CT + j * LD;
    const float cb = row[b], wj = WV[j];
    const v2 cb2 = v2{cb, cb}, wj2 = v2{wj, wj};
    vec = vec + cb * GV[j];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float4 c0 = *reinterpret_cast<const float4*>(row + 8 * p), c1 = *reinterpret_cast<const float4*>(row + 8 * p + 4);
      acc[p][0] = acc[p][0] + (v2{c0.x, c0.y} * cb2) * wj2; acc[p][1] = acc[p][1] + (v2{c0.z, c0.w} * cb2) * wj2;
      acc[p][2] = acc[p][2] + (v2{c1.x, c1.y} * cb2) * wj2; acc[p][3] = acc[p][3] + (v2{c1.z, c1.w} * cb2) * wj2;
    }
  }
  if (lane < NX) q.lx[ro * NX + lane] = vec;
  else if (lane < NC && cu) q.lu[rc * NU + lane - NX] = vec;
  const int rows = cu ? NC : NX;                 // (index T has no ctrl rows)
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int a = 8 * p + r;
      const float v = r & 1 ? acc[p][r / 2].y : acc[p][r / 2].x;
      if (a < NX) {
        if (lane < NX) q.lxx[(ro * NX + a) * NX + lane] = v;
      } else if (a < rows) {
        if (lane < NX) q.lux[(rc * NU + a - NX) * NX + lane] = v;
        else if (lane < NC) q.luu[(rc * NU + a - NX) * NU + lane - NX] = v;
      }
    }
}

}  // namespace rsr
