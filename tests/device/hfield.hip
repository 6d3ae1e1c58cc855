// hfield.hip -- TEST ONLY: the height-field narrow phase of rsr_device.hpp (hfield_place / hfield_search<NPAIR> / hfield_finish,
// closest_on_triangle) run one wave per problem, for tests/test_device_hfield*.py (loader: tests/device_harness.py).  One wave
// handles NPAIR = Go2Dims::NP spheres against one field in collision()'s own sequence; the DModel it hands to the product's
// functions has only its hfield_* members set (they read nothing else).  The one thing written here rather than called is the
// serial scan the header names as hfield_search's bit reference.  Built into tests/device/_build/, never into the product library.
#include <hip/hip_runtime.h>

#include "../../rsr_mjx_amd/csrc/rsr_env.hpp"

namespace {
using namespace rsr;

constexpr int NPAIR = Go2Dims::NP;
constexpr float SENTINEL = -7.25f;        // what the job's fields hold where hfield_place writes nothing

struct Field { const float *size, *data; const int *nrow, *ncol; };      // device pointers: size[4], data[nrow * ncol]
struct Spheres { const float *hpos, *hmat, *spos, *radius; };            // [n][3], [n][9], [n][NPAIR][3], [n][NPAIR]
struct JobOut {
  int* ji;       // [n][NPAIR][4]: state, c0, r0, 1 when the wave ran hfield_search
  float* jf;     // [n][NPAIR][16]: p (3), q (3), n (3), dist, best after the search; q (3), best before it
};

__device__ __forceinline__ DModel field_model(const Field& f) {
  DModel m;      // (only these four are read; everything else stays unset and is never touched)
  m.hfield_size = (gp_f)f.size; m.hfield_data = (gp_f)f.data; m.hfield_nrow = (gp_i)f.nrow; m.hfield_ncol = (gp_i)f.ncol;
  return m;
}

__device__ __forceinline__ HfJob blank_job() {
  HfJob j;
  j.state = 0; j.p = j.q = j.n = v3(SENTINEL, SENTINEL, SENTINEL); j.dist = j.best = SENTINEL; j.c0 = j.r0 = -1;
  return j;
}

// the pair lanes place, every lane searches when any pair has state 2, the pair lanes finish: collision()'s sequence
__global__ __launch_bounds__(64) void contact_kernel(Field f, Spheres s, JobOut o, int* flag, float* dist, float* pos, float* nrm) {
  const int lane = threadIdx.x, w = blockIdx.x;
  const DModel m = field_model(f);
  HfJob hf = blank_job();
  const V3 hpos = v3(s.hpos[3 * w], s.hpos[3 * w + 1], s.hpos[3 * w + 2]);
  const float* hmat = s.hmat + 9 * w;
  const size_t pr = (size_t)w * NPAIR + (lane < NPAIR ? lane : 0);
  const float radius = s.radius[pr];
  if (lane < NPAIR) hfield_place(m, hpos, hmat, v3(s.spos[3 * pr], s.spos[3 * pr + 1], s.spos[3 * pr + 2]), radius, hf);
  const HfJob pre = hf;
  const bool any = __ballot(hf.state == 2) != 0ull;
  if (any) hfield_search<NPAIR>(m, lane, hf);
  if (lane < NPAIR) {
    float d = 0.0f; V3 p = v3(0, 0, 0), n = v3(0, 0, 0);
    bool hit = false;
    if (hf.state != 0) hit = hfield_finish(hpos, hmat, radius, hf, d, p, n);
    flag[pr] = hit ? 1 : 0; dist[pr] = d;
    pos[3 * pr] = p.x; pos[3 * pr + 1] = p.y; pos[3 * pr + 2] = p.z;
    nrm[3 * pr] = n.x; nrm[3 * pr + 1] = n.y; nrm[3 * pr + 2] = n.z;
    int* ji = o.ji + 4 * pr; float* jf = o.jf + 16 * pr;
    ji[0] = hf.state; ji[1] = hf.c0; ji[2] = hf.r0; ji[3] = any ? 1 : 0;
    const float v[16] = {hf.p.x, hf.p.y, hf.p.z, hf.q.x, hf.q.y, hf.q.z, hf.n.x, hf.n.y, hf.n.z, hf.dist, hf.best,
                         pre.q.x, pre.q.y, pre.q.z, pre.best, 0.0f};
#pragma unroll
    for (int c = 0; c < 16; ++c) jf[c] = v[c];
  }
}

// THE SERIAL SCAN: the pair's lane walks the eight triangles k = 0..7 = bits (row, column, half) of its 2 x 2 cells with the
// product's closest_on_triangle and keeps a candidate only when it is strictly closer.  Vertices as hfield_search forms them.
// (Bit for bit with hfield_search only where the compiler may not contract a * b + c: see UNITS in tests/device_harness.py.)
__global__ __launch_bounds__(64) void scan_kernel(Field f, Spheres s, int* state, float* q, float* best) {
  const int lane = threadIdx.x, w = blockIdx.x;
  if (lane >= NPAIR) return;
  const DModel m = field_model(f);
  HfJob hf = blank_job();
  const size_t pr = (size_t)w * NPAIR + lane;
  hfield_place(m, v3(s.hpos[3 * w], s.hpos[3 * w + 1], s.hpos[3 * w + 2]), s.hmat + 9 * w,
               v3(s.spos[3 * pr], s.spos[3 * pr + 1], s.spos[3 * pr + 2]), s.radius[pr], hf);
  float bv = 3.0e38f; V3 bq = hf.p;
  if (hf.state == 2) {
    const int ncol = m.hfield_ncol[0], nrow = m.hfield_nrow[0];
    const float sx = m.hfield_size[0], sy = m.hfield_size[1], sz = m.hfield_size[2];
    const float* __restrict__ data = m.hfield_data;
    const float dx = 2.0f * sx / (float)(ncol - 1), dy = 2.0f * sy / (float)(nrow - 1);
    const V3 p = hf.p;
    for (int k = 0; k < 8; ++k) {
      const int cc = hf.c0 + ((k >> 1) & 1), rr = hf.r0 + (k >> 2);
      float xa = -sx + dx * (float)cc, ya = -sy + dy * (float)rr, xb = xa + dx, yb = ya + dy;
      V3 v00 = v3(xa, ya, data[rr * ncol + cc] * sz), v10 = v3(xb, ya, data[rr * ncol + cc + 1] * sz);
      V3 v01 = v3(xa, yb, data[(rr + 1) * ncol + cc] * sz), v11 = v3(xb, yb, data[(rr + 1) * ncol + cc + 1] * sz);
      const V3 c = (k & 1) ? closest_on_triangle(p, v00, v11, v01) : closest_on_triangle(p, v00, v10, v11);
      const V3 d = p - c; const float d2 = dot(d, d);
      if (d2 < bv) { bv = d2; bq = c; }
    }
  }
  state[pr] = hf.state; best[pr] = bv;
  q[3 * pr] = bq.x; q[3 * pr + 1] = bq.y; q[3 * pr + 2] = bq.z;
}

// one lane per (p, a, b, c): in[n][12] -> q[n][3]
__global__ __launch_bounds__(64) void triangle_kernel(int n, const float* in, float* q) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* v = in + 12 * (size_t)i;
  const V3 c = closest_on_triangle(v3(v[0], v[1], v[2]), v3(v[3], v[4], v[5]), v3(v[6], v[7], v[8]), v3(v[9], v[10], v[11]));
  q[3 * (size_t)i] = c.x; q[3 * (size_t)i + 1] = c.y; q[3 * (size_t)i + 2] = c.z;
}

int finish_launch() {
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return (int)err;
}
}  // namespace

extern "C" {

// spheres per wave (Go2Dims::NP)
int rsr_hf_npair(void) { return NPAIR; }

// n waves of NPAIR spheres against one field.  Device pointers; nrow / ncol are device ints, >= 3 each (as the host's check_hfield
// demands of a model).  Returns 0, a hipError_t, or -1 for a bad count.
int rsr_hf_contact(int n, const float* size, const float* data, const int* nrow, const int* ncol, const float* hpos, const float* hmat,
                   const float* spos, const float* radius, int* flag, float* dist, float* pos, float* nrm, int* job_i, float* job_f) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(contact_kernel, dim3(n), dim3(64), 0, 0, Field{size, data, nrow, ncol}, Spheres{hpos, hmat, spos, radius},
                     JobOut{job_i, job_f}, flag, dist, pos, nrm);
  return finish_launch();
}

// hfield_place + the serial scan on the same inputs: state[n][NPAIR], q[n][NPAIR][3], best[n][NPAIR] (q = p, best = 3e38 where
// the pair does not search)
int rsr_hf_scan(int n, const float* size, const float* data, const int* nrow, const int* ncol, const float* hpos, const float* hmat,
                const float* spos, const float* radius, int* state, float* q, float* best) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(scan_kernel, dim3(n), dim3(64), 0, 0, Field{size, data, nrow, ncol}, Spheres{hpos, hmat, spos, radius}, state, q, best);
  return finish_launch();
}

int rsr_hf_triangle(int n, const float* in, float* q) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(triangle_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, in, q);
  return finish_launch();
}

}  // extern "C"
