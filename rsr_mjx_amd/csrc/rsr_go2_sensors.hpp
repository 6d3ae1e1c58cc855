// rsr_go2_sensors.hpp -- the Go2 IMU sensors (gyro, velocimeter, gravity, accelerometer) from what the last forward pass left in
// LDS: the env kernels' observations and the physics kernels' sensor stage (physics/rsr_sensors.hpp) share them.
#pragma once
#include "rsr_env.hpp"

namespace rsr {

struct G2Sens { float gyro[3], linvel[3], gravity[3], up[3], glin[3], gang[3], accel[3]; };
// element i (0..2, a lane index) of a sensor triple by selects: indexing the register array with a lane index would put the
// whole struct into scratch memory
// (the three values pass through an empty asm: a select between loads of the struct would be rewritten into one load through
// a selected address, which pins the struct in memory just the same)
__device__ __forceinline__ float pick3(const float (&v)[3], int i) {
  float a = v[0], b = v[1], c = v[2];
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
  return i == 0 ? a : (i == 1 ? b : c);
}

template <class C>
__device__ __forceinline__ void go2_sensors(const DModel& m, const Smem<C>& s, G2Sens& o) {
  const int imu = m.env_ids[0];
  const float* R = &s.smat[9 * imu];
  V3 w = ld3(&s.sangvel[3 * imu]), v = ld3(&s.slinvel[3 * imu]);
  // site-frame quantities: R^T x
  o.gyro[0] = R[0] * w.x + R[3] * w.y + R[6] * w.z; o.gyro[1] = R[1] * w.x + R[4] * w.y + R[7] * w.z; o.gyro[2] = R[2] * w.x + R[5] * w.y + R[8] * w.z;
  o.linvel[0] = R[0] * v.x + R[3] * v.y + R[6] * v.z; o.linvel[1] = R[1] * v.x + R[4] * v.y + R[7] * v.z; o.linvel[2] = R[2] * v.x + R[5] * v.y + R[8] * v.z;
  o.gravity[0] = R[0] * 0.0f + R[3] * 0.0f + R[6] * -1.0f; o.gravity[1] = R[1] * 0.0f + R[4] * 0.0f + R[7] * -1.0f; o.gravity[2] = R[2] * 0.0f + R[5] * 0.0f + R[8] * -1.0f;
  o.up[0] = R[2]; o.up[1] = R[5]; o.up[2] = R[8];
  o.glin[0] = v.x; o.glin[1] = v.y; o.glin[2] = v.z; o.gang[0] = w.x; o.gang[1] = w.y; o.gang[2] = w.z;
}

// accelerometer of the IMU site (MuJoCo sensor_acc: rne_postconstraint cacc + objectAcceleration, local frame):
// cacc = accb (velocity-product part saved by smooth_forces) + sum over the body's chain of cdof * qacc, moved to the site
// (lin + ang x dif), rotated into the site frame, plus w_local x v_local.  Wave-cooperative; every lane gets the result.
template <class C>
__device__ __forceinline__ void go2_accelerometer(const DModel& m, const Smem<C>& s, int lane, float qacc_i, G2Sens& o) {
  const int imu = m.env_ids[0], b = m.site_bodyid[imu];
  const bool on = lane < C::NV && ((m.body_dofmask[b] >> lane) & 1);
  float c6[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) c6[c] = on ? s.cdof[6 * lane + c] * qacc_i : 0.0f;
  wave_sum3(c6[0], c6[1], c6[2]); wave_sum3(c6[3], c6[4], c6[5]);
#pragma unroll
  for (int c = 0; c < 6; ++c) c6[c] += s.accb[c];
  V3 dif = ld3(&s.spos[3 * imu]) - ld3(&s.com[3 * m.body_rootid[b]]);
  V3 ang = v3(c6[0], c6[1], c6[2]), lin = v3(c6[3], c6[4], c6[5]) + cross(ang, dif);
  const float* R = &s.smat[9 * imu];
  V3 w = ld3(&s.sangvel[3 * imu]), v = ld3(&s.slinvel[3 * imu]);
  auto rt = [&](V3 x) { return v3(R[0] * x.x + R[3] * x.y + R[6] * x.z, R[1] * x.x + R[4] * x.y + R[7] * x.z, R[2] * x.x + R[5] * x.y + R[8] * x.z); };
  V3 al = rt(lin), wl = rt(w), vl = rt(v), cr = cross(wl, vl);
  o.accel[0] = al.x + cr.x; o.accel[1] = al.y + cr.y; o.accel[2] = al.z + cr.z;
}

}  // namespace rsr
