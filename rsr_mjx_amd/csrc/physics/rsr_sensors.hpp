// rsr_sensors.hpp -- the sensor stage of the physics kernels (rsr_physics_set_sensors, include/rsr_physics.h): data.sensordata of
// a table of site sensors, from what the last forward pass left in LDS.  It reuses the Go2 sensor code of rsr_go2_sensors.hpp
// (go2_sensors / go2_accelerometer), expression for expression, so that the IMU sensors equal the env's privileged_state bit for bit.
#pragma once
#include "../rsr_go2_sensors.hpp"
#include "rsr_physics.hpp"

namespace rsr {

__device__ __forceinline__ V3 site_rt(const float* R, V3 x) {      // R^T x, in go2_sensors' expression order
  return v3(R[0] * x.x + R[3] * x.y + R[6] * x.z, R[1] * x.x + R[4] * x.y + R[7] * x.z, R[2] * x.x + R[5] * x.y + R[8] * x.z);
}
__device__ __forceinline__ float pick_v3(V3 x, int c) { return c == 0 ? x.x : (c == 1 ? x.y : x.z); }

// go2_accelerometer for any site on the IMU's body (the body whose bias s.accb the kernels keep): the same arithmetic with the
// site in place of env_ids[0].  Wave-cooperative; every lane gets the result.
template <class C>
__device__ __forceinline__ V3 site_accelerometer(const DModel& m, const Smem<C>& s, int lane, float qacc_i, int site) {
  const int b = m.site_bodyid[site];
  const bool on = lane < C::NV && ((m.body_dofmask[b] >> lane) & 1);
  float c6[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) c6[c] = on ? s.cdof[6 * lane + c] * qacc_i : 0.0f;
  wave_sum3(c6[0], c6[1], c6[2]); wave_sum3(c6[3], c6[4], c6[5]);
#pragma unroll
  for (int c = 0; c < 6; ++c) c6[c] += s.accb[c];
  V3 dif = ld3(&s.spos[3 * site]) - ld3(&s.com[3 * m.body_rootid[b]]);
  V3 ang = v3(c6[0], c6[1], c6[2]), lin = v3(c6[3], c6[4], c6[5]) + cross(ang, dif);
  const float* R = &s.smat[9 * site];
  V3 w = ld3(&s.sangvel[3 * site]), v = ld3(&s.slinvel[3 * site]);
  auto rt = [&](V3 x) { return v3(R[0] * x.x + R[3] * x.y + R[6] * x.z, R[1] * x.x + R[4] * x.y + R[7] * x.z, R[2] * x.x + R[5] * x.y + R[8] * x.z); };
  V3 al = rt(lin), wl = rt(w), vl = rt(v), cr = cross(wl, vl);
  return v3(al.x + cr.x, al.y + cr.y, al.z + cr.z);
}

// Sensor element `lane` (lanes < sa.nsd hold one each; the others return 0).  Called by all lanes, after the forward pass whose
// outputs it reads (site frames, site velocities, xquat, cdof / com / accb) and after a barrier.  qacc_i: this lane's qacc of
// that pass.
template <class C>
__device__ __forceinline__ float sensor_stage(const DModel& m, const Smem<C>& s, int lane, float qacc_i, const SensArgs& sa) {
  V3 acc = v3(0.0f, 0.0f, 0.0f);
  if constexpr (C::XFRC) {
    if (sa.acc_site >= 0) {                        // wave-uniform
      if (sa.acc_site == m.env_ids[0]) {
        G2Sens sn;
        go2_accelerometer<C>(m, s, lane, qacc_i, sn);
        acc = v3(sn.accel[0], sn.accel[1], sn.accel[2]);
      } else {
        acc = site_accelerometer<C>(m, s, lane, qacc_i, sa.acc_site);
      }
    }
  }
  if (lane >= sa.nsd) return 0.0f;
  const int4 el = sa.el[lane];
  const int site = el.y, ref = el.z, c = el.w;
  const float* R = &s.smat[9 * site];
  switch (el.x) {
    case RSR_S_GYRO: return pick_v3(site_rt(R, ld3(&s.sangvel[3 * site])), c);
    case RSR_S_VELOCIMETER: return pick_v3(site_rt(R, ld3(&s.slinvel[3 * site])), c);
    case RSR_S_ACCELEROMETER: return pick_v3(acc, c);
    case RSR_S_FRAMEPOS: {
      const V3 p = ld3(&s.spos[3 * site]);
      return pick_v3(ref >= 0 ? site_rt(&s.smat[9 * ref], p - ld3(&s.spos[3 * ref])) : p, c);
    }
    case RSR_S_FRAMEXAXIS: return R[3 * c];
    case RSR_S_FRAMEZAXIS: return R[3 * c + 2];
    case RSR_S_FRAMEQUAT: {
      const Q4 q = qmul(ld4(&s.xquat[4 * m.site_bodyid[site]]),
                        Q4{m.site_quat[4 * site], m.site_quat[4 * site + 1], m.site_quat[4 * site + 2], m.site_quat[4 * site + 3]});
      return c == 0 ? q.w : (c == 1 ? q.x : (c == 2 ? q.y : q.z));
    }
    case RSR_S_FRAMELINVEL: return s.slinvel[3 * site + c];
    case RSR_S_FRAMEANGVEL: return s.sangvel[3 * site + c];
    default: return 0.0f;
  }
}

}  // namespace rsr
