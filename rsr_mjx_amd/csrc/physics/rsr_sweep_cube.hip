// rsr_sweep_cube.hip -- sweep unit of the Airbot cube / sf kernels: sweep_kernel (rsr_sweep.hpp) beside rsr_cube.hip, same flags.
#include "../rsr_airbot.hpp"
#include "rsr_sweep.hpp"

namespace rsr {

int launch_sweep_cube(const Launch& x, const SweepArgs& sw) {
  using C = CubeDims;
  auto go = [&](auto kernel, auto... args) { hipLaunchKernelGGL(kernel, dim3(x.grid), dim3(64), sizeof(Smem<C>), x.stream, x.dm, x.L, x.a, x.ph.p, x.ph.r, sw, args...); return 0; };
  return x.ph.ap.xfrc ? go(sweep_kernel<C, RSR_WAVES_PER_EU, Applied>, x.ph.ap) : go(sweep_kernel<C, RSR_WAVES_PER_EU>);
}

}  // namespace rsr
