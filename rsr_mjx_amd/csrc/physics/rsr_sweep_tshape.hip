// rsr_sweep_tshape.hip -- sweep unit of the Airbot T-shape kernels: sweep_kernel (rsr_sweep.hpp) beside rsr_tshape.hip, same flags.
#include "../rsr_airbot.hpp"
#include "rsr_sweep.hpp"

namespace rsr {

int launch_sweep_tshape(const Launch& x, const SweepArgs& sw) {
  using C = TShapeDims;
  auto go = [&](auto kernel, auto... args) { hipLaunchKernelGGL(kernel, dim3(x.grid), dim3(64), sizeof(Smem<C>), x.stream, x.dm, x.L, x.a, x.ph.p, x.ph.r, sw, args...); return 0; };
  return x.ph.ap.xfrc ? go(sweep_kernel<C, RSR_WAVES_PER_EU, Applied>, x.ph.ap) : go(sweep_kernel<C, RSR_WAVES_PER_EU>);
}

}  // namespace rsr
