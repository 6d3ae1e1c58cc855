// rsr_sweep_go2.hip -- sweep unit of the Go2 kernels: sweep_kernel (rsr_sweep.hpp) beside rsr_go2.hip, same flags; the Dims are
// picked as launch_go2 picks them.
#include "../rsr_go2.hpp"
#include "rsr_sweep.hpp"

namespace rsr {

template <class C, int WAVES>
static int launch_dims(const Launch& x, const SweepArgs& sw) {
  auto go = [&](auto kernel, auto... args) { hipLaunchKernelGGL(kernel, dim3(x.grid), dim3(64), sizeof(Smem<C>), x.stream, x.dm, x.L, x.a, x.ph.p, x.ph.r, sw, args...); return 0; };
  return x.ph.ap.xfrc ? go(sweep_kernel<C, WAVES, Applied>, x.ph.ap) : go(sweep_kernel<C, WAVES>);
}

int launch_sweep_go2(const Launch& x, const SweepArgs& sw) {
  if (x.env_kind == ENV_GO2_HANDSTAND) return launch_dims<HandDims, RSR_HS_WAVES_PER_EU>(x, sw);
  if (x.hfield) return launch_dims<Go2Dims, RSR_GO2_WAVES_PER_EU>(x, sw);
  return launch_dims<Go2FlatDims, RSR_GO2_WAVES_PER_EU>(x, sw);
}

}  // namespace rsr
