// rsr_cube.hip -- unit of the Airbot cube / sf kernels: env reset and step, and the physics layer's kernels (launch_physics).
#include "rsr_airbot.hpp"
#include "physics/rsr_physics_kernels.hpp"

namespace rsr {

int launch_cube(int op, const Launch& x) {
  using C = CubeDims;
  switch (op) {
    case OP_RESET: hipLaunchKernelGGL((reset_kernel<C, ENV_CUBE>), dim3(x.grid), dim3(64), sizeof(Smem<C>), x.stream, x.dm, x.L, x.a); return 0;
    case OP_STEP: hipLaunchKernelGGL((step_kernel<C, ENV_CUBE>), dim3(x.grid), dim3(64), sizeof(Smem<C>), x.stream, x.dm, x.L, x.a, x.sc); return 0;
    case OP_STEP_OCCUPANCY: return step_occupancy(step_kernel<C, ENV_CUBE>, sizeof(Smem<C>));
    default: return launch_physics<C, RSR_WAVES_PER_EU>(op, x);      // a physics op, or -1: an op the unit does not know
  }
}

}  // namespace rsr
