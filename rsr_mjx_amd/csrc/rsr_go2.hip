// rsr_go2.hip -- unit of the Go2 kernels: joystick on a plane (Go2FlatDims) or a height field (Go2Dims), handstand / footstand
// (HandDims); env reset and step, and the physics layer's kernels (launch_physics) of each.
#include "rsr_go2.hpp"
#include "physics/rsr_physics_kernels.hpp"

namespace rsr {

using EnvKernel = void (*)(const DModel*, Layout, StepArgs);

template <class C, int WAVES>
static int launch_dims(int op, const Launch& x, EnvKernel reset, EnvKernel step) {
  switch (op) {
    case OP_RESET: hipLaunchKernelGGL(reset, dim3(x.grid), dim3(64), sizeof(Smem<C>), x.stream, x.dm, x.L, x.a); return 0;
    case OP_STEP: hipLaunchKernelGGL(step, dim3(x.grid), dim3(64), sizeof(Smem<C>), x.stream, x.dm, x.L, x.a); return 0;
    case OP_STEP_OCCUPANCY: return step_occupancy(step, sizeof(Smem<C>));
    default: return launch_physics<C, WAVES>(op, x);      // a physics op, or -1: an op the unit does not know
  }
}

int launch_go2(int op, const Launch& x) {
  static_assert(sizeof(Smem<Go2FlatDims>) == sizeof(Smem<Go2Dims>), "one LDS image for both Go2 joystick kernels (rsr_model_dims reports it)");
  if (x.env_kind == ENV_GO2_HANDSTAND) return launch_dims<HandDims, RSR_HS_WAVES_PER_EU>(op, x, hs_reset_kernel<HandDims>, hs_step_kernel<HandDims>);
  if (x.hfield) return launch_dims<Go2Dims, RSR_GO2_WAVES_PER_EU>(op, x, go2_reset_kernel<Go2Dims>, go2_step_kernel<Go2Dims>);
  return launch_dims<Go2FlatDims, RSR_GO2_WAVES_PER_EU>(op, x, go2_reset_kernel<Go2FlatDims>, go2_step_kernel<Go2FlatDims>);
}

}  // namespace rsr
