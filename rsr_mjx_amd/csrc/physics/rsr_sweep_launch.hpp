// rsr_sweep_launch.hpp -- the launch of rsr_physics_param_rollouts (include/rsr_physics.h): its arguments and the entry of each
// sweep unit (physics/rsr_sweep_cube.hip, rsr_sweep_tshape.hip, rsr_sweep_go2.hip), one per model family beside the family unit
// and built with its flags.  An op in all but the enum: PhysOp and launch_physics (rsr_physics.hpp, rsr_physics_kernels.hpp) are
// pinned at their eight ops by tests/test_dynamics_api.py, so the launch has units of its own until that test next changes
// (DESIGN.md 4j); the host picks the unit by the model's family in one place (sweep_launch in rsr_physics.hip).
#pragma once
#include "../rsr_launch.hpp"

namespace rsr {

// What sweep_kernel takes beside sample_kernel's arguments (PhysArgs p, RollArgs r, and Applied while the forces are on).
struct SweepArgs {
  const float* leaf[RSR_DR_COUNT];   // per-sample leaves [M][K][width], indexed by enum rsr_dr_field; null: the env's own leaf
  int K;                             // samples per slot
  int ctrl_per_sample;               // r.ctrl is [M][K][T][nu]; 0: [M][T][nu], shared by a slot's K samples
};

// each launches sweep_kernel of its family on x.grid = slots x K workgroups (x.ph.p, x.ph.r, x.ph.ap as OP_PHYS_SAMPLE) and returns 0
int launch_sweep_cube(const Launch& x, const SweepArgs& sw);
int launch_sweep_tshape(const Launch& x, const SweepArgs& sw);
int launch_sweep_go2(const Launch& x, const SweepArgs& sw);

}  // namespace rsr
