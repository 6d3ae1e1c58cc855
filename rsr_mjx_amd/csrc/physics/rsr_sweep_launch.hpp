// rsr_sweep_launch.hpp -- the launch of rsr_physics_param_rollouts and rsr_physics_feedback_rollouts (include/rsr_physics.h): its arguments and the entry of each
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
  // rsr_physics_feedback_rollouts (rsr_feedback.hpp); fb_gain null: open loop, r.ctrl is applied as it stands
  const float* fb_gain;              // [M][T][nu][2 nv], or with fb_per_sample [M][K][T][nu][2 nv]
  const float* fb_qpos;              // [..][T][nq]
  const float* fb_qvel;              // [..][T][nv]
  float* ctrl_out;                   // [M][K][T][nu] the applied ctrl, or null
  int fb_per_sample;                 // the three feedback rows are per sample
  int fb_clamp;                      // clamp to actuator_ctrlrange where actuator_ctrllimited
};

// each launches sweep_kernel of its family on x.grid = slots x K workgroups (x.ph.p, x.ph.r, x.ph.ap as OP_PHYS_SAMPLE) and returns 0
int launch_sweep_cube(const Launch& x, const SweepArgs& sw);
int launch_sweep_tshape(const Launch& x, const SweepArgs& sw);
int launch_sweep_go2(const Launch& x, const SweepArgs& sw);

}  // namespace rsr
