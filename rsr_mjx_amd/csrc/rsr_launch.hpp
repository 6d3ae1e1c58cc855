// rsr_launch.hpp -- the launch entry of each family unit.  The library is three units of kernels, one per model family, each with
// its own flags (rsr_mjx_amd/build.py): rsr_cube.hip (Airbot cube / sf), rsr_tshape.hip (Airbot T-shape), rsr_go2.hip (Go2 joystick,
// flat or on a height field, and handstand / footstand).  Each exports one function that launches its kernels; the host picks the
// unit from the model's KernelSpec (rsr_host.hpp) in one place (launch in rsr_mjx.hip).
#pragma once
#include "rsr_env.hpp"
#include "physics/rsr_physics.hpp"

namespace rsr {

// The env ops.  The physics ops are enum PhysOp (physics/rsr_physics.hpp), whose values start above these: an entry takes either.
enum Op {
  OP_RESET,              // rsr_reset: grid = envs
  OP_STEP,               // rsr_step: the Airbot units' persistent work-queue grid (sc), the Go2 unit's grid = envs
  OP_STEP_OCCUPANCY,     // returns the resident workgroups per CU of the step kernel (0: unknown); launches nothing
};

struct Launch {
  int grid;
  hipStream_t stream;
  const DModel* dm;     // device model view
  Layout L;
  StepArgs a;
  Sched sc;             // OP_STEP of the Airbot units
  PhysLaunch ph;        // the physics ops, each its own field
  int env_kind;         // the Go2 unit's pick: handstand / footstand, or the joystick with (hfield) or without the height field
  bool hfield;
};

// each returns 0, or what its op says above; -1: an op the unit does not know (nothing is launched)
int launch_cube(int op, const Launch& x);
int launch_tshape(int op, const Launch& x);
int launch_go2(int op, const Launch& x);

template <class K>
int step_occupancy(K kernel, size_t lds) {
  int per_cu = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, lds) == hipSuccess ? per_cu : 0;
}

}  // namespace rsr
