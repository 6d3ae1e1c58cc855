// rsr_host.hpp -- what the two host units share (rsr_mjx.hip: the C ABI of include/rsr_mjx.h; physics/rsr_physics.hip: that of
// include/rsr_physics.h): the model and batch structs, error reporting, and the dispatch of launches to the family units.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "rsr_launch.hpp"

using rsr::DModel;
using rsr::Layout;

int fail(int code, const std::string& msg);        // sets rsr_last_error, returns code
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(RSR_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

struct blob_entry { char name[40]; int32_t dtype, count, offset, reserved; };

struct rsr_model {
  std::vector<char> blob;
  rsr_dims dims;
  Layout layout;
  bool has_hfield = false;      // any PAIR_HFIELD_SPHERE pair: the Go2 kernels with the height-field narrow phase
  const void* find(const char* name, int* count = nullptr) const {
    const int32_t* h = reinterpret_cast<const int32_t*>(blob.data());
    const blob_entry* e = reinterpret_cast<const blob_entry*>(blob.data() + 16);
    for (int i = 0; i < h[2]; ++i)
      if (std::strncmp(e[i].name, name, 40) == 0) { if (count) *count = e[i].count; return blob.data() + e[i].offset; }
    if (count) *count = 0;
    return nullptr;
  }
  ptrdiff_t offset_of(const char* name) const {
    const void* p = find(name);
    return p ? static_cast<const char*>(p) - blob.data() : -1;
  }
};

struct rsr_batch {
  const rsr_model* model;
  int n, device;
  float* state; bool owns_state;
  char* dblob;
  DModel dm;            // host copy of the device model view
  DModel* dmodel;       // the same struct in device memory (kernels take a pointer: fewer live SGPRs)
  const float *dr_fric, *dr_mass, *dr_damp, *dr_floss;
  const float* dr_ex[5];    // body_ipos, qpos0, dof_armature, actuator_gainprm, actuator_biasprm
  float* debug;
  hipEvent_t ev0, ev1; bool timing; int launches;
  // work-queue dispatch of the Airbot step kernels (rsr_device.hpp: Sched)
  int* sched;           // device: ticket[2], err[2], then flags[n]
  unsigned launch_id;
  int units, step_grid;
  int spin_cap, withhold_env;   // rsr_batch_set_fault_injection (test hook)
  int whole_envs;               // rsr_batch_set_whole_envs: envs stepped as one unit each (-1: all but two resident rounds' worth)
  int prio_policy, prio_slots;  // rsr_batch_set_priority (-1: chosen from the batch size per launch); resident waves of the step kernel
  int action_repeat;            // rsr_batch_set_action_repeat (1: the wrappers fused in the step kernels)
  DModel* dmodel_plain;         // device copy of the model view with the wrapper flags cleared (action_repeat > 1), or null
  float* racc;                  // [n] reward sums of the repeats, or null
};

namespace rsr {
// the unit holding an env kind's kernels: the only place that maps env kinds to kernels
enum Family { FAMILY_NONE = -1, FAMILY_CUBE, FAMILY_TSHAPE, FAMILY_GO2 };
Family family_of(int env_kind);
}  // namespace rsr

rsr::StepArgs make_args(rsr_batch* b);
// the batch's launch arguments: grid = envs, its model view, record layout and StepArgs, on the caller's stream
rsr::Launch launch_args(rsr_batch* b, void* hip_stream);
// op (rsr::Op) by the family unit of the batch's env kind; returns what the unit's launch entry returns
int launch(const rsr_batch* b, int op, const rsr::Launch& x);
