// rsr_host.hpp -- what the two host units share (rsr_mjx.hip: the C ABI of include/rsr_mjx.h; physics/rsr_physics.hip: that of
// include/rsr_physics.h): the model and batch structs, error reporting, what the host knows of each kernel family (KernelSpec), and
// the dispatch of launches to the family units.
#pragma once
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "rsr_launch.hpp"

using rsr::DModel;
using rsr::Layout;

int fail(int code, const std::string& msg);        // sets rsr_last_error, returns code
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(RSR_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace rsr {
// the unit holding an env kind's kernels
enum Family { FAMILY_CUBE, FAMILY_TSHAPE, FAMILY_GO2 };

// What the host needs to know of the kernels an env kind runs, read off their Dims once (spec_of): the dimensions a model must
// have, the structure rsr_model_create checks it for, and the sizes the record layout and rsr_model_dims report.
struct KernelSpec {
  Family family;
  int nq, nv, nu, nb, nj, ng, ns, np, neq, nf, nl, obs, nmet;     // a model fits when it has exactly these
  int nga, condim;                       // geom slots of the LDS image; the condim of every contact pair
  int tree1, tree2;                      // tree1 > 0: separate kinematic trees over dofs [0, tree1), [tree1, tree2), [tree2, nv)
  int iso0, iso1;                        // iso1 > iso0: dofs [iso0, iso1) decoupled from the rest
  bool arrow; int ant, alegn, alegs;     // block-arrow factorisation: ant trunk dofs carrying alegs legs of alegn dofs
  bool hfield;                           // sphere / height-field pairs are compiled in
  int ncon, nefc, lds_bytes;
  int ninfo, priv;                       // floats of the record's Go2 info block and of each privileged-obs block
  constexpr auto tie() const {           // every field, for comparing two specs
    return std::tie(family, nq, nv, nu, nb, nj, ng, ns, np, neq, nf, nl, obs, nmet, nga, condim, tree1, tree2, iso0, iso1, arrow, ant, alegn,
                    alegs, hfield, ncon, nefc, lds_bytes, ninfo, priv);
  }
};
template <class C>
constexpr KernelSpec spec_of(Family family) {
  return {family, C::NQ, C::NV, C::NU, C::NB, C::NJ, C::NG, C::NS, C::NP, C::NEQ, C::NF, C::NL, C::OBS, C::NMET,
          C::NGA, C::CONDIM, C::TREE1, C::TREE2, C::ISO0, C::ISO1, C::ARROW, C::ANT, C::ALEGN, C::ALEGS, C::HFIELD,
          C::NCON, C::NEFC, (int)sizeof(Smem<C>), C::NINFO, C::NINFO > 0 ? GO2_PRIV : 0};
}
// the spec of an env kind, or null: no kernel is built for it.  The only host code that names the Dims types (rsr_mjx.hip).
const KernelSpec* kernel_spec(int env_kind);
}  // namespace rsr

struct blob_entry { char name[40]; int32_t dtype, count, offset, reserved; };

struct rsr_model {
  std::vector<char> blob;
  rsr_dims dims;
  Layout layout;
  const rsr::KernelSpec* spec = nullptr;      // of dims.env_kind; set once rsr_model_create has accepted the model
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


rsr::StepArgs make_args(rsr_batch* b);
// the batch's launch arguments: grid = envs, its model view, record layout and StepArgs, on the caller's stream
rsr::Launch launch_args(rsr_batch* b, void* hip_stream);
// op (rsr::Op or rsr::PhysOp) by the family unit of the batch's model (KernelSpec::family); returns what the unit's launch entry returns
int launch(const rsr_batch* b, int op, const rsr::Launch& x);
