// rsr_mjx.hip -- the C ABI of librsrmjx.so (include/rsr_mjx.h): model and blob parsing, batches, record views, timing, and the
// batch-level kernels (rollout metrics, action repeat).  The env kernels live in the family units (rsr_launch.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "rsr_host.hpp"

namespace rsr {

// ---------------------------------------------------------------- end-of-rollout metric reduction
// One launch instead of a handful of library reductions: out = {envs, sum of reward, sum of done, mean of the running episode's
// summed reward} over the batch, summed in a fixed order (per-thread strided partial sums, then a binary tree in LDS), so the
// result does not depend on timing.  One workgroup: the batch is a few thousand records and the launch is latency bound.
__global__ __launch_bounds__(1024) void rollout_metrics_kernel(const float* __restrict__ state, Layout L, int n, float* __restrict__ out) {
  __shared__ float red[3][1024];
  const int t = threadIdx.x;
  float r = 0.0f, d = 0.0f, em = 0.0f;
  for (int e = t; e < n; e += 1024) {
    const float* rec = state + (size_t)e * L.rec;
    r += rec[L.reward]; d += rec[L.done]; em += rec[L.episode_metrics];
  }
  red[0][t] = r; red[1][t] = d; red[2][t] = em;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; red[2][t] += red[2][t + w]; }
    __syncthreads();
  }
  if (t == 0) { out[0] = (float)n; out[1] = red[0][0]; out[2] = red[1][0]; out[3] = red[2][0] / (float)n; }
}

// ---------------------------------------------------------------- action_repeat > 1 (brax EpisodeWrapper.step: scan of env.step)
// The fused step kernels carry the wrappers for action_repeat = 1, the only value the reference passes (RSR/train.py:81).  For a
// larger value rsr_step runs the step kernels `repeat` times on a copy of the model view with the wrapper flags cleared (plain
// env.step) and these three small kernels carry the wrappers around them: the reward is the sum of the repeats' rewards in order,
// steps and the episode length advance by `repeat`, done / truncation / episode metrics are formed once from the last repeat's
// state, AutoReset restores the first state after that.  One wavefront per env; nothing here is on the reference's hot path.
__global__ __launch_bounds__(64) void repeat_pre_kernel(float* __restrict__ state, Layout L, int n, int wrap_flags, float* __restrict__ racc) {
  const int e = blockIdx.x;
  if (e >= n || threadIdx.x != 0) return;
  float* rec = state + (size_t)e * L.rec;
  if ((wrap_flags & 2) != 0 && rec[L.done] != 0.0f) rec[L.steps] = 0.0f;      // AutoResetWrapper.step pre-step
  racc[e] = 0.0f;
}
__global__ __launch_bounds__(256) void repeat_acc_kernel(const float* __restrict__ state, Layout L, int n, float* __restrict__ racc) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) racc[e] += state[(size_t)e * L.rec + L.reward];
}
__global__ __launch_bounds__(64) void repeat_post_kernel(float* __restrict__ state, Layout L, int n, int wrap_flags, int repeat, int episode_length,
                                                        int nmet, int obs_dim, int priv_dim, int xfrc_at, const float* __restrict__ racc) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= n) return;
  float* rec = state + (size_t)e * L.rec;
  const bool wrap_episode = wrap_flags & 1, wrap_autoreset = (wrap_flags & 2) != 0;
  const float reward = racc[e];
  float done = rec[L.done], steps = rec[L.steps];
  const float prev_done = wrap_episode ? rec[L.episode_done] : 0.0f;
  const float em_old = (wrap_episode && lane < nmet + 2) ? rec[L.episode_metrics + lane] : 0.0f;
  const float met = (lane >= 2 && lane < nmet + 2) ? rec[L.metrics + lane - 2] : 0.0f;
  bool over = false;
  float trunc = 0.0f;
  if (wrap_episode) {
    steps += (float)repeat;
    over = steps >= (float)episode_length;
    trunc = over ? 1.0f - done : 0.0f;
    if (lane < nmet + 2) {
      const float add = lane == 0 ? reward : (lane == 1 ? (float)repeat : met);
      rec[L.episode_metrics + lane] = prev_done != 0.0f ? 0.0f : em_old + add;
    }
  }
  if (over) done = 1.0f;
  __syncthreads();
  if (lane == 0) {
    rec[L.reward] = reward;
    if (wrap_episode) { rec[L.truncation] = trunc; rec[L.episode_done] = done; }
    rec[L.steps] = steps;
    rec[L.done] = done;
  }
  if (wrap_autoreset && done != 0.0f) {
    if (xfrc_at >= 0 && lane < 3) rec[L.go2_info + xfrc_at + lane] = 0.0f;      // data.xfrc_applied goes back with `data`
    for (int t = lane; t < L.persist_end; t += 64) rec[t] = rec[L.f_qpos + t];
    for (int t = lane; t < obs_dim; t += 64) rec[L.obs + t] = rec[L.f_obs + t];
    for (int t = lane; t < priv_dim; t += 64) rec[L.priv_obs + t] = rec[L.f_priv_obs + t];
  }
}
}  // namespace rsr

// =====================================================================================
// host side: C ABI
// =====================================================================================
static thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

const rsr::KernelSpec* rsr::kernel_spec(int env_kind) {
  static constexpr KernelSpec cube = spec_of<CubeDims>(FAMILY_CUBE), tshape = spec_of<TShapeDims>(FAMILY_TSHAPE),
                              go2 = spec_of<Go2Dims>(FAMILY_GO2), go2_flat = spec_of<Go2FlatDims>(FAMILY_GO2), hand = spec_of<HandDims>(FAMILY_GO2);
  // a joystick model is accepted against Go2Dims and runs Go2FlatDims when it has no height-field pair (launch_go2): apart from
  // that stage the host must see one kernel
  constexpr auto but_hfield = [](KernelSpec k) { k.hfield = false; return k; };
  static_assert(go2.hfield && but_hfield(go2).tie() == go2_flat.tie(), "Go2FlatDims is Go2Dims without the height-field stage");
  switch (env_kind) {
    case ENV_CUBE: case ENV_AIRBOT_SF: return &cube;
    case ENV_TSHAPE: return &tshape;
    case ENV_GO2: return &go2;
    case ENV_GO2_HANDSTAND: return &hand;
    default: return nullptr;
  }
}

static bool go2_family(const rsr_model* m) { return m->spec->family == rsr::FAMILY_GO2; }

static Layout make_layout(const rsr_dims& d, const rsr::KernelSpec& k) {
  Layout L{};
  int o = 0;
  auto take = [&](int n) { int r = o; o += n; return r; };
  L.qpos = take(d.nq); L.qvel = take(d.nv); L.ctrl = take(d.nu); L.warm = take(d.nv); L.time = take(1);
  L.xpos = take(d.nbody * 3); L.site_xpos = take(d.nsite * 3);
  L.persist_end = o;
  L.f_qpos = take(d.nq); L.f_qvel = take(d.nv); L.f_ctrl = take(d.nu); L.f_warm = take(d.nv); L.f_time = take(1);
  L.f_xpos = take(d.nbody * 3); L.f_site_xpos = take(d.nsite * 3);
  L.obs = take(d.obs_dim); L.f_obs = take(d.obs_dim);
  L.reward = take(1); L.done = take(1); L.metrics = take(d.nmetrics);
  L.target_pos = take(3); L.new_cube_pos = take(2); L.site_pos = take(3); L.cube_pos = take(3); L.last_action = take(1);
  L.target_base_pos = take(3); L.target_vertical_pos = take(3); L.target_w = take(1); L.new_T_pos = take(2);
  L.T_pos = take(3); L.xita = take(1);
  L.go2_info = take(k.ninfo);
  L.priv_obs = take(k.priv); L.f_priv_obs = take(k.priv);
  L.steps = take(1); L.truncation = take(1); L.episode_done = take(1); L.episode_metrics = take(2 + d.nmetrics);
  L.stats = take(4);
  L.rec = (o + 15) & ~15;
  return L;
}

extern "C" const char* rsr_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------- rsr_model_create: what the kernels of a spec assume of a model
// Each check returns null or why the model is refused (RSR_ERR_UNSUPPORTED); rsr_model_create runs them in the order of `checks`.
namespace {
template <class T>
const T* field(const rsr_model& m, const char* name, int* count = nullptr) { return static_cast<const T*>(m.find(name, count)); }

bool fits(const rsr_dims& d, const int* c2, const rsr::KernelSpec& k) {
  return d.nq == k.nq && d.nv == k.nv && d.nu == k.nu && d.nbody == k.nb && d.njnt == k.nj && d.ngeom == k.ng && d.nsite == k.ns &&
         d.npair == k.np && d.neq == k.neq && c2[0] == k.nf && c2[1] == k.nl && d.obs_dim == k.obs && d.nmetrics == k.nmet;
}

const char* check_joints(rsr_model& m, const rsr::KernelSpec&) {
  return field<int>(m, "counts2")[3] > 1 ? "bodies with more than one joint are not built" : nullptr;
}

// geom slots: as many as the kernel's LDS image keeps, each a geom id, every pair geom among them (model.py: geom_slots)
const char* check_geom_slots(rsr_model& m, const rsr::KernelSpec& k) {
  int ns = 0, np1 = 0;
  const int* gs = field<int>(m, "geom_slot_ids", &ns);
  bool ok = gs && ns == k.nga;
  for (int i = 0; ok && i < ns; ++i) ok = gs[i] >= 0 && gs[i] < k.ng && (k.nga != k.ng || gs[i] == i);
  const int *pg1 = field<int>(m, "pair_geom1", &np1), *pg2 = field<int>(m, "pair_geom2");
  for (int q = 0; ok && q < np1; ++q) {
    bool f1 = false, f2 = false;
    for (int i = 0; i < ns; ++i) { f1 |= gs[i] == pg1[q]; f2 |= gs[i] == pg2[q]; }
    ok = f1 && f2;
  }
  return ok ? nullptr : "geom_slot_ids do not match the kernel's geom slots (Dims::NGA) or miss a pair geom";
}

// the Airbot kernels factor one kinematic tree per DPP row (Dims::ROWTREE): dof ranges [0, TREE1), [TREE1, TREE2), [TREE2, nv)
// must be separate trees -- no body chain and no equality constraint may straddle them
const char* check_trees(rsr_model& m, const rsr::KernelSpec& k) {
  if (k.tree1 <= 0) return nullptr;
  auto trees_of = [&](unsigned mask) {
    const unsigned m0 = (1u << k.tree1) - 1u, m01 = (1u << k.tree2) - 1u;
    return ((mask & m0) != 0u) + ((mask & (m01 & ~m0)) != 0u) + ((mask & ~m01) != 0u);
  };
  int nbm = 0, neq = 0;
  const unsigned* bm = field<unsigned>(m, "body_dofmask", &nbm);
  bool ok = bm != nullptr;
  for (int b = 0; ok && b < nbm; ++b) ok = trees_of(bm[b]) <= 1;
  const int *e1 = field<int>(m, "eq_obj1id", &neq), *e2 = field<int>(m, "eq_obj2id"), *jd = field<int>(m, "jnt_dofadr");
  for (int q = 0; ok && e1 && e2 && jd && q < neq; ++q) {
    const bool j1 = e1[q] >= 0 && e1[q] < k.nj, j2 = e2[q] >= 0 && e2[q] < k.nj;
    if (j1 && j2) ok = trees_of((1u << jd[e1[q]]) | (1u << jd[e2[q]])) <= 1;
  }
  return ok ? nullptr : "the Airbot kernels need the arm and the free bodies as separate kinematic trees over fixed dof ranges";
}

// the Go2 kernels factor M and H in block-arrow form (Dims::ARROW): dofs 0..5 are the trunk, every further group of three dofs
// is a leg, and no body chain and no contact pair may touch two legs
const char* check_arrow(rsr_model& m, const rsr::KernelSpec& k) {
  if (!k.arrow) return nullptr;
  auto legs_of = [&](unsigned mask) {
    int n = 0;
    for (int l = 0; l < k.alegs; ++l) n += ((mask >> (k.ant + k.alegn * l)) & ((1u << k.alegn) - 1u)) != 0u;
    return n;
  };
  int nbm = 0, npm = 0;
  const unsigned* bm = field<unsigned>(m, "body_dofmask", &nbm);
  const unsigned *pm1 = field<unsigned>(m, "pair_mask1", &npm), *pm2 = field<unsigned>(m, "pair_mask2");
  bool ok = bm && pm1 && pm2;
  for (int b = 0; ok && b < nbm; ++b) ok = legs_of(bm[b]) <= 1;
  for (int q = 0; ok && q < npm; ++q) ok = legs_of(pm1[q] | pm2[q]) <= 1;
  return ok ? nullptr : "the Go2 kernels need a trunk of 6 dofs carrying legs of 3 dofs that only couple through the trunk";
}

const char* check_condim(rsr_model& m, const rsr::KernelSpec& k) {
  int npc = 0; const int* pc = field<int>(m, "pair_condim", &npc);
  for (int i = 0; i < npc; ++i) if (pc[i] != k.condim) return "contact pairs must all have the condim the kernel is built for (Airbot 4, Go2 3)";
  return nullptr;
}
const char* check_equality(rsr_model& m, const rsr::KernelSpec&) {
  int nea = 0; const int* ea = field<int>(m, "eq_active0", &nea);
  for (int i = 0; i < nea; ++i) if (!ea[i]) return "inactive equality constraints are not built";
  return nullptr;
}
const char* check_integrator(rsr_model& m, const rsr::KernelSpec&) {
  const int integrator = field<int>(m, "opt_integrator")[0];
  return integrator != rsr::INT_IMPLICITFAST && integrator != rsr::INT_EULER ? "integrator" : nullptr;
}

// the kernels treat dofs [ISO0, ISO1) as decoupled from the rest: no chain, pair or equality may straddle the range
const char* check_iso(rsr_model& m, const rsr::KernelSpec& k) {
  if (k.iso1 <= k.iso0) return nullptr;
  const unsigned iso = ((1u << k.iso1) - 1u) & ~((1u << k.iso0) - 1u);
  auto straddles = [&](unsigned mask) { return (mask & iso) && (mask & ~iso); };
  int nb = 0, np1 = 0, np2 = 0, ne1 = 0, ne2 = 0, nj = 0;
  const unsigned* bm = field<unsigned>(m, "body_dofmask", &nb);
  const unsigned *m1 = field<unsigned>(m, "pair_mask1", &np1), *m2 = field<unsigned>(m, "pair_mask2", &np2);
  const int *e1 = field<int>(m, "eq_obj1id", &ne1), *e2 = field<int>(m, "eq_obj2id", &ne2), *jd = field<int>(m, "jnt_dofadr", &nj);
  bool bad = !bm || !m1 || !m2 || np1 != np2 || !jd;
  const unsigned low = (1u << k.iso0) - 1u;      // the trees before / after the range must be separate too (mass matrix blocks)
  for (int i = 0; !bad && i < nb; ++i) bad = straddles(bm[i]) || ((bm[i] & low) && (bm[i] & ~low));
  for (int i = 0; !bad && i < np1; ++i) bad = straddles(m1[i] | m2[i]);
  for (int i = 0; !bad && e1 && e2 && i < ne1 && i < ne2; ++i) {
    unsigned mk = (e1[i] >= 0 && e1[i] < nj ? 1u << jd[e1[i]] : 0u) | (e2[i] >= 0 && e2[i] < nj ? 1u << jd[e2[i]] : 0u);
    bad = straddles(mk);
  }
  return bad ? "the kernel assumes the target body's dofs share no chain, contact pair or equality with other dofs" : nullptr;
}

// height-field pairs: kernels with Dims::HFIELD only, one field, spheres no wider than a grid cell; notes whether the model has any
const char* check_hfield(rsr_model& m, const rsr::KernelSpec& k) {
  int npk = 0, nh = 0, nsz = 0, nd = 0, ng2 = 0, ngs = 0;
  const int* pk = field<int>(m, "pair_kind", &npk);
  bool any_hf = false;
  for (int i = 0; pk && i < npk; ++i) any_hf |= (pk[i] == rsr::PAIR_HFIELD_SPHERE);
  m.has_hfield = any_hf;
  if (!any_hf) return nullptr;
  const int *hr = field<int>(m, "hfield_nrow", &nh), *hc = field<int>(m, "hfield_ncol");
  const float* hs = field<float>(m, "hfield_size", &nsz);
  m.find("hfield_data", &nd);
  bool ok = k.hfield && hr && hc && hs && nh == 1 && nsz == 4 && hr[0] >= 3 && hc[0] >= 3 && nd == hr[0] * hc[0];
  if (ok) {
    const float cell = std::fmin(2.0f * hs[0] / (float)(hc[0] - 1), 2.0f * hs[1] / (float)(hr[0] - 1));
    const int* g2 = field<int>(m, "pair_geom2", &ng2);
    const float* gs = field<float>(m, "geom_size", &ngs);
    for (int i = 0; i < npk; ++i)
      if (pk[i] == rsr::PAIR_HFIELD_SPHERE && (i >= ng2 || g2[i] < 0 || 3 * g2[i] + 2 >= ngs || 2.0f * gs[3 * g2[i]] > cell)) ok = false;
  }
  return ok ? nullptr : "height-field pairs need the Go2 kernels, exactly one height field of at least 3x3 samples, and spheres no wider than a grid cell";
}

using Check = const char* (*)(rsr_model&, const rsr::KernelSpec&);
constexpr Check checks[] = {check_joints, check_geom_slots, check_trees, check_arrow, check_condim,
                            check_equality, check_integrator, check_iso, check_hfield};
}  // namespace

extern "C" int rsr_model_create(const void* blob, size_t nbytes, rsr_model** out) {
  if (!blob || !out || nbytes < 32) return fail(RSR_ERR_ARG, "rsr_model_create: null or short blob");
  const int32_t* h = static_cast<const int32_t*>(blob);
  if (std::memcmp(blob, "RSRM", 4) != 0 || h[1] != 2 || (size_t)h[3] > nbytes)
    return fail(RSR_ERR_ARG, "rsr_model_create: not an RSRM v2 blob (v2: the lane records carry solimp clamped and with 1 / width: rsr_mjx_amd/model.py impedance_consts)");
  {  // every directory entry must lie inside the blob before anything is read through it (header: magic, version, entry count, bytes)
    const long long nent = h[2];
    if (nent < 0 || 16 + (unsigned long long)nent * sizeof(blob_entry) > nbytes) return fail(RSR_ERR_ARG, "rsr_model_create: entry table exceeds the blob");
    const blob_entry* e = reinterpret_cast<const blob_entry*>(static_cast<const char*>(blob) + 16);
    for (long long i = 0; i < nent; ++i) {
      const bool named = std::memchr(e[i].name, 0, sizeof(e[i].name)) != nullptr;
      if (!named || e[i].count < 0 || e[i].offset < 0 || (e[i].offset & 3) || (unsigned long long)e[i].offset + 4ull * (unsigned long long)e[i].count > nbytes)
        return fail(RSR_ERR_ARG, "rsr_model_create: blob entry " + std::to_string(i) + " has no name terminator or points outside the blob");
    }
  }
  auto m = std::make_unique<rsr_model>();
  m->blob.assign(static_cast<const char*>(blob), static_cast<const char*>(blob) + nbytes);
  int ndims = 0, nei = 0;
  const int* dims = field<int>(*m, "dims", &ndims);
  const int* ei = field<int>(*m, "env_int", &nei);
  if (!dims || !ei || ndims < 9 || nei < 6) return fail(RSR_ERR_ARG, "rsr_model_create: blob lacks dims/env_int");
  {  // fields read below or by fill_dmodel without a further check
    static const char* const need[] = {"counts2", "opt_integrator", "opt_timestep", "opt_gravity", "opt_tolerance", "opt_ls_tolerance", "opt_impratio",
                                       "stat_meaninertia", "opt_iterations", "opt_ls_iterations", "opt_disable_eulerdamp", "opt_disable_refsafe",
                                       "pair_condim", "pair_kind", "pair_geom1", "pair_geom2", "geom_size", "eq_active0", "lane_rec", "geom_slot_ids"};
    for (const char* f : need) {
      int cnt = 0;
      if (!m->find(f, &cnt) || (cnt < 1 && std::strcmp(f, "pair_condim") && std::strcmp(f, "pair_kind") && std::strcmp(f, "pair_geom1") && std::strcmp(f, "pair_geom2") && std::strcmp(f, "eq_active0")))
        return fail(RSR_ERR_ARG, std::string("rsr_model_create: blob lacks field ") + f);
    }
    int nc2 = 0, ng = 0; m->find("counts2", &nc2); m->find("opt_gravity", &ng);
    if (nc2 < 4 || ng < 3) return fail(RSR_ERR_ARG, "rsr_model_create: counts2 / opt_gravity too short");
  }
  rsr_dims& d = m->dims;
  d.nq = dims[0]; d.nv = dims[1]; d.nu = dims[2]; d.nbody = dims[3]; d.njnt = dims[4]; d.ngeom = dims[5];
  d.nsite = dims[6]; d.neq = dims[7]; d.npair = dims[8];
  d.env_kind = ei[0]; d.n_frames = ei[1]; d.episode_length = ei[2]; d.obs_dim = ei[4]; d.nmetrics = ei[5];
  const rsr::KernelSpec* k = rsr::kernel_spec(d.env_kind);
  if (!k || !fits(d, field<int>(*m, "counts2"), *k))
    return fail(RSR_ERR_UNSUPPORTED, "rsr_model_create: model dims / env kind have no compiled kernel (built: Airbot cube, Airbot sf, Airbot T-shape, Go2 joystick, Go2 handstand / footstand)");
  for (Check check : checks)
    if (const char* why = check(*m, *k)) return fail(RSR_ERR_UNSUPPORTED, std::string("rsr_model_create: ") + why);
  m->spec = k;
  d.ncon_max = k->ncon; d.nefc_max = k->nefc; d.lds_bytes = k->lds_bytes;
  m->layout = make_layout(d, *k);
  d.rec_floats = m->layout.rec;
  *out = m.release();
  return RSR_OK;
}

extern "C" int rsr_model_dims(const rsr_model* m, rsr_dims* out) {
  if (!m || !out) return fail(RSR_ERR_ARG, "rsr_model_dims: null");
  *out = m->dims;
  return RSR_OK;
}
extern "C" void rsr_model_destroy(rsr_model* model) { delete model; }

static int fill_dmodel(const rsr_model* m, const char* dbase, DModel& dm) {
#define P(T, name) { ptrdiff_t o = m->offset_of(#name); if (o < 0) return fail(RSR_ERR_ARG, "blob lacks field " #name); dm.name = (decltype(dm.name))(dbase + o); }
  P(int, body_parentid) P(int, body_rootid) P(int, body_jntnum) P(int, body_jntadr) P(int, body_dofnum) P(int, body_dofadr) P(int, body_depth)
  P(float, body_pos) P(float, body_quat) P(float, body_ipos) P(float, body_iquat) P(float, body_mass) P(float, body_inertia) P(float, body_invweight0)
  P(int, jnt_type) P(int, jnt_qposadr) P(int, jnt_dofadr) P(int, jnt_bodyid) P(int, jnt_limited) P(int, jnt_actfrclimited)
  P(float, jnt_pos) P(float, jnt_axis) P(float, jnt_range) P(float, jnt_actfrcrange) P(float, jnt_solref) P(float, jnt_solimp) P(float, jnt_margin)
  P(int, dof_bodyid) P(int, dof_jntid)
  P(unsigned, dof_ancmask) P(unsigned, dof_velmask) P(unsigned, body_dofmask) P(unsigned, body_submask)
  P(float, dof_armature) P(float, dof_damping) P(float, dof_frictionloss) P(float, dof_invweight0) P(float, dof_solref) P(float, dof_solimp)
  P(int, geom_bodyid) P(int, geom_priority) P(float, geom_size) P(float, geom_pos) P(float, geom_quat) P(float, geom_friction) P(int, geom_slot_ids)
  P(int, site_bodyid) P(float, site_pos) P(float, site_quat)
  P(int, eq_obj1id) P(int, eq_obj2id) P(int, eq_active0) P(float, eq_data) P(float, eq_solref) P(float, eq_solimp)
  P(int, actuator_trnid) P(int, actuator_ctrllimited) P(int, actuator_forcelimited)
  P(float, actuator_gear) P(float, actuator_gainprm) P(float, actuator_biasprm) P(float, actuator_ctrlrange) P(float, actuator_forcerange)
  P(int, pair_geom1) P(int, pair_geom2) P(int, pair_kind) P(int, pair_condim)
  P(float, pair_solref) P(float, pair_solimp) P(float, pair_margin) P(float, pair_gap)
  P(int, fric_dofs) P(int, limit_jnts) P(float, qpos0)
  P(int, pair_b1) P(int, pair_b2) P(int, pair_root1) P(int, pair_root2) P(unsigned, pair_mask1) P(unsigned, pair_mask2)
  P(float, pair_tw) P(float, pair_incl) P(int, dof_rootid) P(int, dof_jtype) P(int, dof_k) P(int, dof_act) P(int, dof_afl)
  P(float, dof_afrange) P(int, body_jtype) P(int, body_qposadr) P(float, body_jpos) P(float, body_jaxis)
  P(int4, lane_rec)
  { int nrec = 0; m->find("lane_rec", &nrec); if (nrec != rsr::LQ_COUNT * 64 * 4) return fail(RSR_ERR_ARG, "blob field lane_rec has the wrong size (model.py lane_records vs enum LaneQuad)"); }
  P(float, hfield_size) P(float, hfield_data) P(int, hfield_nrow) P(int, hfield_ncol)
  P(int, env_ids) P(float, env_action_scale) P(float, env_ctrl_lo) P(float, env_ctrl_hi) P(float, env_reset) P(float, env_reward)
  if (go2_family(m)) {
    P(float, env_go2f) P(float, env_go2_scales) P(float, env_go2_home) P(float, env_go2_soft) P(int, env_go2i)
  } else { dm.env_go2f = dm.env_go2_scales = dm.env_go2_home = dm.env_go2_soft = nullptr; dm.env_go2i = nullptr; }
#undef P
  auto F = [&](const char* n) { return static_cast<const float*>(m->find(n)); };
  auto I = [&](const char* n) { return static_cast<const int*>(m->find(n)); };
  dm.timestep = F("opt_timestep")[0];
  for (int i = 0; i < 3; ++i) dm.gravity[i] = F("opt_gravity")[i];
  dm.tolerance = F("opt_tolerance")[0]; dm.ls_tolerance = F("opt_ls_tolerance")[0]; dm.impratio = F("opt_impratio")[0];
  dm.meaninertia = F("stat_meaninertia")[0];
  dm.iterations = I("opt_iterations")[0]; dm.ls_iterations = I("opt_ls_iterations")[0]; dm.integrator = I("opt_integrator")[0];
  dm.disable_eulerdamp = I("opt_disable_eulerdamp")[0]; dm.disable_refsafe = I("opt_disable_refsafe")[0];
  dm.nfric = I("counts2")[0]; dm.nlimit = I("counts2")[1]; dm.maxdepth = I("counts2")[2];
  { int nc2 = 0; const int* c2 = static_cast<const int*>(m->find("counts2", &nc2)); dm.max_sub = nc2 > 5 ? c2[4] : 32; dm.max_chain = nc2 > 5 ? c2[5] : 32; }
  const int* ei = I("env_int");
  dm.env_kind = ei[0]; dm.n_frames = ei[1]; dm.episode_length = ei[2]; dm.wrap_flags = ei[3];
  return RSR_OK;
}

extern "C" int rsr_batch_create(const rsr_model* m, int num_envs, int hip_device, float* state, rsr_batch** out) {
  if (!m || !out || num_envs <= 0) return fail(RSR_ERR_ARG, "rsr_batch_create: bad argument");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(RSR_ERR_HIP, std::string("rsr_batch_create: no HIP device (this library has no CPU path): hipGetDeviceCount -> ") +
                                 hipGetErrorString(e) + ", count " + std::to_string(ndev));
  if (hip_device < 0 || hip_device >= ndev) return fail(RSR_ERR_ARG, "rsr_batch_create: hip_device out of range");
  HIPCHK(hipSetDevice(hip_device));
  rsr_batch* b = new rsr_batch();
  b->model = m; b->n = num_envs; b->device = hip_device;
  b->dr_fric = b->dr_mass = b->dr_damp = b->dr_floss = nullptr; b->debug = nullptr;
  for (auto& p : b->dr_ex) p = nullptr;
  b->timing = false; b->launches = 0; b->ev0 = b->ev1 = nullptr;
  b->state = state; b->owns_state = false; b->dblob = nullptr;
  if (!state) {
    size_t bytes = (size_t)num_envs * m->layout.rec * sizeof(float);
    if (hipMalloc(&b->state, bytes) != hipSuccess) { delete b; return fail(RSR_ERR_NOMEM, "rsr_batch_create: hipMalloc(state)"); }
    b->owns_state = true;
    (void)hipMemset(b->state, 0, bytes);
  }
  if (hipMalloc(&b->dblob, m->blob.size()) != hipSuccess) { if (b->owns_state) (void)hipFree(b->state); delete b; return fail(RSR_ERR_NOMEM, "rsr_batch_create: hipMalloc(model)"); }
  auto release = [&]() {            // every failure path below frees what has been allocated so far
    if (b->dmodel) (void)hipFree(b->dmodel);
    if (b->sched) (void)hipFree(b->sched);
    if (b->dblob) (void)hipFree(b->dblob);
    if (b->owns_state && b->state) (void)hipFree(b->state);
    delete b;
  };
  b->dmodel = nullptr; b->sched = nullptr;
  { hipError_t ce = hipMemcpy(b->dblob, m->blob.data(), m->blob.size(), hipMemcpyHostToDevice);
    if (ce != hipSuccess) { release(); return fail(RSR_ERR_HIP, std::string("rsr_batch_create: hipMemcpy(model): ") + hipGetErrorString(ce)); } }
  int rc = fill_dmodel(m, b->dblob, b->dm);
  if (rc) { release(); return rc; }
  b->launch_id = 0; b->units = 1; b->step_grid = 0; b->spin_cap = RSR_SPIN_CAP_DEFAULT; b->withhold_env = -1; b->whole_envs = -1;
  b->prio_policy = -1; b->prio_slots = 1;
  b->action_repeat = 1; b->dmodel_plain = nullptr; b->racc = nullptr;
  const int step_per_cu = launch(b, rsr::OP_STEP_OCCUPANCY, launch_args(b, nullptr));    // resident workgroups per CU of the step kernel
  if (go2_family(m)) {
    int per_cu = step_per_cu;
    hipDeviceProp_t prop;
    if (per_cu <= 0 || hipGetDeviceProperties(&prop, hip_device) != hipSuccess) { per_cu = 16; prop.multiProcessorCount = 256; }
    b->prio_slots = per_cu * prop.multiProcessorCount;
    if (const char* pv = std::getenv("RSR_PRIO_MODE")) b->prio_policy = std::atoi(pv);    // diagnostic (tools/ab_bench.py)
  } else {
    const size_t sb = (4 + (size_t)num_envs) * sizeof(int);
    if (hipMalloc(&b->sched, sb) != hipSuccess) { b->sched = nullptr; release(); return fail(RSR_ERR_NOMEM, "rsr_batch_create: hipMalloc(sched)"); }
    (void)hipMemset(b->sched, 0, sb);
    // resident waves of the step kernel on this device: the grid of the persistent launch
    int per_cu = step_per_cu; hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) != hipSuccess || per_cu <= 0) { per_cu = 8; prop.multiProcessorCount = 256; }
    if (const char* gv = std::getenv("RSR_GRID_PER_CU")) { const int g = std::atoi(gv); if (g > 0 && g < per_cu) per_cu = g; }   // diagnostic: fewer resident waves
    b->step_grid = per_cu * prop.multiProcessorCount;
    const char* ev = std::getenv("RSR_UNITS");
    b->units = ev ? std::atoi(ev) : RSR_DEFAULT_UNITS;
    if (b->units < 1) b->units = 1;
    if (b->units > m->dims.n_frames) b->units = m->dims.n_frames;
    if (b->units > RSR_MAX_UNITS) b->units = RSR_MAX_UNITS;
    if (const char* wv = std::getenv("RSR_WHOLE_ENVS")) b->whole_envs = std::atoi(wv);      // diagnostic (tools/ab_bench.py)
    b->prio_policy = 0;      // the work queue balances itself: rotate / final-set priorities measured at +-0.2 % on the cube and the T-shape
  }
  if (hipMalloc(&b->dmodel, sizeof(DModel)) != hipSuccess) { b->dmodel = nullptr; release(); return fail(RSR_ERR_NOMEM, "rsr_batch_create: hipMalloc(dmodel)"); }
  { hipError_t ce = hipMemcpy(b->dmodel, &b->dm, sizeof(DModel), hipMemcpyHostToDevice);
    if (ce != hipSuccess) { release(); return fail(RSR_ERR_HIP, std::string("rsr_batch_create: hipMemcpy(dmodel): ") + hipGetErrorString(ce)); } }
  *out = b;
  return RSR_OK;
}

extern "C" void rsr_batch_destroy(rsr_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->dblob) (void)hipFree(b->dblob);
  if (b->dmodel) (void)hipFree(b->dmodel);
  if (b->dmodel_plain) (void)hipFree(b->dmodel_plain);
  if (b->racc) (void)hipFree(b->racc);
  if (b->sched) (void)hipFree(b->sched);
  if (b->owns_state && b->state) (void)hipFree(b->state);
  delete b;
}

extern "C" int rsr_batch_set_dr(rsr_batch* b, const float* geom_friction, const float* body_mass, const float* dof_damping,
                                const float* dof_frictionloss) {
  if (!b) return fail(RSR_ERR_ARG, "rsr_batch_set_dr: null batch");
  b->dr_fric = geom_friction; b->dr_mass = body_mass; b->dr_damp = dof_damping; b->dr_floss = dof_frictionloss;
  return RSR_OK;
}

extern "C" int rsr_batch_set_dr_field(rsr_batch* b, int dr_field, const float* dev_values) {
  if (!b) return fail(RSR_ERR_ARG, "rsr_batch_set_dr_field: null batch");
  switch (dr_field) {
    case RSR_DR_GEOM_FRICTION: b->dr_fric = dev_values; return RSR_OK;
    case RSR_DR_BODY_MASS: b->dr_mass = dev_values; return RSR_OK;
    case RSR_DR_DOF_DAMPING: b->dr_damp = dev_values; return RSR_OK;
    case RSR_DR_DOF_FRICTIONLOSS: b->dr_floss = dev_values; return RSR_OK;
    case RSR_DR_BODY_IPOS: case RSR_DR_QPOS0: case RSR_DR_DOF_ARMATURE: case RSR_DR_ACTUATOR_GAINPRM: case RSR_DR_ACTUATOR_BIASPRM:
      if (!go2_family(b->model))
        return fail(RSR_ERR_UNSUPPORTED, "rsr_batch_set_dr_field: this field is per-env only in the Go2 kernels (randomize.py); the Airbot kernels take the four fields of rsr_batch_set_dr");
      b->dr_ex[dr_field - RSR_DR_BODY_IPOS] = dev_values;
      return RSR_OK;
    default: return fail(RSR_ERR_ARG, "rsr_batch_set_dr_field: unknown field");
  }
}

extern "C" int rsr_batch_set_schedule(rsr_batch* b, int units) {
  if (!b || units < 1) return fail(RSR_ERR_ARG, "rsr_batch_set_schedule: bad argument");
  b->units = units > b->model->dims.n_frames ? b->model->dims.n_frames : units;
  if (b->units > RSR_MAX_UNITS) b->units = RSR_MAX_UNITS;
  return RSR_OK;
}

extern "C" int rsr_batch_set_whole_envs(rsr_batch* b, int whole_envs) {
  if (!b || whole_envs > b->n) return fail(RSR_ERR_ARG, "rsr_batch_set_whole_envs: bad argument");
  b->whole_envs = whole_envs < 0 ? -1 : whole_envs;
  return RSR_OK;
}

extern "C" int rsr_batch_set_action_repeat(rsr_batch* b, int repeat) {
  if (!b || repeat < 1 || repeat > 64) return fail(RSR_ERR_ARG, "rsr_batch_set_action_repeat: repeat must be 1 ... 64");
  HIPCHK(hipSetDevice(b->device));
  if (repeat > 1 && !b->dmodel_plain) {
    DModel plain = b->dm;
    plain.wrap_flags = 0;
    if (hipMalloc(&b->dmodel_plain, sizeof(DModel)) != hipSuccess) { b->dmodel_plain = nullptr; return fail(RSR_ERR_NOMEM, "rsr_batch_set_action_repeat: hipMalloc(dmodel)"); }
    if (hipMalloc(&b->racc, (size_t)b->n * sizeof(float)) != hipSuccess) {
      (void)hipFree(b->dmodel_plain); b->dmodel_plain = nullptr; b->racc = nullptr;
      return fail(RSR_ERR_NOMEM, "rsr_batch_set_action_repeat: hipMalloc(reward sums)");
    }
    HIPCHK(hipMemcpy(b->dmodel_plain, &plain, sizeof(DModel), hipMemcpyHostToDevice));
  }
  b->action_repeat = repeat;
  return RSR_OK;
}

extern "C" int rsr_batch_set_priority(rsr_batch* b, int policy) {
  if (!b || policy > rsr::RSR_PRIO_CATCH_UP) return fail(RSR_ERR_ARG, "rsr_batch_set_priority: bad argument");
  b->prio_policy = policy < 0 ? -1 : policy;
  return RSR_OK;
}

extern "C" int rsr_batch_set_fault_injection(rsr_batch* b, int spin_cap, int withhold_env) {
  if (!b) return fail(RSR_ERR_ARG, "rsr_batch_set_fault_injection: null batch");
  b->spin_cap = spin_cap > 0 ? spin_cap : RSR_SPIN_CAP_DEFAULT;
  b->withhold_env = (withhold_env >= 0 && withhold_env < b->n) ? withhold_env : -1;
  return RSR_OK;
}

extern "C" int rsr_batch_check(rsr_batch* b, void* hip_stream, int* handoff_timeouts) {
  if (!b) return fail(RSR_ERR_ARG, "rsr_batch_check: null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));
  int err[2] = {0, 0};
  if (b->sched) HIPCHK(hipMemcpy(err, b->sched + 2, sizeof(err), hipMemcpyDeviceToHost));
  if (handoff_timeouts) *handoff_timeouts = err[0];
  if (err[0] > 0)
    return fail(RSR_ERR_HANDOFF, "rsr_batch_check: " + std::to_string(err[0]) + " work-unit hand-off wait(s) timed out since the batch was created (last: env " +
                                     std::to_string(err[1]) + "); those envs' stats[3] read -1 for the step concerned and their state is not to be trusted");
  return RSR_OK;
}

extern "C" int rsr_batch_set_debug(rsr_batch* b, float* dev_buffer) {
  if (!b) return fail(RSR_ERR_ARG, "rsr_batch_set_debug: null batch");
  b->debug = dev_buffer;
  return RSR_OK;
}

rsr::StepArgs make_args(rsr_batch* b) {
  rsr::StepArgs a{};
  a.state = b->state; a.n = b->n;
  a.dr_geom_friction = b->dr_fric; a.dr_body_mass = b->dr_mass; a.dr_dof_damping = b->dr_damp; a.dr_dof_frictionloss = b->dr_floss;
  a.dr_body_ipos = b->dr_ex[0]; a.dr_qpos0 = b->dr_ex[1]; a.dr_dof_armature = b->dr_ex[2]; a.dr_gainprm = b->dr_ex[3]; a.dr_biasprm = b->dr_ex[4];
  a.debug = b->debug;
  // default: waves that start together take turns; a joystick batch of more than one resident round lets its late starters catch up,
  // except when they are few (up to 5/8 of a round beyond the first: the slots the oldest-first arbitration frees early are worth more
  // than an even finish there -- 5120 / 6144 envs on 4096 slots lose 3.5 / 2 % under either policy, 7168 gain 9 %: DESIGN.md 4)
  const bool rotate = b->model->dims.env_kind == rsr::ENV_GO2_HANDSTAND || b->n <= b->prio_slots;
  const bool few_late = !rotate && (long long)b->n * 8 < (long long)b->prio_slots * 13;
  a.prio_mode = b->prio_policy >= 0 ? b->prio_policy : (rotate ? rsr::RSR_PRIO_ROTATE : (few_late ? rsr::RSR_PRIO_OFF : rsr::RSR_PRIO_CATCH_UP));
  a.prio_slots = b->prio_slots;
  return a;
}

rsr::Launch launch_args(rsr_batch* b, void* hip_stream) {
  rsr::Launch x{};
  x.grid = b->n; x.stream = static_cast<hipStream_t>(hip_stream);
  x.dm = b->dmodel; x.L = b->model->layout; x.a = make_args(b);
  x.env_kind = b->model->dims.env_kind; x.hfield = b->model->has_hfield;
  return x;
}

int launch(const rsr_batch* b, int op, const rsr::Launch& x) {
  switch (b->model->spec->family) {
    case rsr::FAMILY_CUBE: return rsr::launch_cube(op, x);
    case rsr::FAMILY_TSHAPE: return rsr::launch_tshape(op, x);
    case rsr::FAMILY_GO2: return rsr::launch_go2(op, x);
  }
  return 0;
}

extern "C" int rsr_reset(rsr_batch* b, const uint32_t* keys, void* hip_stream) {
  if (!b || !keys) return fail(RSR_ERR_ARG, "rsr_reset: null argument");
  HIPCHK(hipSetDevice(b->device));
  rsr::Launch x = launch_args(b, hip_stream);
  x.a.keys = keys;
  launch(b, rsr::OP_RESET, x);
  HIPCHK(hipGetLastError());
  return RSR_OK;
}

extern "C" int rsr_step(rsr_batch* b, const float* action, void* hip_stream) {
  if (!b || !action) return fail(RSR_ERR_ARG, "rsr_step: null argument");
  HIPCHK(hipSetDevice(b->device));
  rsr::Launch x = launch_args(b, hip_stream);
  x.a.action = action;
  hipStream_t st = x.stream;
  const int repeat = b->action_repeat;
  const Layout& LY = b->model->layout;
  const rsr_dims& dd = b->model->dims;
  const bool go2 = go2_family(b->model);
  if (repeat > 1) x.dm = b->dmodel_plain;         // plain env.step, the wrappers around the repeats
  if (repeat > 1)
    hipLaunchKernelGGL(rsr::repeat_pre_kernel, dim3(b->n), dim3(64), 0, st, b->state, LY, b->n, b->dm.wrap_flags, b->racc);
  for (int rep = 0; rep < repeat; ++rep) {
  if (!go2) {                                     // the Airbot step kernels: persistent work-queue launch
    ++b->launch_id;
    if ((b->launch_id & 0xFFFFFFu) == 0u) {        // the flags carry 24 bits of the launch number: clear them before the number repeats
      ++b->launch_id;
      HIPCHK(hipMemsetAsync(b->sched + 4, 0, (size_t)b->n * sizeof(int), st));
    }
    // envs stepped as one unit: by default all but two resident rounds' worth (the launch then still drains in short units, with
    // a slack of two resident rounds between the phases of a split env); a batch that fits the resident waves is not split at all
    // (every env has a wave to itself from the start: phases would only add hand-offs; 1024 envs 3.64 -> 4.48 M env-steps/s)
    int n_whole = b->units <= 1 ? b->n : (b->whole_envs >= 0 ? b->whole_envs : (b->n <= b->step_grid ? b->n : (b->n > 2 * b->step_grid ? b->n - 2 * b->step_grid : 0)));
    if (n_whole > b->n) n_whole = b->n;
    x.sc = rsr::Sched{b->sched, b->sched + 2, reinterpret_cast<unsigned*>(b->sched + 4), b->launch_id, b->units, n_whole, b->spin_cap, b->withhold_env};
    const long long work = (long long)n_whole + (long long)b->units * (b->n - n_whole);
    x.grid = (int)(work > b->step_grid ? b->step_grid : work);
  }
  launch(b, rsr::OP_STEP, x);
  if (repeat > 1)
    hipLaunchKernelGGL(rsr::repeat_acc_kernel, dim3((b->n + 255) / 256), dim3(256), 0, st, b->state, LY, b->n, b->racc);
  }
  if (repeat > 1)
    hipLaunchKernelGGL(rsr::repeat_post_kernel, dim3(b->n), dim3(64), 0, st, b->state, LY, b->n, b->dm.wrap_flags, repeat, b->dm.episode_length,
                       dd.nmetrics, dd.obs_dim, b->model->spec->priv, dd.env_kind == rsr::ENV_GO2 ? (int)rsr::G2_XFRC : -1, b->racc);
  HIPCHK(hipGetLastError());
  if (b->timing) b->launches++;
  return RSR_OK;
}

extern "C" int rsr_view(rsr_batch* b, int field_id, void** dev_ptr, int64_t shape[2], int64_t stride[2]) {
  if (!b || !dev_ptr || !shape || !stride) return fail(RSR_ERR_ARG, "rsr_view: null argument");
  const Layout& L = b->model->layout;
  const rsr_dims& d = b->model->dims;
  const rsr::KernelSpec& k = *b->model->spec;
  const int view[][2] = {      // {offset, width} of every rsr_field, in the enum's order
      {L.qpos, d.nq}, {L.qvel, d.nv}, {L.ctrl, d.nu}, {L.warm, d.nv}, {L.time, 1}, {L.xpos, d.nbody * 3}, {L.site_xpos, d.nsite * 3},
      {L.obs, d.obs_dim}, {L.reward, 1}, {L.done, 1}, {L.metrics, d.nmetrics},
      {L.target_pos, 3}, {L.new_cube_pos, 2}, {L.site_pos, 3}, {L.cube_pos, 3}, {L.last_action, 1},
      {L.target_base_pos, 3}, {L.target_vertical_pos, 3}, {L.target_w, 1}, {L.new_T_pos, 2}, {L.T_pos, 3}, {L.xita, 1},
      {L.go2_info, k.ninfo},
      {L.steps, 1}, {L.truncation, 1}, {L.episode_done, 1}, {L.episode_metrics, 2 + d.nmetrics},
      {L.f_qpos, d.nq}, {L.f_qvel, d.nv}, {L.f_ctrl, d.nu}, {L.f_warm, d.nv}, {L.f_time, 1},
      {L.f_xpos, d.nbody * 3}, {L.f_site_xpos, d.nsite * 3}, {L.f_obs, d.obs_dim},
      {L.priv_obs, k.priv}, {L.f_priv_obs, k.priv}, {L.stats, 4}};
  static_assert(sizeof(view) / sizeof(view[0]) == RSR_F_COUNT, "one entry per rsr_field");
  if (field_id < 0 || field_id >= RSR_F_COUNT) return fail(RSR_ERR_ARG, "rsr_view: unknown field id");
  const int off = view[field_id][0], w = view[field_id][1];
  *dev_ptr = b->state + off;
  shape[0] = b->n; shape[1] = w;
  stride[0] = L.rec; stride[1] = 1;
  return RSR_OK;
}

extern "C" int rsr_rollout_metrics(rsr_batch* b, float* dev_out, void* hip_stream) {
  if (!b || !dev_out) return fail(RSR_ERR_ARG, "rsr_rollout_metrics: null argument");
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(rsr::rollout_metrics_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(hip_stream), b->state, b->model->layout, b->n, dev_out);
  HIPCHK(hipGetLastError());
  return RSR_OK;
}

extern "C" int rsr_timing_begin(rsr_batch* b, void* hip_stream) {
  if (!b) return fail(RSR_ERR_ARG, "rsr_timing_begin: null batch");
  HIPCHK(hipSetDevice(b->device));
  if (!b->ev0) { HIPCHK(hipEventCreate(&b->ev0)); HIPCHK(hipEventCreate(&b->ev1)); }
  b->launches = 0; b->timing = true;
  HIPCHK(hipEventRecord(b->ev0, static_cast<hipStream_t>(hip_stream)));
  return RSR_OK;
}

extern "C" int rsr_timing_end(rsr_batch* b, void* hip_stream, float* total_ms, int* launches) {
  if (!b || !b->timing || !total_ms || !launches) return fail(RSR_ERR_ARG, "rsr_timing_end: bad argument / timing not begun");
  HIPCHK(hipEventRecord(b->ev1, static_cast<hipStream_t>(hip_stream)));
  HIPCHK(hipEventSynchronize(b->ev1));
  HIPCHK(hipEventElapsedTime(total_ms, b->ev0, b->ev1));
  *launches = b->launches;
  b->timing = false;
  return RSR_OK;
}