/*
 * rsr_physics.h -- physics-level C ABI of librsrmjx.so, on top of the env batch of rsr_mjx.h: the two calls every reference env
 * is written against (_src/mjx_env.py:30-73).
 *
 *   rsr_physics_forward <- mjx_env.init(model, qpos, qvel, ctrl): one mjx.forward on the record's qpos / qvel / ctrl
 *                          (qacc_warmstart as the record holds it; the caller zeroes it first to match init).
 *   rsr_physics_step    <- mjx_env.step(model, data, ctrl, n_substeps): writes ctrl into the record, then nsteps x mjx.step.
 *
 * A physics handle shares its batch with rsr_step: same model, same per-env leaves of rsr_batch_set_dr / rsr_batch_set_dr_field,
 * same record.  The calls read and write only the pipeline fields qpos, qvel, ctrl, qacc_warmstart, time, xpos, site_xpos (a
 * forward leaves qpos, qvel, ctrl and time as they are); obs, reward, done, metrics, info_*, first_* and stats are left alone, and
 * no PRNG key advances.  data.xfrc_applied is zero.  As in MJX's Data (and in the record after rsr_step), xpos / site_xpos and the
 * xquat / contacts of rsr_physics_view are those of the last forward pass, taken before the final integration.  One wavefront per
 * env, a plain launch: the scheduling knobs of rsr_step do not apply.  A following rsr_step continues from the state these leave.
 * Conventions as in rsr_mjx.h (0 on success, rsr_last_error; asynchronous on hip_stream, NULL = default stream).
 */
#ifndef RSR_PHYSICS_H_
#define RSR_PHYSICS_H_

#include "rsr_mjx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsr_physics rsr_physics;

/* A physics handle on batch b, which must outlive it.  Allocates the side buffer of rsr_physics_view (zeroed).  Every model the
 * env kernels are built for has physics kernels; anything else is RSR_ERR_UNSUPPORTED. */
int rsr_physics_create(rsr_batch* b, rsr_physics** out);
void rsr_physics_destroy(rsr_physics* p);

/* ctrl: device float32 [num_envs, nu], or NULL to keep the record's ctrl.  nsteps >= 1, otherwise RSR_ERR_ARG. */
int rsr_physics_step(rsr_physics* p, const float* ctrl, int nsteps, void* hip_stream);
int rsr_physics_forward(rsr_physics* p, void* hip_stream);
/* rsr_physics_forward on the envs env_ids[0 .. count) only (device int32; ids outside [0, num_envs) are skipped): the other envs'
 * record and side-buffer rows are not touched.  What set_state(..., env_ids) of rsr_mjx_amd/physics.py runs. */
int rsr_physics_forward_envs(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream);

/* Physics outputs beyond the record: zero-copy strided views (as rsr_view) of the handle's side buffer, which lives outside the
 * persistent record (rec_floats, RSR_F_COUNT and rsr_view are unchanged) and is filled by rsr_physics_step / _forward.  rsr_step
 * never writes it (exporting these from the fused env kernels would change their code), so after an rsr_step the views still show
 * the last physics call's values.
 *   RSR_P_QACC            [nv]              data.qacc of the last forward pass (= the qacc_warmstart the call leaves)
 *   RSR_P_ACTUATOR_FORCE  [nu]              data.actuator_force
 *   RSR_P_XQUAT           [nbody*4]         data.xquat (w, x, y, z)
 *   RSR_P_NCON            [1]               active contacts kept (at most ncon_max), as float
 *   RSR_P_CONTACT         [ncon_max*9]      per contact slot: dist, pos[3], frame normal[3], geom1, geom2 (geoms as float);
 *                                           slots >= ncon hold zeros and geom ids -1
 *   RSR_P_NCON_DROPPED    [1]               active contacts beyond ncon_max that the kernel dropped, as float */
enum rsr_physics_field {
  RSR_P_QACC = 0, RSR_P_ACTUATOR_FORCE, RSR_P_XQUAT, RSR_P_NCON, RSR_P_CONTACT, RSR_P_NCON_DROPPED,
  RSR_P_COUNT
};
int rsr_physics_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);

#ifdef __cplusplus
}
#endif
#endif /* RSR_PHYSICS_H_ */
