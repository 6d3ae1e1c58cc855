/*
 * rsr_physics.h -- physics-level C ABI of librsrmjx.so, on top of the env batch of rsr_mjx.h: the two calls every reference env
 * is written against (_src/mjx_env.py:30-73).
 *
 *   rsr_physics_forward <- mjx_env.init(model, qpos, qvel, ctrl): one mjx.forward on the record's qpos / qvel / ctrl
 *                          (qacc_warmstart as the record holds it; the caller zeroes it first to match init).
 *   rsr_physics_step    <- mjx_env.step(model, data, ctrl, n_substeps): writes ctrl into the record, then nsteps x mjx.step.
 *   rsr_physics_rollout <- mujoco.rollout.rollout / lax.scan(mjx.step): T control steps in one launch, trajectories [N, T, w].
 *   rsr_physics_sample_rollouts <- mujoco.rollout.rollout on K copies of a state / vmap(lax.scan(mjx.step)): K ctrl sequences
 *                          per env from its current state, trajectories [M, K, T, w]; the record is read only.
 *   rsr_physics_param_rollouts <- the same with the model varied: vmap(lambda leaves: lax.scan(mjx.step)) over K sets of model
 *                          leaves per env (friction, mass, damping, gains, ...), with no replica batch; the record is read only.
 *   rsr_physics_feedback_rollouts <- the same in closed loop: lax.scan of u = ctrl + gain (x (-) x_ref) then mjx.step, the control
 *                          of every control step computed on the device from the sample's own state; the record is read only.
 *   rsr_physics_cost_rollouts <- the same reduced on the device: vmap(lambda: sum(lax.scan(cost(mjx.step)))), the running cost
 *                          [M, K] of a weighted least-squares tracking cost per sample, trajectories only on request.
 *   rsr_physics_set_sensors: the site sensors of data.sensordata (RSR_P_SENSORDATA, and a rollout's sensordata rows).
 *   rsr_physics_set_applied / rsr_physics_applied_view: data.xfrc_applied and data.qfrc_applied, per-env inputs of every forward
 *                          pass of these calls (zero until set).
 *   rsr_physics_dynamics <- mj_fullM, data.qfrc_bias / qfrc_passive / qfrc_actuator and mj_jacSite at the record's current state
 *                          (after the last integration, unlike the views of rsr_physics_view), in a buffer of its own.
 *   rsr_physics_constraint <- data.efc_force, data.qfrc_constraint and mj_contactForce of one mjx.forward at the record's current
 *                          state, in a buffer of its own.
 *   rsr_physics_transition_fd <- mjd_transitionFD / jax.jacobian(mjx.step): finite-difference Jacobians A, B, C, D of
 *                          rsr_physics_step about the record's current state, in a buffer of its own.
 *   rsr_physics_trajectory_fd <- mjd_transitionFD at every step of a nominal rollout / vmap(jax.jacobian(mjx.step)) over the
 *                          states of lax.scan(mjx.step): A_t, B_t, C_t, D_t for t < T in two launches; the record is read only.
 *   rsr_physics_lqr_backward <- the backward pass of iLQR / time-varying LQR (the Riccati recursion over lax.scan(reverse=True)):
 *                          A_t, B_t and a quadratic cost model in, the gains K_t, k_t of rsr_physics_feedback_rollouts out, one
 *                          launch; neither the model nor the record is read.
 *   rsr_physics_lqr_box <- the backward pass of control-limited DDP (Tassa, Mansard and Todorov 2014): the same with k_t the
 *                          minimiser of a box-constrained QP and the gain rows of the clamped controls zero, one launch.
 *   rsr_physics_cost_expand <- jax.grad / jax.hessian (Gauss-Newton) of the cost of rsr_physics_cost_rollouts about a nominal run:
 *                          the cost rows and the C_t, D_t of rsr_physics_trajectory_fd in, lx, lu, lxx, luu, lux of
 *                          rsr_physics_lqr_backward out, one launch; neither the model nor the record is read.
 *   rsr_physics_ik      <- an IK library on top of mj_jacSite (damped least squares on site pose targets): M problems, one launch,
 *                          every iteration on the device; the record is read only.
 *   rsr_physics_kalman  <- a Kalman filter and RTS smoother over a log (lax.scan over A_t, C_t forwards, then reverse=True): the
 *                          linearised / error-state EKF about the nominal run of rsr_physics_trajectory_fd, M problems, one launch;
 *                          neither the model nor the record is read.
 *
 * A physics handle shares its batch with rsr_step: same model, same per-env leaves of rsr_batch_set_dr / rsr_batch_set_dr_field,
 * same record.  The calls read and write only the pipeline fields qpos, qvel, ctrl, qacc_warmstart, time, xpos, site_xpos (a
 * forward leaves qpos, qvel, ctrl and time as they are); obs, reward, done, metrics, info_*, first_* and stats are left alone, and
 * no PRNG key advances.  rsr_step ignores the applied forces of a physics handle (the Go2 joystick's kick is env logic with a path
 * of its own).  As in MJX's Data (and in the record after rsr_step), xpos / site_xpos and the
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
 *   RSR_P_NCON_DROPPED    [1]               active contacts beyond ncon_max that the kernel dropped, as float
 *   RSR_P_SENSORDATA      [nsensordata]     data.sensordata of the sensor table (rsr_physics_set_sensors) at the last physics
 *                                           call; width 0 while no table is set.  Row stride RSR_MAX_SENSORDATA, its own
 *                                           buffer: the view's pointer does not move when the table changes */
enum rsr_physics_field {
  RSR_P_QACC = 0, RSR_P_ACTUATOR_FORCE, RSR_P_XQUAT, RSR_P_NCON, RSR_P_CONTACT, RSR_P_NCON_DROPPED, RSR_P_SENSORDATA,
  RSR_P_COUNT
};
int rsr_physics_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);

/* Site sensors (data.sensordata), MuJoCo's definitions for objtype "site".  R, p: the site's frame and position; v, w: its
 * linear and angular velocity in the world frame (object velocity at the site); ref: a second site.
 *   RSR_S_GYRO           [3]   R^T w
 *   RSR_S_VELOCIMETER    [3]   R^T v
 *   RSR_S_ACCELEROMETER  [3]   R^T (linear acceleration at the site, from cacc) + (R^T w) x (R^T v).  Go2 models only, and only on
 *                              a site of the body whose acceleration bias the kernels track (the IMU's); one such site per table
 *   RSR_S_FRAMEPOS       [3]   p, or R_ref^T (p - p_ref) with a ref site
 *   RSR_S_FRAMEXAXIS     [3]   first column of R
 *   RSR_S_FRAMEZAXIS     [3]   third column of R
 *   RSR_S_FRAMEQUAT      [4]   xquat[body] * site_quat (w, x, y, z), not canonicalised
 *   RSR_S_FRAMELINVEL    [3]   v
 *   RSR_S_FRAMEANGVEL    [3]   w
 * Only framepos takes a ref site. */
enum rsr_sensor_type {
  RSR_S_GYRO = 0, RSR_S_VELOCIMETER, RSR_S_ACCELEROMETER, RSR_S_FRAMEPOS, RSR_S_FRAMEXAXIS, RSR_S_FRAMEZAXIS, RSR_S_FRAMEQUAT,
  RSR_S_FRAMELINVEL, RSR_S_FRAMEANGVEL,
  RSR_S_COUNT
};
#define RSR_MAX_SENSORDATA 64

/* The sensor table: nsensor rows of 4 int32 (host memory): type, site id, ref site id or -1, address (first column in sensordata;
 * row i starts where row i-1 ends, row 0 at 0).  At most RSR_MAX_SENSORDATA floats in all.  nsensor = 0 clears the table.
 * Everything is checked before any device work (bad ids, types, addresses, ref sites: RSR_ERR_ARG; an accelerometer the kernels
 * cannot evaluate: RSR_ERR_UNSUPPORTED); on error the previous table stays.  Waits for the device (the table is read by launches
 * in flight).  With a table set, rsr_physics_step / _forward / _forward_envs also fill RSR_P_SENSORDATA after their last forward
 * pass; with none set they run exactly as before. */
int rsr_physics_set_sensors(rsr_physics* p, const int32_t* table, int nsensor);

/* Trajectory buffers of rsr_physics_rollout, device float32, env-major [num_envs, T, width]; a NULL pointer is not recorded.
 *   qpos [nq], qvel [nv], time [1]                   the state after control step t
 *   actuator_force [nu], ncon [1], sensordata [nsensordata]   the last forward pass of control step t, before its final
 *                                                             integration (as the side buffer after rsr_physics_step) */
typedef struct rsr_rollout_out {
  float* qpos;
  float* qvel;
  float* time;
  float* actuator_force;
  float* ncon;
  float* sensordata;
} rsr_rollout_out;

/* T control steps in one launch: for t = 0 .. T-1, ctrl[:, t, :] then nsteps x mjx.step, then the rows t of `out`.  ctrl: device
 * float32 [num_envs, T, nu].  Leaves the record, the side buffer and RSR_P_SENSORDATA exactly as T calls of rsr_physics_step
 * with ctrl[:, t, :] would.  out may be NULL (nothing recorded).  RSR_ERR_ARG: null handle or ctrl, T < 1, nsteps < 1,
 * sensordata requested with no sensor table set. */
int rsr_physics_rollout(rsr_physics* p, const float* ctrl, int T, int nsteps, const rsr_rollout_out* out, void* hip_stream);

/* Sampled rollouts, for sampling planners (predictive sampling, MPPI, CEM): from the state each listed env is in now, K control
 * sequences of T control steps, one launch with one wavefront per (env, sample).  M = count, or num_envs with env_ids NULL.
 * Sample (s, k) starts from the record of env e = env_ids[s] as it stands (qpos, qvel, qacc_warmstart, time), with env e's
 * per-env leaves and, while they are on, its applied forces (held for all T control steps), and runs ctrl[s, k, t] then
 * nsteps x mjx.step for t = 0 .. T-1: bit for bit the trajectory rsr_physics_rollout would record on a batch whose env holds
 * that record row and those leaves.  ctrl: device float32 [M, K, T, nu].  out: the non-NULL members are [M, K, T, width], the
 * fields and their meaning per control step as for rsr_physics_rollout; rows are indexed by slot s, the position in env_ids,
 * not by env id.  Only these buffers are written: the record (the K samples of an env share its row, read only), the side
 * buffer, RSR_P_SENSORDATA and the dynamics, constraint, transition and inverse buffers are untouched, and no PRNG key advances;
 * the handle owns no buffer for this call.  A member of out holds 4 M K T width bytes: record only what the planner's cost reads.
 * env_ids: device int32 [count], or NULL for every env (count is ignored); an id outside [0, num_envs) runs nothing and its
 * slot's rows are left alone.  RSR_ERR_ARG, checked before any device work: null handle, null ctrl, null out or an out with all
 * six members NULL, K < 1, T < 1, nsteps < 1, env_ids with count < 1, sensordata requested with no sensor table set, M K or
 * T nsteps at or above 2^31. */
int rsr_physics_sample_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, int K, int T, int nsteps,
                                const rsr_rollout_out* out, void* hip_stream);

/* Parameter rollouts, for system identification, domain-randomised planning and CEM over model parameters: from the state each
 * listed env is in now, K sets of model leaves, each run for T control steps, one launch with one wavefront per (env, sample)
 * and no replica batch.  M = count, or num_envs with env_ids NULL.  Sample (s, k) starts from the record of env e = env_ids[s]
 * as it stands (qpos, qvel, qacc_warmstart, time), with, while they are on, env e's applied forces (held for all T control
 * steps), and with env e's leaves except those `params` gives: bit for bit the trajectory rsr_physics_rollout would record on a
 * batch whose env holds that record row and, as its per-env leaves, row (s, k) of every given leaf.
 * Per-sample model leaves: device float32 [M, K, width], width as rsr_batch_set_dr_field, indexed by enum rsr_dr_field;
 * a NULL member = the env's own leaf (its per-env value, or the model's).  params may be NULL or all-NULL: every sample then
 * runs the env's own leaves, and with RSR_PR_CTRL_PER_SAMPLE the call is rsr_physics_sample_rollouts.
 * ctrl: device float32 [M, T, nu], one sequence shared by the K samples of a slot (one logged control sequence), or with
 * RSR_PR_CTRL_PER_SAMPLE [M, K, T, nu].  out: the non-NULL members are [M, K, T, width], the fields and their meaning per
 * control step as for rsr_physics_rollout; rows, of ctrl, params and out alike, are indexed by slot s, the position in env_ids,
 * not by env id.  Only the buffers of out are written: the record (the K samples of an env share its row, read only), the side
 * buffer, RSR_P_SENSORDATA, the dynamics, constraint, transition and inverse buffers and the batch's own leaf tensors
 * (rsr_batch_set_dr / rsr_batch_set_dr_field) are untouched, and no PRNG key advances; the handle owns no buffer for this call.
 * A member of out holds 4 M K T width bytes: record only what the loss reads.
 * env_ids: device int32 [count], or NULL for every env (count is ignored); an id outside [0, num_envs) runs nothing and its
 * slot's rows are left alone.  Checked before any device work.  RSR_ERR_ARG: null handle, null ctrl, null out or an out with all
 * six members NULL, K < 1, T < 1, nsteps < 1, unknown flag bits, env_ids with count < 1, sensordata requested with no sensor
 * table set, M K or T nsteps at or above 2^31.  RSR_ERR_UNSUPPORTED: a non-NULL member among the last five leaves
 * (RSR_DR_BODY_IPOS ..) on a model whose kernels lack them (the Airbot ones), as rsr_batch_set_dr_field. */
typedef struct rsr_param_samples { const float* leaf[RSR_DR_COUNT]; } rsr_param_samples;
#define RSR_PR_CTRL_PER_SAMPLE 1     /* ctrl is [M, K, T, nu]; without it [M, T, nu], shared by a slot's K samples */
int rsr_physics_param_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl,
                               const rsr_param_samples* params, int K, int T, int nsteps, int flags,
                               const rsr_rollout_out* out, void* hip_stream);

/* Closed-loop rollouts, for iLQR / iLQG forward passes, MPPI with a feedback term, CEM over controller gains and identification
 * from logs recorded under a controller: rsr_physics_param_rollouts in every respect but one (one wavefront per (env, sample),
 * the record read only, rows indexed by slot, params NULL or partly NULL, applied forces held for all T control steps).  At the
 * start of control step t the control is computed from the sample's own current state (the record's at t = 0, the state after
 * control step t-1 otherwise):
 *   dq  = mj_differentiatePos(qpos_ref[., t], qpos) with dt = 1: qpos (-) qpos_ref in the tangent space [nv]; a free joint's
 *         rotation is the rotation vector of conj(q_ref) q, as rsr_physics_transition_fd takes its differences, and exactly 0
 *         where q equals q_ref bit for bit: a sample on the reference trajectory with the reference's ctrl stays on it
 *   dv  = qvel - qvel_ref[., t]                                                                          [nv]
 *   u_j = ctrl[., t, j] + sum_{i < nv} gain[., t, j, i] dq_i + sum_{i < nv} gain[., t, j, nv + i] dv_i
 *         accumulated in that order from ctrl[., t, j], one fp32 fma per term
 *   u_j = clamp(u_j, actuator_ctrlrange_j)     only with RSR_FB_CLAMP and actuator_ctrllimited_j
 * and u is held for the control step's nsteps substeps.  An iLQR line search folds its alpha k_t into a per-sample ctrl.
 * ctrl: device float32 [M, T, nu], or with RSR_FB_CTRL_PER_SAMPLE [M, K, T, nu].  fb: gain [M, T, nu, 2 nv], qpos_ref [M, T, nq]
 * and qvel_ref [M, T, nv], shared by the K samples of a slot, or with RSR_FB_PER_SAMPLE [M, K, T, ..] all three.  params, out,
 * env_ids, K, T, nsteps: as rsr_physics_param_rollouts.  ctrl_out: NULL, or device float32 [M, K, T, nu] that receives the u that
 * was applied.  Only the buffers of out and ctrl_out are written: the record, every buffer of the handle, the batch's own leaf
 * tensors and the PRNG keys are untouched; the handle owns no buffer for this call.  An id outside [0, num_envs) runs nothing and
 * its slot's rows, those of ctrl_out included, are left alone.  Checked before any device work.  RSR_ERR_ARG: everything
 * rsr_physics_param_rollouts refuses, except that an out with all six members NULL is refused only when ctrl_out is NULL too (a
 * NULL out always is); a NULL fb or an fb with a NULL member; unknown flag bits.  RSR_ERR_UNSUPPORTED: as rsr_physics_param_rollouts. */
typedef struct rsr_feedback { const float* gain; const float* qpos_ref; const float* qvel_ref; } rsr_feedback;
#define RSR_FB_CTRL_PER_SAMPLE 1   /* ctrl is [M,K,T,nu]; without it [M,T,nu]                          */
#define RSR_FB_PER_SAMPLE      2   /* gain / qpos_ref / qvel_ref rows are [M,K,T,..]; without it [M,T,..] */
#define RSR_FB_CLAMP           4   /* clamp u to actuator_ctrlrange where actuator_ctrllimited         */
int rsr_physics_feedback_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl,
                                  const rsr_feedback* fb, const rsr_param_samples* params, int K, int T, int nsteps,
                                  int flags, const rsr_rollout_out* out, float* ctrl_out, void* hip_stream);

/* Cost rollouts, for MPPI, predictive sampling and CEM (the cost of every control sequence), an iLQR line search (the cost of
 * every alpha of rsr_physics_feedback_rollouts) and system identification (the loss of every leaf set against a log): the
 * rollouts above with the running cost of each sample formed on the device, [M, K] numbers out instead of [M, K, T, width]
 * trajectories.  One launch, one wavefront per (env, sample).
 * The rollout.  Sample (s, k) runs exactly the rollout of rsr_physics_feedback_rollouts with the same ctrl, fb, params, flags
 * (RSR_FB_*), K, T and nsteps, or with fb NULL (open loop) exactly that of rsr_physics_param_rollouts, RSR_FB_CTRL_PER_SAMPLE
 * standing for RSR_PR_CTRL_PER_SAMPLE: the trajectory is the same bit for bit, and so are the rows of traj (NULL or all-NULL:
 * nothing recorded) and of out->ctrl (the u that was applied: ctrl_out of rsr_physics_feedback_rollouts; open loop, ctrl itself).
 * The residuals are taken at the end of control step t, from the state after that step's last integration (the state row t of
 * traj holds), against row [s, t] of the references, which the K samples of a slot share:
 *   dq = qpos (-) qpos_ref[s, t]      in the tangent space [nv]: mj_differentiatePos as rsr_physics_feedback_rollouts takes it,
 *                                     exactly 0 where the two are equal bit for bit
 *   dv = qvel - qvel_ref[s, t]        [nv]
 *   du = u_t - ctrl_ref[s, t]         [nu]; u_t: the control that was applied in step t, after feedback and clamp
 *   ds = sensordata_t - sensor_ref[s, t]   [nsensordata]; sensordata_t: the sensordata row t of traj
 * The cost.  c_t = 1/2 (sum w_qpos dq^2 + sum w_qvel dv^2 + sum w_ctrl du^2 + sum w_sensor ds^2), cost = sum over t of c_t, in
 * fp32 and in a fixed order: entry i of each term is (w_i d_i) d_i, two roundings; lane i of the wavefront adds its entries of
 * the four terms in the order qpos, qvel, ctrl, sensor (a term that is off, or that has no entry i, adds +0), no contraction; the
 * 64 lane sums are added by the kernels' wave_sum (a fixed tree: pairs, quads, eights, rows of 16 lanes, then
 * (row 3 + row 2) + (row 1 + row 0)) and halved: c_t; cost accumulates c_t from +0 for t = 0 .. T-1.  terms: the same with each term's lane entries alone,
 * four sums.  A sample's outputs depend on that sample's inputs alone, bit for bit: not on M, K, the slot's position, on which
 * optional outputs are requested, or on the run.  A terminal cost is a heavier row T-1; time-varying weights are the rows.
 * Weights are read as given (the sign and size are the caller's; a bound on the rounding error assumes weights >= 0), and
 * non-finite states propagate into the cost: there is no status word.
 * cost (struct rsr_cost): device float32, rows by slot.  A NULL weight turns its term off and its reference is not read (qpos_ref
 * and qvel_ref still are for out->dx); a NULL qvel_ref, ctrl_ref or sensor_ref stands for zeros.
 * out (struct rsr_cost_out): device float32, rows by (slot, sample); cost is required, the others are written when not NULL.
 * Nothing but the buffers of traj and out is written: the record, every buffer of the handle, the batch's own leaf tensors and
 * the PRNG keys are untouched; the handle owns no buffer for this call.  An id outside [0, num_envs) runs nothing and its slot's
 * rows are left alone, in every output.  Checked before any device work.  RSR_ERR_ARG: everything
 * rsr_physics_feedback_rollouts refuses, except that fb may be NULL and traj may be NULL or all-NULL; an fb with a NULL member;
 * RSR_FB_PER_SAMPLE or RSR_FB_CLAMP with fb NULL; a NULL cost, out or out->cost; all four weights NULL; w_qpos, or out->dx,
 * without qpos_ref; w_sensor or sensor_ref with no sensor table set.  RSR_ERR_UNSUPPORTED: as rsr_physics_param_rollouts. */
typedef struct rsr_cost {            /* device float32, rows by slot, shared by a slot's K samples */
  const float *qpos_ref;   /* [M, T, nq]   required when w_qpos is given                 */
  const float *qvel_ref;   /* [M, T, nv]   NULL: zeros                                   */
  const float *ctrl_ref;   /* [M, T, nu]   NULL: zeros                                   */
  const float *sensor_ref; /* [M, T, nsensordata] NULL: zeros                            */
  const float *w_qpos, *w_qvel, *w_ctrl, *w_sensor;  /* [M, T, nv|nv|nu|nsensordata]; NULL: that term is off and its ref is not read */
} rsr_cost;
typedef struct rsr_cost_out {
  float *cost;       /* [M, K]            required: sum over t of step cost              */
  float *step_cost;  /* [M, K, T]         optional                                       */
  float *terms;      /* [M, K, 4]         optional: the four terms' sums over t (qpos, qvel, ctrl, sensor) */
  float *dx;         /* [M, K, T, 2 nv]   optional: dq | dv of every control step        */
  float *ctrl;       /* [M, K, T, nu]     optional: the u that was applied (ctrl_out of feedback_rollouts) */
} rsr_cost_out;
int rsr_physics_cost_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl,
                              const rsr_feedback* fb /* NULL: open loop */, const rsr_param_samples* params,
                              const rsr_cost* cost, int K, int T, int nsteps, int flags /* RSR_FB_* */,
                              const rsr_rollout_out* traj /* NULL or all-NULL: nothing recorded */,
                              const rsr_cost_out* out, void* hip_stream);

/* Applied forces (MuJoCo's data.xfrc_applied / data.qfrc_applied): per-env state of the handle, added in every forward pass of
 * rsr_physics_step (each substep), _forward, _forward_envs and _rollout (each substep, held for all T control steps):
 *   qfrc_smooth += qfrc_applied + sum over bodies b >= 1 of J_b(xipos_b)^T [f_b; tau_b]   (mj_xfrcAccumulate)
 * so they reach qacc, the constraint solve, the integration and the sensors.  Row 0 (the world body) is ignored.
 * on = 1: the calls above launch the applied-force kernels; on first use the buffers are allocated and zeroed, and turning them on
 * again keeps their values.  on = 0: the buffers are zeroed and the calls run the plain kernels again.  Waits for the device
 * (launches in flight read the buffers).  RSR_ERR_ARG: null handle, on outside {0, 1}.  rsr_physics_destroy frees the buffers. */
int rsr_physics_set_applied(rsr_physics* p, int on);

/* Writable zero-copy views (as rsr_physics_view) of the applied forces, device float32, row stride = width:
 *   RSR_A_XFRC_APPLIED  [nbody*6]  per body: force[3], torque[3], world frame, acting at the body's centre of mass
 *   RSR_A_QFRC_APPLIED  [nv]       generalised force
 * RSR_ERR_ARG while applied forces are off, or for an unknown id. */
enum rsr_applied_field { RSR_A_XFRC_APPLIED = 0, RSR_A_QFRC_APPLIED, RSR_A_COUNT };
int rsr_physics_applied_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);

/* The model at the current state, for model-based control: one launch that evaluates the record's qpos / qvel / ctrl with the
 * batch's per-env leaves and writes the handle's dynamics buffer.  It describes the state the record holds now, i.e. after the
 * integration of the last rsr_physics_step, whereas the side buffer of rsr_physics_view shows that step's last forward pass.
 * Nothing else is written: the record (qpos is not normalised; xpos, site_xpos, qacc_warmstart stay), the side buffer and
 * RSR_P_SENSORDATA are untouched, and no PRNG key advances.  Applied forces enter none of the outputs.
 *   RSR_D_QM             [nv*nv]    joint-space inertia, dense, symmetric, armature included (mj_fullM)
 *   RSR_D_QFRC_BIAS      [nv]       Coriolis, centrifugal and gravity forces
 *   RSR_D_QFRC_PASSIVE   [nv]       -damping * qvel
 *   RSR_D_QFRC_ACTUATOR  [nv]       gear * actuator_force, clamped to the joint's actfrcrange
 *                                   (qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator, plus any applied forces)
 *   RSR_D_JAC            [K*6*nv]   per Jacobian site k: jacp rows x, y, z then jacr rows x, y, z, each [nv], world frame
 *                                   (mj_jacSite); columns of dofs that do not move the site's body are 0
 *   RSR_D_JAC_SITE_XPOS  [K*3]      the sites' world positions, where the Jacobians were taken
 * K is the number of sites of rsr_physics_set_jac_sites (0 until set: width 0).  The buffer is allocated and zeroed by the first
 * of these three calls; the views' pointers and row stride do not move afterwards.  rsr_physics_destroy frees it. */
#define RSR_MAX_JAC_SITES 8
enum rsr_dynamics_field {
  RSR_D_QM = 0, RSR_D_QFRC_BIAS, RSR_D_QFRC_PASSIVE, RSR_D_QFRC_ACTUATOR, RSR_D_JAC, RSR_D_JAC_SITE_XPOS,
  RSR_D_COUNT
};
/* site_ids: nsite site ids (host memory), at most RSR_MAX_JAC_SITES; nsite = 0 clears the table.  Checked before any device work
 * (null handle, nsite outside [0, RSR_MAX_JAC_SITES], a null table, an id outside [0, nsite of the model): RSR_ERR_ARG); on
 * error the previous table stays.  Waits for the device (launches in flight read the table). */
int rsr_physics_set_jac_sites(rsr_physics* p, const int32_t* site_ids, int nsite);
/* env_ids: device int32 [count], or NULL for every env (count is ignored); ids outside [0, num_envs) are skipped.  Only the
 * listed envs' rows of the buffer are written.  RSR_ERR_ARG: null handle, env_ids with count < 1. */
int rsr_physics_dynamics(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream);
/* Zero-copy view (as rsr_physics_view) of one field of the dynamics buffer.  RSR_ERR_ARG for an unknown id. */
int rsr_physics_dynamics_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);

/* Constraint and contact forces: one launch that runs one mjx.forward pass at the record's current state -- its qpos / qvel / ctrl /
 * qacc_warmstart, the batch's per-env leaves and, while they are on, the handle's applied forces -- and writes the handle's
 * constraint buffer.  Like rsr_physics_dynamics it describes the state after the last integration.  Nothing else is written: the
 * record (qacc_warmstart, xpos and site_xpos included), the side buffer, RSR_P_SENSORDATA and the dynamics buffer are untouched,
 * and no PRNG key advances.  The pass is the one rsr_physics_forward would run on the same record: its qacc and contact list are
 * those bit for bit.  The row forces are evaluated at the solver's final qacc (MJX's _update_constraint), so
 * M qacc = qfrc_smooth + qfrc_constraint holds to the solver's convergence (one Newton iteration on the Go2 models).
 * nefc_max and ncon_max: rsr_dims.  NPYR = 2 (condim - 1) pyramid edges per contact: 4 on the Go2 models, 6 on the Airbot ones;
 * the edges of a contact come in pairs (+, -) per direction: tangent 1, tangent 2, then torsion (condim 4). */
enum rsr_constraint_field {
  RSR_C_QFRC_CONSTRAINT = 0,  /* [nv]           J^T efc_force at the solver's final qacc */
  RSR_C_QACC,                 /* [nv]           qacc of this pass */
  RSR_C_EFC_COUNTS,           /* [4]            nefc, ne, nf, nl (active limits), as float */
  RSR_C_EFC_FORCE,            /* [nefc_max]     rows in the model's order: equality, dof friction, active limits,
                                                contacts x NPYR pyramid edges; rows >= nefc are 0 */
  RSR_C_NCON,                 /* [1] */
  RSR_C_CONTACT,              /* [ncon_max*9]   as RSR_P_CONTACT, same slots */
  RSR_C_CONTACT_WRENCH,       /* [ncon_max*7]   per slot: normal force (>= 0), force[3], torque[3] in the world frame,
                                                acting on geom2's body at the contact point (geom1's body gets the
                                                negative); torque is the torsional moment about the normal, 0 for condim 3;
                                                slots >= ncon are 0 */
  RSR_C_COUNT
};
/* env_ids: device int32 [count], or NULL for every env (count is ignored); ids outside [0, num_envs) are skipped.  Only the
 * listed envs' rows of the buffer are written.  RSR_ERR_ARG: null handle, env_ids with count < 1; checked before any device
 * work.  The buffer is allocated and zeroed by the first of these two calls; the views' pointers and row stride do not move
 * afterwards.  rsr_physics_destroy frees it. */
int rsr_physics_constraint(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream);
/* Zero-copy view (as rsr_physics_view) of one field of the constraint buffer.  RSR_ERR_ARG for an unknown id. */
int rsr_physics_constraint_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);

/* Transition Jacobians by finite differences (MuJoCo's mjd_transitionFD).  With x = (qpos, qvel) and u = ctrl as the record holds
 * them and F = rsr_physics_step(u, nsteps), one launch evaluates, for every listed env and every column k of
 * ncol = 2 nv + nu, the two perturbed runs and their difference:
 *   k < nv            qpos moved by mj_integratePos(qpos, +-eps e_k): hinge / slide and free-joint translations add, a free joint's
 *                     rotation multiplies its quaternion on the right by exp(+-eps e / 2)
 *   nv <= k < 2 nv    qvel[k - nv] +- eps
 *   2 nv <= k         ctrl[k - 2 nv] +- eps, with no ctrl-range handling (MuJoCo nudges ctrl back into its range; this does not)
 * Every run starts from the record's qacc_warmstart and carries the warm start across its nsteps substeps as rsr_physics_step
 * does, with the batch's per-env leaves and, while they are on, the handle's applied forces: each run is bit for bit the
 * rsr_physics_step it stands for.  Rows 0 .. nv-1 of a column are mj_differentiatePos(y+.qpos, y-.qpos) / h, rows nv .. 2 nv-1
 * (y+.qvel - y-.qvel) / h, and with a sensor table set the rows of C and D are (sensordata+ - sensordata-) / h, sensordata being
 * that of the run's last forward pass (as RSR_P_SENSORDATA after rsr_physics_step).  RSR_FD_CENTERED: h = 2 eps; without it the
 * second run is the unperturbed state and h = eps.  These are finite differences of the step at the given eps, not its
 * derivative: friction loss, limits and contact activation make the step piecewise smooth at the scale of any usable eps.
 * Nothing but the handle's transition buffer (and, with RSR_FD_STATES, its states buffer) is written: the record, the side
 * buffer, RSR_P_SENSORDATA, the dynamics buffer and the constraint buffer are untouched, and no PRNG key advances.
 * One wavefront per (env, column).
 *   RSR_T_COLUMNS   [ncol * (2 nv + RSR_MAX_SENSORDATA)]  column-major: per column k a row of d qpos [nv], d qvel [nv],
 *                                                         d sensordata [nsensordata]; the rest of the row is written as 0.  A = rows of
 *                                                         columns k < 2 nv, entries < 2 nv, transposed; B: columns k >= 2 nv
 *   RSR_T_STATES_X  [ncol * 2 * (nq + nv + nu)]           with RSR_FD_STATES: per column and run (+eps; then -eps or the
 *                                                         unperturbed state) the perturbed qpos, qvel, ctrl
 *   RSR_T_STATES_Y  [ncol * 2 * (nq + nv)]                and that run's end state qpos, qvel
 * env_ids: device int32 [count], or NULL for every env (count is ignored); ids outside [0, num_envs) are skipped.  Only the
 * listed envs' rows are written.  RSR_ERR_ARG, checked before any device work: null handle, nsteps outside [1, 2^30), eps not finite or <= 0,
 * unknown flag bits, env_ids with count < 1.  The transition buffer is allocated and zeroed by the first call that needs it, the
 * states buffer by the first call with RSR_FD_STATES or the first view of it; the views' pointers and row strides do not move
 * afterwards.  rsr_physics_destroy frees them. */
#define RSR_FD_CENTERED 1
#define RSR_FD_STATES 2
enum rsr_transition_field { RSR_T_COLUMNS = 0, RSR_T_STATES_X, RSR_T_STATES_Y, RSR_T_COUNT };
int rsr_physics_transition_fd(rsr_physics* p, const int32_t* env_ids, int count, int nsteps, float eps, int flags, void* hip_stream);
/* Zero-copy view (as rsr_physics_view) of the transition buffer or of one half of the states buffer.  RSR_ERR_ARG for an unknown id. */
int rsr_physics_transition_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);

/* Transition Jacobians along a trajectory, for the backward pass of iLQR, time-varying LQR, linearised MPC and EKF smoothing over
 * a log: what T rounds of rsr_physics_transition_fd then rsr_physics_step would give, without advancing the env and with every
 * column of every control step in one launch.  M = count, or num_envs with env_ids NULL; slot s is env e = env_ids[s], and an id
 * may appear more than once.  Rows of ctrl and of out are indexed by slot s, the position in env_ids, not by env id.
 * ctrl: device float32 [M, T, nu].
 * Nominal trajectory: from the record of env e as it stands (qpos, qvel, qacc_warmstart, time), ctrl[s, t] then nsteps x mjx.step
 * for t = 0 .. T-1, with env e's per-env leaves and, while they are on, its applied forces (held for all T control steps): bit for
 * bit what rsr_physics_sample_rollouts with K = 1 records.  out->qpos [M, T+1, nq] and out->qvel [M, T+1, nv] are optional (NULL:
 * not recorded): row 0 is the start state, row t+1 the state after control step t.
 * out->columns, required: [M, T, ncol, 2 nv + nsensordata] with ncol = 2 nv + nu; the rows are tight, not padded to
 * RSR_MAX_SENSORDATA (the buffer is the caller's).  Block (s, t) equals, bit for bit, the first 2 nv + nsensordata entries of every
 * RSR_T_COLUMNS row that rsr_physics_transition_fd(nsteps, eps, flags) would write on a record advanced by t calls of
 * rsr_physics_step(ctrl[:, 0 .. t-1], nsteps) and holding ctrl[s, t] as its ctrl, the warm start the nominal run carried to step t
 * included: both perturbed runs of a column start from it, as rsr_physics_transition_fd starts from the record's.  Columns, eps and
 * the differences are those of rsr_physics_transition_fd.
 * flags: RSR_FD_CENTERED or 0; RSR_FD_STATES and unknown bits are RSR_ERR_ARG.
 * Two launches on hip_stream: the nominal run, one wavefront per slot, then one wavefront per (slot, t, column).  The record is
 * read only.  Only the buffers of out and the handle's nominal scratch are written: the side buffer, RSR_P_SENSORDATA, the
 * dynamics, constraint, transition, states and inverse buffers, the batch's own leaf tensors and the PRNG keys are untouched.
 * The nominal scratch holds qpos | qvel | qacc_warmstart before each control step, M T (nq + 2 nv) floats.  It is allocated by the
 * first call that needs it and replaced only by a call that needs more, which waits for the device first (launches in flight read
 * it); rsr_physics_destroy frees it.  Two calls on one handle must not overlap on different streams: they share the scratch.
 * env_ids: device int32 [count], or NULL for every env (count is ignored); an id outside [0, num_envs) runs nothing and its slot's
 * rows in all three buffers are left alone.  RSR_ERR_ARG, checked before any device work: null handle, null ctrl, null out or null
 * out->columns, T < 1, nsteps outside [1, 2^30), eps not finite or <= 0, bad flags, env_ids with count < 1, T nsteps or
 * M T ncol at or above 2^31. */
typedef struct rsr_trajectory_fd_out { float* columns; float* qpos; float* qvel; } rsr_trajectory_fd_out;
int rsr_physics_trajectory_fd(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, int T, int nsteps,
                              float eps, int flags, const rsr_trajectory_fd_out* out, void* hip_stream);

/* LQR backward pass, the step between rsr_physics_trajectory_fd and rsr_physics_feedback_rollouts in an iLQR iteration: the
 * time-varying Riccati recursion of Tassa, Erez and Todorov 2012 (the unregularised Q in the value update) on M independent
 * problems, one launch with one wavefront per slot.  The handle supplies nv, nu, the device and the family's launch entry only: the
 * call reads neither the model nor the record, takes no env_ids, and the M slots are whatever the caller's buffers hold.  All
 * pointers are device float32; nx = 2 nv, ncol = nx + nu.
 * columns: [M, T, ncol, row_stride], row_stride >= nx: the buffer rsr_physics_trajectory_fd writes, passed as it is with
 * row_stride = 2 nv + nsensordata; A_t[i][j] = columns[s, t, j, i] for j < nx, B_t[i][j] = columns[s, t, nx + j, i], state
 * differences in the tangent space (mj_differentiatePos).  Entries at index nx and above of a row are never read.
 * cost: lx [M, T+1, nx] and lxx [M, T+1, nx, nx], row T the terminal cost; lu [M, T, nu], luu [M, T, nu, nu], lux [M, T, nu, nx];
 * lux may be NULL (zero: bit for bit what an all-zero lux gives), the other four are required.  lxx and luu are read as given: the
 * caller passes them symmetric.  mu: [M], one regularisation value per slot, read on the device.
 * From Vx = lx[T], Vxx = lxx[T], for t = T-1 .. 0:
 *   Qx  = lx_t + A^T Vx          Qu  = lu_t + B^T Vx
 *   Qxx = lxx_t + A^T Vxx A      Qux = lux_t + B^T Vxx A      Quu = luu_t + B^T Vxx B
 *   Quu~ = Quu + mu I,      Qux~ = Qux                        (flags = 0)
 *   Quu~ = Quu + mu B^T B,  Qux~ = Qux + mu B^T A             (RSR_LQR_REG_STATE)
 *   k = -Quu~^-1 Qu         K = -Quu~^-1 Qux~                 (Cholesky of Quu~)
 *   Vx  = Qx  + K^T Quu k + K^T Qu  + Qux^T k
 *   Vxx = Qxx + K^T Quu K + K^T Qux + Qux^T K, then Vxx = (Vxx + Vxx^T) / 2
 *   dv[0] += k^T Qu         dv[1] += 1/2 k^T Quu k
 * in fp32, every output element summed in a fixed order: a slot's result depends on that slot's inputs alone, bit for bit, whatever
 * M is and from run to run.
 * out: gain [M, T, nu, nx] = K_t, exactly the gain of rsr_feedback (u = ctrl + gain [dq; dv]); k [M, T, nu]; dv [M, 2], the
 * expected cost change at step size alpha being alpha dv[0] + alpha^2 dv[1]; status [M], as float; and, optional (NULL: not
 * recorded), vx [M, T+1, nx] and vxx [M, T+1, nx, nx], row T the terminal cost, row t the value after step t of the recursion.
 * gain, k, dv and status are required.
 * Failure: step t fails if a Cholesky pivot of Quu~ is <= 0 or not finite.  The slot stops there: status[s] = t, dv[s] = (0, 0),
 * rows t' > t of gain / k / vx / vxx keep what was written and rows t' <= t are left alone; the other slots are unaffected.  On
 * success status[s] = -1.  The caller raises mu[s] and calls again: no host sync is needed to adapt it.
 * Only the buffers of out are written: the record, every buffer of the handle, the batch's own leaf tensors and the PRNG keys are
 * untouched; the handle owns no buffer for this call.  RSR_ERR_ARG, checked before any device work: null handle, columns, cost,
 * mu or out; a NULL required member of cost or out; M < 1 or T < 1; row_stride < 2 nv; unknown flag bits; M (T+1) at or above
 * 2^31. */
typedef struct rsr_lqr_cost { const float* lx; const float* lu; const float* lxx; const float* luu; const float* lux; } rsr_lqr_cost;
typedef struct rsr_lqr_out  { float* gain; float* k; float* dv; float* status; float* vx; float* vxx; } rsr_lqr_out;
#define RSR_LQR_REG_STATE 1     /* regularise through the state: Quu + mu B^T B, Qux + mu B^T A; without it Quu + mu I */
int rsr_physics_lqr_backward(rsr_physics* p, int M, int T, const float* columns, int row_stride,
                             const rsr_lqr_cost* cost, const float* mu, int flags,
                             const rsr_lqr_out* out, void* hip_stream);

/* Control-limited LQR backward pass (box-DDP: Tassa, Mansard and Todorov 2014), the backward pass that agrees with the clamp of
 * rsr_physics_feedback_rollouts (RSR_FB_CLAMP): rsr_physics_lqr_backward with k_t the minimiser of the step's quadratic model over
 * a box, and the gain rows of the clamped controls zero.  columns, cost, mu, flags (RSR_LQR_REG_STATE or 0) and out are exactly
 * those of rsr_physics_lqr_backward, as are the layout, the one launch with one wavefront per slot and the fixed summation order.
 * box: lo, hi [M, T, nu], required: the bounds on the control *change* k_t, i.e. the caller passes ctrlrange - u_nom[t]; -inf / +inf:
 * no bound.  clamped [M, T, nu] (may be NULL): -1 where k_t sits at lo, +1 at hi, 0 where it is free.  qp [M, T, 2] (may be NULL):
 * the Newton steps taken and a code: 0 converged, 1 every control clamped, 2 max_iter reached, 3 the line search found no descent.
 * max_iter in [1, 64].
 * At step t, Qx .. Quu, Quu~ and Qux~ as in rsr_physics_lqr_backward; then with H = Quu~, g = Qu, l = lo[s, t], h = hi[s, t]:
 *   not (l_j <= h_j) for some j (a NaN included): the step fails, like a bad pivot
 *   x = min(max(0, l), h);  full = false;  c_prev = none
 *   for it = 0, 1, ...:
 *     grad_j = g_j + sum_i H_ji x_i                                  (one fma chain over i ascending, from g_j)
 *     c_j = (x_j == l_j and grad_j > 0) or (x_j == h_j and grad_j < 0)
 *     all c: code 1, stop
 *     full and c == c_prev: code 0, stop                             (a full Newton step and the set held: the face's minimiser)
 *     it == max_iter: code 2, stop
 *     Cholesky of Hm = H with the rows and columns of c replaced by the identity's; a bad pivot fails the step
 *     r_j = 0 where c_j, else g_j + sum_{i in c} H_ji x_i            (ascending, from g_j)
 *     y = -Hm^-1 r;  x*_j = x_j where c_j, else y_j;  d = x* - x;  c_prev = c
 *     l_j <= fl(x_j + d_j) <= h_j for every j: x = x*, full = true, next it
 *     full = false;  f(z) = 1/2 z^T H z + g^T z = sum_j (1/2 (H z)_j + g_j) z_j
 *     for n = 0 .. 19, a = 0.6^n (repeated fp32 products): z = min(max(fl(x + a d), l), h); take the first z with
 *       f(x) - f(z) >= 0.1 grad^T (x - z)
 *     none taken: code 3, stop;  else x = z
 *   k = x (a clamped entry is its bound bit for bit)
 *   K: the rows of the last c are 0, the others -Hm^-1 Qux~ with the factor of that c (taken now if the loop's last factor was of
 *   another set); code 1: K = 0 and no factor
 *   Vx, Vxx (from the unregularised Quu, Qux, symmetrised) and dv from these k, K by the formulas of rsr_physics_lqr_backward
 * Every loop is bounded: max_iter Newton steps, 20 trial points, nu columns.  qp[s, t, 0] is `it` at the stop.  H_ff is positive
 * definite wherever a factor exists, so the KKT conditions of a step's QP are sufficient for its minimiser.
 * With lo = -inf and hi = +inf everywhere, and with finite bounds that no step reaches, every buffer of out equals what
 * rsr_physics_lqr_backward writes bit for bit (x = 0, grad = r = g, nothing masked, the full step taken without the Armijo test),
 * clamped is 0 and qp is (1, 0).
 * Failure: as rsr_physics_lqr_backward: status[s] = t, dv[s] = (0, 0), rows t' <= t of every buffer of out and of clamped / qp are
 * left alone, rows t' > t keep what was written; on success status[s] = -1.
 * Only the buffers of out and of box are written; the handle owns no buffer for this call.
 * RSR_ERR_ARG, checked before any device work: everything rsr_physics_lqr_backward refuses; a NULL box, box->lo or box->hi;
 * max_iter outside [1, 64]. */
typedef struct rsr_lqr_box { const float* lo; const float* hi; float* clamped; float* qp; } rsr_lqr_box;
int rsr_physics_lqr_box(rsr_physics* p, int M, int T, const float* columns, int row_stride, const rsr_lqr_cost* cost,
                        const rsr_lqr_box* box, const float* mu, int max_iter, int flags, const rsr_lqr_out* out, void* hip_stream);

/* Cost expansion, the step between rsr_physics_cost_rollouts / rsr_physics_trajectory_fd and rsr_physics_lqr_backward in an iLQR
 * iteration: the weighted least-squares cost of rsr_physics_cost_rollouts, stated once as its struct rsr_cost, expanded to second
 * order about a nominal run into exactly the operands of rsr_lqr_cost, on M independent problems in one launch with one wavefront
 * per (slot, t'), t' = 0 .. T.  The handle supplies nv, nu, the device and the family's launch entry only: the call reads neither
 * the model nor the record, takes no env_ids, and the M slots are whatever the caller's buffers hold.  All pointers are device
 * float32; nx = 2 nv, ncol = nx + nu.
 * cost: the rows of rsr_physics_cost_rollouts, [M, T, width]: w_qpos, w_qvel [.., nv], w_ctrl [.., nu], w_sensor [.., ny]; a NULL
 * weight switches its term off.  ctrl_ref [.., nu] and sensor_ref [.., ny]: NULL stands for zeros.  qpos_ref and qvel_ref are not
 * read: the state residual arrives already formed, as nominal->dx.
 * nominal (struct rsr_cost_nominal): the residual sources on the nominal run.  dx [M, T, nx]: dq | dv at the end of control step t,
 * exactly the dx rows rsr_physics_cost_rollouts writes for the nominal sample; required when w_qpos or w_qvel is given.  ctrl
 * [M, T, nu]: the control that was applied; required with w_ctrl.  sensordata [M, T, ny]: required with w_sensor.
 * columns: [M, T, ncol, row_stride], row_stride >= nx + ny: the buffer rsr_physics_trajectory_fd writes, passed as it is, so
 * C_t[j][a] = columns[s, t, a, nx + j] and D_t[j][p] = columns[s, t, nx + p, nx + j]; required with w_sensor and not read without
 * it.  Entries below nx and entries at or above nx + ny of a row are never read.
 * out (struct rsr_cost_expansion): lx [M, T+1, nx], lu [M, T, nu], lxx [M, T+1, nx, nx], luu [M, T, nu, nu], lux [M, T, nu, nx];
 * all five are required and every element of all five is written.  With du = ctrl - ctrl_ref, ds = sensordata - sensor_ref and
 * W = diag(w_sensor[s, t]):
 *   state part of cost row t  -> index t+1:  lx[t+1] = [w_qpos . dq | w_qvel . dv]   lxx[t+1] = diag(w_qpos | w_qvel)
 *   ctrl part of cost row t   -> index t:    lu[t]   = w_ctrl . du                    luu[t]   = diag(w_ctrl)
 *   sensor part of cost row t -> index t:    lx[t]  += C_t^T (W ds)    lu[t]  += D_t^T (W ds)
 *                                            lxx[t] += C_t^T W C_t     luu[t] += D_t^T W D_t     lux[t] = D_t^T W C_t
 * Row 0 of lx / lxx holds the sensor part only; row T holds the state part of cost row T-1 only (the terminal cost).  A term that
 * is off contributes nothing: its entries are +0 and its residual source is not read.
 * This is the Gauss-Newton expansion.  It is the exact Hessian for the ctrl and qvel terms and for the hinge, slide and translation
 * entries of the qpos term.  For a free joint's rotation the Jacobian of dq with respect to a right-multiplied perturbation is taken
 * as the identity, which is first order in the rotation error: rsr_physics_trajectory_fd perturbs on the right and
 * mj_differentiatePos differences in the same local frame, so the two are consistent.  The sensors' second derivatives are dropped.
 * With weights >= 0, lxx and luu are positive semi-definite by construction.
 * Arithmetic: fp32, no contraction (every product and every sum rounds once).  Every output element is one chain in a fixed order:
 * it starts from its state or ctrl part (w . residual, or the weight on the diagonal; +0 where there is none) and adds the sensor
 * entries j = 0 .. ny-1 ascending, c_a[j] g[j] with g[j] = w_sensor[j] ds[j] for lx / lu and (c_a[j] c_b[j]) w_sensor[j] for lxx /
 * luu / lux (c_a: row a of columns).  A problem's result therefore depends on its own inputs alone, bit for bit, whatever M is and
 * from run to run.  Two guarantees follow:
 *   1. with w_sensor NULL, lx[t+1] is the single fp32 product w . dx[t] bit for bit, lu[t] is w_ctrl . (ctrl - ctrl_ref) with one
 *      subtraction and one product, lxx and luu are exactly diagonal with exactly the weights on the diagonal, and lux, lx[0] and
 *      lxx[0] are exactly +0;
 *   2. lxx and luu are symmetric bit for bit: the product (c_a c_b) commutes and is weighted afterwards.
 * Only the five buffers of out are written: the record, every buffer of the handle, the batch's own leaf tensors and the PRNG keys
 * are untouched; the handle owns no buffer for this call.  RSR_ERR_ARG, checked before any device work: a null handle, cost, nominal
 * or out; a NULL member of out; M < 1 or T < 1; ny outside [0, RSR_MAX_SENSORDATA]; no weight given at all; w_qpos or w_qvel
 * without nominal->dx; w_ctrl without nominal->ctrl; w_sensor with ny == 0, without nominal->sensordata or without columns;
 * row_stride < nx + ny when columns is read; M (T+1) at or above 2^31. */
typedef struct rsr_cost_nominal { const float* dx; const float* ctrl; const float* sensordata; } rsr_cost_nominal;
typedef struct rsr_cost_expansion { float* lx; float* lu; float* lxx; float* luu; float* lux; } rsr_cost_expansion;
int rsr_physics_cost_expand(rsr_physics* p, int M, int T, const float* columns, int row_stride, int ny, const rsr_cost* cost,
                            const rsr_cost_nominal* nominal, const rsr_cost_expansion* out, void* hip_stream);

/* Kalman filter and smoother, the estimation dual of rsr_physics_lqr_backward: a linear time-varying Kalman filter with a
 * Rauch-Tung-Striebel smoother on M independent problems, one launch with one wavefront per slot and all T steps inside it.  The
 * state is the deviation dx_t from a nominal trajectory in the tangent space (mj_differentiatePos), nx = 2 nv: an error-state /
 * linearised EKF.  The handle supplies nv, nu, the device and the family's launch entry only: the call reads neither the model nor
 * the record, takes no env_ids, and the M slots are whatever the caller's buffers hold.  All pointers are device float32.
 * columns: [M, T, ncol, row_stride], ncol = nx + nu: the buffer rsr_physics_trajectory_fd writes, passed as it is.  Of row j < nx of
 * block (s, t), entry i < nx is A_t[i][j] and entry nx + r, r < ny, is C_t[r][j]; rows j >= nx (B, D) and entries at or beyond
 * nx + ny are never read.  1 <= ny <= RSR_MAX_SENSORDATA and nx + ny <= row_stride.  C_t is the Jacobian of step t's sensordata
 * with respect to the state before step t, so the model is dx_{t+1} = A_t dx_t + w_t, dy_t = C_t dx_t + v_t.
 * in: dy [M, T, ny], the measured sensordata minus the nominal run's (rsr_physics_sample_rollouts with K = 1 on the same record);
 * r [M, T, ny], the measurement variances (R_t diagonal; +inf: that sample is missing and is skipped exactly); q [M, T, nx], the
 * process-noise variances (Q_t diagonal, finite and >= 0); x0 [M, nx], may be NULL (zeros); P0 [M, nx, nx], read as given: the
 * caller passes it symmetric.  Because R_t is diagonal the update takes one sensor entry at a time, ascending:
 *   x = x0, P = P0
 *   for t = 0 .. T-1:
 *     for j = 0 .. ny-1 with r_tj != +inf:
 *       w = P c_j (c_j: row j of C_t);  s = c_j . w + r_tj;  nu = dy_tj - c_j . x
 *       x += w (nu / s);  P[i][k] = fma(-(w_i w_k), 1 / s, P[i][k])          (P stays symmetric bit for bit)
 *       nll += 1/2 (nu^2 / s + logf(s) + log 2 pi)
 *     xf[t] = x, pf[t] = P
 *     x = A_t x;  P = (S + S^T) / 2 + diag(q_t) with S = A_t P A_t^T
 *   xf[T] = x, pf[T] = P                  (a prediction: there is no measurement at T)
 * and, if out->xs is given, the smoother: xs[T] = xf[T], ps[T] = pf[T], for t = T-1 .. 0:
 *   Pm = the predict above on pf[t] (the same code, the same bits);  G = pf[t] A_t^T Pm^-1 (Cholesky of Pm)
 *   xs[t] = xf[t] + G (xs[t+1] - A_t xf[t]);  ps[t] = pf[t] + (E + E^T) / 2 with E = G (ps[t+1] - Pm) G^T
 * in fp32, every output element one lane's fma chain in a fixed order: a slot's result depends on that slot's inputs alone, bit for
 * bit, whatever M is and from run to run; with xs NULL the filter outputs are bit for bit those of the smoothing call; and entries
 * with r = +inf give bit for bit the result of the same problem with those sensor columns removed and ny smaller.
 * out: xf [M, T+1, nx] and status [M, 2] (as float) are required; pf [M, T+1, nx, nx] is required when smoothing; xs [M, T+1, nx]
 * turns the smoother on; ps [M, T+1, nx, nx] and nll [M] (the innovation negative log-likelihood) are optional (NULL: not
 * recorded).
 * Failure: status[s] = (filter, smoother), each -1 or the step t that failed.  A filter step fails if an r_tj is neither +inf nor
 * finite and > 0, or if an s is not finite and > 0: the slot stops there, rows < t of xf / pf keep what was written and rows >= t
 * are left alone, nll[s] = 0 and the smoother does not run.  A smoother step fails if a Cholesky pivot of Pm is <= 0 or not
 * finite: rows <= t of xs / ps are left alone, rows > t keep what was written.  The other slots are unaffected.
 * Only the buffers of out are written: the record, every buffer of the handle, the batch's own leaf tensors and the PRNG keys are
 * untouched; the handle owns no buffer for this call.  RSR_ERR_ARG, checked before any device work: null handle, columns, in or
 * out; a NULL dy, r, q, P0, xf or status; xs or ps without pf; ps without xs; M < 1 or T < 1; ny outside
 * [1, RSR_MAX_SENSORDATA]; row_stride < 2 nv + ny; unknown flag bits (there are none yet: flags must be 0); M (T+1) at or above
 * 2^31. */
typedef struct rsr_kalman_in  { const float* dy; const float* r; const float* q; const float* x0; const float* P0; } rsr_kalman_in;
typedef struct rsr_kalman_out { float* xf; float* pf; float* xs; float* ps; float* nll; float* status; } rsr_kalman_out;
int rsr_physics_kalman(rsr_physics* p, int M, int T, const float* columns, int row_stride, int ny,
                       const rsr_kalman_in* in, int flags, const rsr_kalman_out* out, void* hip_stream);

/* Inverse kinematics on site pose targets: which qpos puts these sites there.  Damped least squares (Levenberg-Marquardt with a
 * fixed damping) on M independent problems, one launch with one wavefront per slot and every iteration inside it.  Slot s takes
 * its model, its per-env leaves (the Go2 qpos0 leaf moves the kinematics) and its default start from env env_ids[s] (env_ids
 * NULL: M = the batch's envs, env s); an env may be listed more than once, and an id out of range leaves its slot's rows alone.
 * task (host memory, shared by every slot, passed to the kernel by value: no device table, no state in the handle, independent of
 * rsr_physics_set_jac_sites): nsite sites in [1, RSR_MAX_JAC_SITES], pos_weight[k] >= 0 and rot_weight[k] >= 0 (0: that row is
 * off; not all zero), dofs: bit i set = dof i may move (free-joint dofs allowed; nv <= 32).
 * in (device float32): target_pos [M, nsite, 3]; target_quat [M, nsite, 4] (w, x, y, z; normalised on the device as the
 * kinematics normalises a free joint's quaternion) or NULL, then every rot_weight must be 0; qpos0 [M, nq] or NULL: the record's
 * qpos of the slot's env; damping [M], lambda per slot, read on the device.
 * opt: iters >= 0, tol_pos >= 0, tol_rot >= 0 (0: every iteration runs), max_step >= 0 (0: no cap), limits 0 or 1.
 *   q = start
 *   for it = 0, 1, ...:
 *     kinematics(q)                          (it normalises free-joint quaternions in q, as MJX does)
 *     e_k = p*_k - p_k, r_k = the rotation vector of R*_k R_k^T (world frame, the short way round; R_k: the site's frame)
 *     perr = max_k |e_k| over pos_weight_k > 0, rerr = max_k |r_k| over rot_weight_k > 0
 *     if it == iters or (perr <= tol_pos and rerr <= tol_rot): stop, status 0 if the tolerances hold, else 1
 *     J = rows pos_weight_k jacp_k, rot_weight_k jacr_k (mj_jacSite, as rsr_physics_dynamics), the columns of dofs outside
 *         `dofs` zeroed; b = rows pos_weight_k e_k, rot_weight_k r_k
 *     dq = (J^T J + lambda I)^-1 J^T b       (L D L^T; a zeroed column gives dq = 0 exactly)
 *     if max|dq| > max_step > 0: dq *= max_step / max|dq|
 *     q = mj_integratePos(q, dq)             (a free joint's rotation dofs are a body-frame rotation vector: q (x) exp(dq / 2),
 *                                             normalised; a dof outside `dofs` is not touched)
 *     if limits: clamp hinge / slide q to jnt_range where jnt_limited
 * A lambda that is not finite and positive, or a dq that is not finite, ends the slot with status 2 at the last q; the other
 * slots are unaffected.  A slot's result depends on that slot's inputs alone, bit for bit.
 * out (device): qpos [M, nq] float32; err [M, 2] float32: perr, rerr of the last kinematics pass, i.e. at the returned qpos;
 * info [M, 2] int32: iterations taken, status.  iters = 0 is a forward-kinematics query: the start and its error.
 * Only the buffers of out are written: the record, every buffer of the handle, the batch's own leaf tensors and the PRNG keys are
 * untouched; the handle owns no buffer for this call.  RSR_ERR_ARG, checked before any device work: null handle, task, in, opt or
 * out; a NULL target_pos, damping, qpos, err or info; count < 1 with env_ids; nsite outside [1, RSR_MAX_JAC_SITES]; a site id out
 * of range; a weight that is negative or not finite; all weights zero; a positive rot_weight without target_quat; dofs with a bit
 * at or above nv; iters < 0; a tolerance or max_step that is negative or not finite; limits not 0 or 1. */
typedef struct rsr_ik_task { int32_t nsite; int32_t sites[RSR_MAX_JAC_SITES]; float pos_weight[RSR_MAX_JAC_SITES]; float rot_weight[RSR_MAX_JAC_SITES]; uint32_t dofs; } rsr_ik_task;
typedef struct rsr_ik_in   { const float* target_pos; const float* target_quat; const float* qpos0; const float* damping; } rsr_ik_in;
typedef struct rsr_ik_opt  { int32_t iters; float tol_pos; float tol_rot; float max_step; int32_t limits; } rsr_ik_opt;
typedef struct rsr_ik_out  { float* qpos; float* err; int32_t* info; } rsr_ik_out;
int rsr_physics_ik(rsr_physics* p, const int32_t* env_ids, int count, const rsr_ik_task* task, const rsr_ik_in* in,
                   const rsr_ik_opt* opt, const rsr_ik_out* out, void* hip_stream);

/* Inverse dynamics (mj_inverse / mjx.inverse): given an acceleration per env, the generalised force that must have acted
 * (data.qfrc_inverse).  One launch evaluates the record's current state -- its qpos / qvel / ctrl with the batch's per-env
 * leaves, the state after the last integration as rsr_physics_dynamics and rsr_physics_constraint see it -- at the caller's
 * qacc: the stages of one forward pass up to the constraint rows with their final aref, then the row law at jaref = J a - aref.
 * No Newton solve runs.  qacc: device float32 [num_envs][nv]; row e belongs to env e whether or not env_ids is given.
 *   RSR_I_QFRC_INVERSE     M a + qfrc_bias - qfrc_passive - qfrc_constraint (MuJoCo's definition): the total of everything
 *                          external, actuators included; subtract RSR_I_QFRC_ACTUATOR for the part the model does not explain
 *   RSR_I_QFRC_CONSTRAINT  J^T efc_force
 *   RSR_I_QACC             the continuous-time acceleration a the pass used: qacc itself, or its conversion (RSR_INV_DISCRETE)
 *   RSR_I_QFRC_ACTUATOR    the same expression as RSR_D_QFRC_ACTUATOR
 *   RSR_I_EFC_COUNTS       as RSR_C_EFC_COUNTS
 *   RSR_I_EFC_FORCE        the row forces of MJX's _update_constraint at a: equality rows -D jaref; friction-loss rows -D jaref
 *                          clamped to -+floss outside |jaref| < R floss; limit and contact rows -D min(jaref, 0).  Row order and
 *                          zero padding as RSR_C_EFC_FORCE
 * The handle's applied forces enter none of the outputs: the rows do not depend on them, and qfrc_inverse is what they would
 * have to sum to.  RSR_INV_DISCRETE: qacc is a discrete-time acceleration, (qvel_after - qvel_before) / timestep of one
 * substep.  Where the integrator solves (M + h D) qacc = M a (implicitfast, or Euler with non-zero damping and eulerdamp on) the
 * pass first undoes that: a = qacc + h M^-1 (damp * qacc) (mj_discreteAcc); otherwise a = qacc.
 * The constraints are soft with a large row stiffness D = 1 / R: an error d in qacc becomes up to D |J d| in force on an active
 * row, so forces from differenced fp32 velocities are noisy wherever a contact or a limit is active.
 * Nothing but the handle's inverse buffer is written: the record (qacc_warmstart, xpos and site_xpos included), the side buffer,
 * RSR_P_SENSORDATA and the dynamics, constraint and transition buffers are untouched, and no PRNG key advances.
 * env_ids: device int32 [count], or NULL for every env (count is ignored); ids outside [0, num_envs) are skipped.  Only the
 * listed envs' rows of the buffer are written.  RSR_ERR_ARG, checked before any device work: null handle, null qacc, unknown flag
 * bits, env_ids with count < 1, an unknown field id.  The buffer is allocated and zeroed by the first of these two calls; the
 * views' pointers and row stride do not move afterwards.  rsr_physics_destroy frees it. */
#define RSR_INV_DISCRETE 1
enum rsr_inverse_field {
  RSR_I_QFRC_INVERSE = 0, RSR_I_QFRC_CONSTRAINT, RSR_I_QACC, RSR_I_QFRC_ACTUATOR, RSR_I_EFC_COUNTS, RSR_I_EFC_FORCE,
  RSR_I_COUNT
};
int rsr_physics_inverse(rsr_physics* p, const float* qacc, const int32_t* env_ids, int count, int flags, void* hip_stream);
/* Zero-copy view (as rsr_physics_view) of one field of the inverse buffer.  RSR_ERR_ARG for an unknown id. */
int rsr_physics_inverse_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);

#ifdef __cplusplus
}
#endif
#endif /* RSR_PHYSICS_H_ */
