"""ctypes binding of librsrmjx.so (include/rsr_mjx.h).  Fails loudly when the library is missing:
there is no CPU or PyTorch fallback for the stepper."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

FIELDS = [
    "qpos", "qvel", "ctrl", "qacc_warmstart", "time", "xpos", "site_xpos",
    "obs", "reward", "done", "metrics",
    "info_target_pos", "info_new_cube_pos", "info_site_pos", "info_cube_pos", "info_last_action",
    "info_target_base_pos", "info_target_vertical_pos", "info_target_w", "info_new_T_pos", "info_T_pos", "info_xita", "info_go2",
    "info_steps", "info_truncation", "info_episode_done", "info_episode_metrics",
    "first_qpos", "first_qvel", "first_ctrl", "first_warmstart", "first_time", "first_xpos", "first_site_xpos",
    "first_obs", "privileged_obs", "first_privileged_obs", "stats",
]
FIELD_ID = {n: i for i, n in enumerate(FIELDS)}
DEBUG_FLOATS = 8192


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "nq", "nv", "nu", "nbody", "njnt", "ngeom", "nsite", "neq", "npair",
        "obs_dim", "nmetrics", "n_frames", "episode_length", "env_kind",
        "rec_floats", "ncon_max", "nefc_max", "lds_bytes")]


_lib = None

# every symbol include/rsr_mjx.h declares
# enum rsr_dr_field (include/rsr_mjx.h), in order
DR_FIELDS = [
    "geom_friction", "body_mass", "dof_damping", "dof_frictionloss",
    "body_ipos", "qpos0", "dof_armature", "actuator_gainprm", "actuator_biasprm",
]

# enum rsr_physics_field (include/rsr_physics.h), in order
PHYS_FIELDS = ["qacc", "actuator_force", "xquat", "ncon", "contact", "ncon_dropped", "sensordata"]

# every symbol include/rsr_physics.h declares
PHYS_SYMBOLS = ["rsr_physics_create", "rsr_physics_destroy", "rsr_physics_step", "rsr_physics_forward", "rsr_physics_forward_envs",
                "rsr_physics_view", "rsr_physics_set_sensors", "rsr_physics_rollout", "rsr_physics_set_applied",
                "rsr_physics_applied_view", "rsr_physics_set_jac_sites", "rsr_physics_dynamics", "rsr_physics_dynamics_view",
                "rsr_physics_constraint", "rsr_physics_constraint_view", "rsr_physics_transition_fd", "rsr_physics_transition_view",
                "rsr_physics_inverse", "rsr_physics_inverse_view", "rsr_physics_sample_rollouts", "rsr_physics_param_rollouts",
                "rsr_physics_feedback_rollouts", "rsr_physics_trajectory_fd", "rsr_physics_lqr_backward", "rsr_physics_ik",
                "rsr_physics_cost_rollouts", "rsr_physics_kalman", "rsr_physics_lqr_box", "rsr_physics_cost_expand"]

# enum rsr_applied_field (include/rsr_physics.h), in order
APPLIED_FIELDS = ["xfrc_applied", "qfrc_applied"]

# enum rsr_dynamics_field (include/rsr_physics.h), in order
DYNAMICS_FIELDS = ["qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "jac", "jac_site_xpos"]
MAX_JAC_SITES = 8

# enum rsr_constraint_field (include/rsr_physics.h), in order
CONSTRAINT_FIELDS = ["qfrc_constraint", "qacc", "efc_counts", "efc_force", "ncon", "contact", "contact_wrench"]

# enum rsr_transition_field and the RSR_FD_* flags (include/rsr_physics.h)
TRANSITION_FIELDS = ["columns", "states_x", "states_y"]
FD_CENTERED, FD_STATES = 1, 2

# enum rsr_inverse_field and the RSR_INV_* flags (include/rsr_physics.h)
INVERSE_FIELDS = ["qfrc_inverse", "qfrc_constraint", "qacc", "qfrc_actuator", "efc_counts", "efc_force"]
INV_DISCRETE = 1

# enum rsr_sensor_type (include/rsr_physics.h), in order, with each type's width
SENSOR_TYPES = ["gyro", "velocimeter", "accelerometer", "framepos", "framexaxis", "framezaxis", "framequat", "framelinvel",
                "frameangvel"]
SENSOR_WIDTH = {"gyro": 3, "velocimeter": 3, "accelerometer": 3, "framepos": 3, "framexaxis": 3, "framezaxis": 3, "framequat": 4,
                "framelinvel": 3, "frameangvel": 3}
MAX_SENSORDATA = 64


class RolloutOut(C.Structure):
    """struct rsr_rollout_out (include/rsr_physics.h): device pointers, NULL = not recorded."""
    _fields_ = [(n, C.c_void_p) for n in ("qpos", "qvel", "time", "actuator_force", "ncon", "sensordata")]


class ParamSamples(C.Structure):
    """struct rsr_param_samples (include/rsr_physics.h): device pointers [M, K, width] in DR_FIELDS order, NULL = the env's own leaf."""
    _fields_ = [("leaf", C.c_void_p * len(DR_FIELDS))]


# the RSR_PR_* flags (include/rsr_physics.h)
PR_CTRL_PER_SAMPLE = 1


class Feedback(C.Structure):
    """struct rsr_feedback (include/rsr_physics.h): device pointers, gain [.., T, nu, 2 nv], qpos_ref [.., T, nq], qvel_ref [.., T, nv]."""
    _fields_ = [(n, C.c_void_p) for n in ("gain", "qpos_ref", "qvel_ref")]


# the RSR_FB_* flags (include/rsr_physics.h)
FB_CTRL_PER_SAMPLE, FB_PER_SAMPLE, FB_CLAMP = 1, 2, 4


COST_REFS = ("qpos_ref", "qvel_ref", "ctrl_ref", "sensor_ref")
COST_WEIGHTS = ("w_qpos", "w_qvel", "w_ctrl", "w_sensor")


class Cost(C.Structure):
    """struct rsr_cost (include/rsr_physics.h): device pointers, rows by slot: the references [M, T, nq | nv | nu | nsensordata] and
    the weights [M, T, nv | nv | nu | nsensordata]; a NULL weight = the term is off, a NULL qvel / ctrl / sensor reference = zeros."""
    _fields_ = [(n, C.c_void_p) for n in COST_REFS + COST_WEIGHTS]


class CostOut(C.Structure):
    """struct rsr_cost_out (include/rsr_physics.h): device pointers, cost [M, K] (required), step_cost [M, K, T], terms [M, K, 4],
    dx [M, K, T, 2 nv] and ctrl [M, K, T, nu] (NULL = not written)."""
    _fields_ = [(n, C.c_void_p) for n in ("cost", "step_cost", "terms", "dx", "ctrl")]



class TrajectoryFdOut(C.Structure):
    """struct rsr_trajectory_fd_out (include/rsr_physics.h): device pointers, columns [M, T, ncol, 2 nv + nsd] (required), the nominal
    qpos [M, T+1, nq] and qvel [M, T+1, nv] (NULL = not recorded)."""
    _fields_ = [(n, C.c_void_p) for n in ("columns", "qpos", "qvel")]


class LqrCost(C.Structure):
    """struct rsr_lqr_cost (include/rsr_physics.h): device pointers, lx [M, T+1, nx], lu [M, T, nu], lxx [M, T+1, nx, nx],
    luu [M, T, nu, nu], lux [M, T, nu, nx] (NULL = zero); nx = 2 nv."""
    _fields_ = [(n, C.c_void_p) for n in ("lx", "lu", "lxx", "luu", "lux")]


class LqrOut(C.Structure):
    """struct rsr_lqr_out (include/rsr_physics.h): device pointers, gain [M, T, nu, nx], k [M, T, nu], dv [M, 2], status [M]
    (required), vx [M, T+1, nx] and vxx [M, T+1, nx, nx] (NULL = not recorded)."""
    _fields_ = [(n, C.c_void_p) for n in ("gain", "k", "dv", "status", "vx", "vxx")]


class LqrBox(C.Structure):
    """struct rsr_lqr_box (include/rsr_physics.h): device pointers, lo and hi [M, T, nu] (required; -inf / +inf = no bound), clamped
    [M, T, nu] and qp [M, T, 2] (NULL = not recorded)."""
    _fields_ = [(n, C.c_void_p) for n in ("lo", "hi", "clamped", "qp")]


class CostNominal(C.Structure):
    """struct rsr_cost_nominal (include/rsr_physics.h): device pointers, the residual sources of rsr_physics_cost_expand on the
    nominal run: dx [M, T, 2 nv] (needed by w_qpos / w_qvel), ctrl [M, T, nu] (by w_ctrl), sensordata [M, T, ny] (by w_sensor)."""
    _fields_ = [(n, C.c_void_p) for n in ("dx", "ctrl", "sensordata")]


class CostExpansion(C.Structure):
    """struct rsr_cost_expansion (include/rsr_physics.h): device pointers, the outputs of rsr_physics_cost_expand, all required:
    the members of struct rsr_lqr_cost, to be written."""
    _fields_ = [(n, C.c_void_p) for n in ("lx", "lu", "lxx", "luu", "lux")]


class KalmanIn(C.Structure):
    """struct rsr_kalman_in (include/rsr_physics.h): device pointers, dy [M, T, ny], r [M, T, ny] (+inf = missing), q [M, T, nx],
    x0 [M, nx] (NULL = zeros), P0 [M, nx, nx]; nx = 2 nv."""
    _fields_ = [(n, C.c_void_p) for n in ("dy", "r", "q", "x0", "P0")]


class KalmanOut(C.Structure):
    """struct rsr_kalman_out (include/rsr_physics.h): device pointers, xf [M, T+1, nx] and status [M, 2] (required), pf
    [M, T+1, nx, nx] (required with xs), xs [M, T+1, nx] (NULL = no smoother), ps [M, T+1, nx, nx] and nll [M] (NULL = not recorded)."""
    _fields_ = [(n, C.c_void_p) for n in ("xf", "pf", "xs", "ps", "nll", "status")]


# the RSR_LQR_* flags (include/rsr_physics.h)
LQR_REG_STATE = 1


class IkTask(C.Structure):
    """struct rsr_ik_task (include/rsr_physics.h): the site table, shared by every slot and passed by value: nsite, the site ids,
    the position and orientation weights (0 = off) and the dof mask (bit i: dof i may move)."""
    _fields_ = [("nsite", C.c_int32), ("sites", C.c_int32 * MAX_JAC_SITES), ("pos_weight", C.c_float * MAX_JAC_SITES),
                ("rot_weight", C.c_float * MAX_JAC_SITES), ("dofs", C.c_uint32)]


class IkIn(C.Structure):
    """struct rsr_ik_in (include/rsr_physics.h): device pointers, target_pos [M, nsite, 3], target_quat [M, nsite, 4] (NULL = no
    orientation rows), qpos0 [M, nq] (NULL = the record's qpos), damping [M]."""
    _fields_ = [(n, C.c_void_p) for n in ("target_pos", "target_quat", "qpos0", "damping")]


class IkOpt(C.Structure):
    """struct rsr_ik_opt (include/rsr_physics.h)"""
    _fields_ = [("iters", C.c_int32), ("tol_pos", C.c_float), ("tol_rot", C.c_float), ("max_step", C.c_float), ("limits", C.c_int32)]


class IkOut(C.Structure):
    """struct rsr_ik_out (include/rsr_physics.h): device pointers, qpos [M, nq] and err [M, 2] float32, info [M, 2] int32."""
    _fields_ = [(n, C.c_void_p) for n in ("qpos", "err", "info")]


SYMBOLS = [
    "rsr_model_create", "rsr_model_dims", "rsr_model_destroy", "rsr_batch_create", "rsr_batch_destroy",
    "rsr_batch_set_dr", "rsr_batch_set_dr_field", "rsr_batch_set_schedule", "rsr_batch_set_whole_envs", "rsr_batch_set_priority", "rsr_batch_set_action_repeat", "rsr_batch_check", "rsr_batch_set_fault_injection", "rsr_rollout_metrics", "rsr_reset", "rsr_step", "rsr_view", "rsr_batch_set_debug",
    "rsr_timing_begin", "rsr_timing_end", "rsr_last_error",
]


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RSR_MJX_LIB", _build.LIB)   # override: diagnostic builds (tools/gpu_stage_profile.py)
    # torch ships its own HIP runtime; import it first so librsrmjx.so binds to the same libamdhip64
    # (two runtimes in one process do not see each other's device context).
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -m rsr_mjx_amd.build` (hipcc, gfx950). "
            "The stepper has no CPU fallback.")
    L = C.CDLL(path)
    vp, i32, i64p = C.c_void_p, C.c_int, C.POINTER(C.c_int64)
    L.rsr_model_create.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.rsr_model_dims.argtypes = [vp, C.POINTER(Dims)]
    L.rsr_model_destroy.argtypes = [vp]
    L.rsr_model_destroy.restype = None
    L.rsr_batch_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.rsr_batch_set_dr_field.argtypes = [vp, i32, vp]
    L.rsr_batch_destroy.argtypes = [vp]
    L.rsr_batch_destroy.restype = None
    L.rsr_batch_set_dr.argtypes = [vp, vp, vp, vp, vp]
    L.rsr_reset.argtypes = [vp, vp, vp]
    L.rsr_step.argtypes = [vp, vp, vp]
    L.rsr_view.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p]
    L.rsr_physics_create.argtypes = [vp, C.POINTER(vp)]
    L.rsr_physics_destroy.argtypes = [vp]
    L.rsr_physics_destroy.restype = None
    L.rsr_physics_step.argtypes = [vp, vp, i32, vp]
    L.rsr_physics_forward.argtypes = [vp, vp]
    L.rsr_physics_forward_envs.argtypes = [vp, vp, i32, vp]
    L.rsr_physics_view.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p]
    L.rsr_physics_set_sensors.argtypes = [vp, vp, i32]
    L.rsr_physics_rollout.argtypes = [vp, vp, i32, i32, vp, vp]
    L.rsr_physics_set_applied.argtypes = [vp, i32]
    L.rsr_physics_applied_view.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p]
    L.rsr_physics_set_jac_sites.argtypes = [vp, vp, i32]
    L.rsr_physics_dynamics.argtypes = [vp, vp, i32, vp]
    L.rsr_physics_dynamics_view.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p]
    L.rsr_physics_constraint.argtypes = [vp, vp, i32, vp]
    L.rsr_physics_constraint_view.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p]
    L.rsr_physics_transition_fd.argtypes = [vp, vp, i32, i32, C.c_float, i32, vp]
    L.rsr_physics_transition_view.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p]
    L.rsr_physics_inverse.argtypes = [vp, vp, vp, i32, i32, vp]
    L.rsr_physics_inverse_view.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p]
    L.rsr_physics_sample_rollouts.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp, vp]
    L.rsr_physics_param_rollouts.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp]
    L.rsr_physics_feedback_rollouts.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.rsr_physics_cost_rollouts.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.rsr_physics_trajectory_fd.argtypes = [vp, vp, i32, vp, i32, i32, C.c_float, i32, vp, vp]
    L.rsr_physics_lqr_backward.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, vp, vp]
    L.rsr_physics_lqr_box.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp]
    L.rsr_physics_ik.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.rsr_physics_kalman.argtypes = [vp, i32, i32, vp, i32, i32, vp, i32, vp, vp]
    L.rsr_physics_cost_expand.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    L.rsr_batch_set_debug.argtypes = [vp, vp]
    L.rsr_batch_set_schedule.argtypes = [vp, i32]
    L.rsr_batch_set_whole_envs.argtypes = [vp, i32]
    L.rsr_batch_set_priority.argtypes = [vp, i32]
    L.rsr_batch_set_action_repeat.argtypes = [vp, i32]
    L.rsr_rollout_metrics.argtypes = [vp, vp, vp]
    L.rsr_batch_check.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.rsr_batch_set_fault_injection.argtypes = [vp, i32, i32]
    L.rsr_timing_begin.argtypes = [vp, vp]
    L.rsr_timing_end.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.rsr_last_error.restype = C.c_char_p
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"librsrmjx error {rc}: {lib().rsr_last_error().decode()}")
