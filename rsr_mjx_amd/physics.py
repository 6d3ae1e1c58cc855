"""Physics-level access to an env batch: the two calls every reference env is written against (_src/mjx_env.py:30-73).

    mjx_env.init(model, qpos, qvel, ctrl)      ->  Physics.set_state(qpos, qvel, ctrl)   (one mjx.forward)
    mjx_env.step(model, data, ctrl, n_substeps) ->  Physics.step(ctrl, nsteps)           (nsteps x mjx.step)
    mujoco.rollout.rollout / lax.scan(mjx.step)  ->  Physics.rollout(ctrl [N, T, nu])     (one launch, trajectories [N, T, w])
    mujoco.rollout on K copies of a state / vmap(lax.scan(mjx.step)) ->  Physics.sample_rollouts(ctrl [M, K, T, nu])
                                                                                          (K sequences per env from its current
                                                                                           state, [M, K, T, w]; the record stays)
    vmap over model leaves of lax.scan(mjx.step) ->  Physics.param_rollouts(ctrl [M, T, nu], {leaf: [M, K, ...]})
                                                                                          (K sets of model leaves per env from its
                                                                                           current state, [M, K, T, w]; no replica
                                                                                           batch, the record and the leaves stay)
    lax.scan of u = ctrl + gain (x (-) x_ref), mjx.step ->  Physics.feedback_rollouts(ctrl, gain, qpos_ref, qvel_ref)
                                                                                          (the same in closed loop: the control of
                                                                                           every control step from the sample's own
                                                                                           state, on the device; [M, K, T, w])
    vmap of sum(lax.scan(cost(mjx.step)))        ->  Physics.cost_rollouts(ctrl, cost)    (either of the two with the running cost
                                                                                           of a weighted tracking cost formed on
                                                                                           the device: [M, K], no trajectory read)
    mjx_env.get_sensor_data(model, data, name)  ->  Physics.sensor(name)                 (site sensors, Physics.set_sensors)
    data.replace(xfrc_applied=..., qfrc_applied=...) ->  Physics.set_applied(xfrc, qfrc)  (held by every later step / forward /
                                                                                           rollout, like a Data field)
    mj_fullM / data.qfrc_bias / mj_jacSite       ->  Physics.dynamics()                   (qM, qfrc_bias, qfrc_passive,
                                                                                           qfrc_actuator, jacp, jacr at the
                                                                                           record's current state)
    data.efc_force / qfrc_constraint / mj_contactForce ->  Physics.constraint_forces()    (one mjx.forward at the record's current
                                                                                           state; Physics.contact_forces())
    mjd_transitionFD / jax.jacobian(mjx.step)    ->  Physics.transition_fd()              (finite differences of step at a given
                                                                                           eps: fd_A, fd_B, fd_C, fd_D)
    mjd_transitionFD along a nominal rollout     ->  Physics.trajectory_fd(ctrl [M, T, nu]) (A_t, B_t, C_t, D_t at every control
                                                                                           step of the trajectory ctrl gives from
                                                                                           the current state; the record stays)
    the Riccati recursion of iLQR / TV-LQR      ->  Physics.lqr_backward(columns, lx, lu, lxx, luu)
                                                                                          (A_t, B_t and a quadratic cost model in,
                                                                                           the gains of feedback_rollouts out; one
                                                                                           launch, nothing of the env is read)
    control-limited DDP's backward pass          ->  Physics.lqr_backward_box(columns, lx, lu, lxx, luu, lo, hi)
                                                                                          (the same with lo <= k_t <= hi, e.g.
                                                                                           Physics.ctrl_bounds(u_nom): what agrees
                                                                                           with feedback_rollouts(clamp=True))
    jax.grad / Gauss-Newton hessian of the cost  ->  Physics.cost_expand(cost, dx, ctrl, sensordata, columns)
                                                                                          (the cost dict of cost_rollouts about a
                                                                                           nominal run in, lx, lu, lxx, luu, lux of
                                                                                           lqr_backward out; one launch, nothing of
                                                                                           the env is read;
                                                                                           Physics.differentiate_state forms dx)
    a Kalman filter / RTS smoother over a log   ->  Physics.kalman_smooth(columns, dy, r, q, P0)
                                                                                          (A_t, C_t of trajectory_fd and measured
                                                                                           minus nominal sensordata in, filtered and
                                                                                           smoothed state deviations out; one launch,
                                                                                           nothing of the env is read;
                                                                                           Physics.integrate_state adopts them)
    an IK library on top of mj_jacSite          ->  Physics.ik(sites, target_pos, target_quat=None)
                                                                                          (which qpos puts these sites there:
                                                                                           damped least squares, M problems in one
                                                                                           launch; the record stays)
    mj_inverse / mjx.inverse (data.qfrc_inverse)  ->  Physics.inverse(qacc)               (the force behind a given acceleration,
                                                                                           no solve: qfrc_inverse)

`Physics(env)` shares the batch of a BatchedEnv (Airbot cube / sf / T-shape, Go2 joystick, handstand / footstand): the same model,
the same per-env domain randomisation, the same record and the same stream.  The pipeline fields it exposes are the record's own
views, so a following `env.step` continues from whatever state these calls leave (rsr_physics_step / rsr_physics_forward,
include/rsr_physics.h).  As in MJX's Data, the position-dependent outputs (xpos, xquat, site_xpos, contacts) after a step are those
of the last forward pass, before the final integration.  The applied forces are per-env state of the Physics handle: env.step
ignores them (the Go2 joystick's kick keeps its own path inside the env kernel).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Sequence

from . import _lib
from . import sensors as _sensors

ROLLOUT_FIELDS = ("qpos", "qvel", "time", "actuator_force", "ncon", "sensordata")


class _DevArray:
    """__cuda_array_interface__ of a strided float32 region of library-owned device memory (the physics side buffer)."""

    def __init__(self, ptr: int, shape, strides_elems):
        self.__cuda_array_interface__ = dict(shape=tuple(int(s) for s in shape), typestr="<f4", data=(int(ptr), False), version=2,
                                             strides=tuple(4 * int(s) for s in strides_elems))


def _eps(who: str, eps) -> float:
    """a finite-difference step as a float, finite and > 0"""
    import math
    eps = float(eps)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError(f"{who}: eps must be finite and > 0, got {eps}")
    return eps


def _view(ptr, shape, stride, device):
    import torch
    if shape[1] == 0:                              # (sensordata while no sensors are set)
        return torch.empty((shape[0], 0), dtype=torch.float32, device=device)
    return torch.as_tensor(_DevArray(ptr.value, (shape[0], shape[1]), (stride[0], stride[1])), device=device)


class Physics:
    """Physics-only stepping, forward, rollouts and state setting on the envs of `env` (a BatchedEnv).  `sensors`: a sensor spec
    (see set_sensors), e.g. the env definition's `sensors`; None: no sensor stage."""

    def __init__(self, env, sensors: Optional[Sequence[tuple]] = None):
        import torch
        self.env = env
        self.num_envs = env.num_envs
        self.dims = env.dims
        self.device = env.device
        v = env._views
        d = self.dims
        # record views (shared with the env's State)
        self.qpos, self.qvel, self.ctrl, self.qacc_warmstart = v["qpos"], v["qvel"], v["ctrl"], v["qacc_warmstart"]
        self.time = v["time"][:, 0]
        self.xpos = v["xpos"].unflatten(1, (d.nbody, 3))
        self.site_xpos = v["site_xpos"].unflatten(1, (d.nsite, 3))
        # the physics handle owns the side buffer of the physics outputs
        self._h = C.c_void_p()
        _lib.check(_lib.lib().rsr_physics_create(env._batch, C.byref(self._h)))
        side = self._side = {name: self._fetch("rsr_physics_view", fid) for fid, name in enumerate(_lib.PHYS_FIELDS)}
        self.qacc = side["qacc"]
        self.actuator_force = side["actuator_force"]
        self.xquat = side["xquat"].unflatten(1, (d.nbody, 4))
        self._sensor_adr: Dict[str, tuple] = {}
        self.sensordata = side["sensordata"]
        # data.xfrc_applied [N, nbody, 6] / data.qfrc_applied [N, nv]: writable views while applied forces are on, else None
        self.xfrc_applied = None
        self.qfrc_applied = None
        # the dynamics buffer's views (dynamics): fetched on first use, when the library allocates the buffer
        self._dyn: Optional[Dict[str, Any]] = None
        # the constraint buffer's views (constraint_forces): likewise
        self._con: Optional[Dict[str, Any]] = None
        # the transition buffer's and the states buffer's views (transition_fd): likewise
        self._fd: Dict[str, Any] = {}
        # the inverse buffer's views (inverse): likewise
        self._inv: Optional[Dict[str, Any]] = None
        # {method name: the tensors its last launch reads, the int32 env ids included}.  The launches are asynchronous, so an entry
        # is written ahead of the C call and replaced by that method's next launch only: another method's launch may follow at
        # once, and must not drop what the one in flight still reads.
        self._held: Dict[str, tuple] = {}
        if sensors is not None:
            self.set_sensors(sensors)

    def _fetch(self, view_fn: str, fid: int):
        """field `fid` of one of the library's *_view entry points, as a tensor on the handle's memory"""
        ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
        _lib.check(getattr(_lib.lib(), view_fn)(self._h, fid, C.byref(ptr), shape, stride))
        return _view(ptr, shape, stride, self.device)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                import torch
                torch.cuda.synchronize(self.device)       # launches that write the side buffer may still be in flight
                _lib.lib().rsr_physics_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def n_substeps(self) -> int:
        return int(self.dims.n_frames)

    @property
    def ncon_max(self) -> int:
        return int(self.dims.ncon_max)

    def _stream(self):
        return self.env._stream()

    def _accel_site(self) -> Optional[int]:
        """the site whose body's acceleration the kernels track (env_ids[0] of the Go2 family: the IMU), or None"""
        from .envs import config as cfg
        if int(self.dims.env_kind) in (cfg.ENV_GO2, cfg.ENV_GO2_HANDSTAND):
            return self.env.sys.id("site", "imu")
        return None

    def set_sensors(self, spec: Optional[Sequence[tuple]]) -> None:
        """Sets the sensor table: `spec` is a list of (name, type, site, ref_site=None), sites by name, types of
        _lib.SENSOR_TYPES (None or []: no sensors).  From then on step / forward / set_state also fill `sensordata`
        [N, nsensordata] (MuJoCo's sensordata layout, sensors in spec order), and rollout can record it."""
        import torch
        spec = list(spec or [])
        table, where = _sensors.sensor_table(self.env.sys, spec, self._accel_site())
        _lib.check(_lib.lib().rsr_physics_set_sensors(self._h, table.ctypes.data_as(C.c_void_p) if len(table) else None, len(table)))
        self._sensor_adr = where
        self.sensordata = self._side["sensordata"] = self._fetch("rsr_physics_view", _lib.PHYS_FIELDS.index("sensordata"))

    @property
    def nsensordata(self) -> int:
        return int(self.sensordata.shape[1])

    def sensor(self, name: str, data=None):
        """The columns of sensor `name` in `data` (default: the current sensordata [N, nsensordata]; a rollout's
        sensordata [N, T, nsensordata] works too): mjx_env.get_sensor_data."""
        if name not in self._sensor_adr:
            raise KeyError(f"no sensor {name!r}; set: {list(self._sensor_adr)}")
        adr, w = self._sensor_adr[name]
        data = self.sensordata if data is None else data
        return data[..., adr:adr + w]

    def _ids(self, env_ids, who: str, repeats: bool = False):
        """env_ids as an int64 tensor on the device (None: every env), checked: in range, no repeats (unless `repeats`)."""
        import torch
        if env_ids is None:
            return torch.arange(self.num_envs, device=self.device, dtype=torch.int64)
        ids = torch.as_tensor(env_ids, device=self.device).to(torch.int64).reshape(-1)
        if ids.numel() and bool(((ids < 0) | (ids >= self.num_envs)).any()):
            raise ValueError(f"{who}: env_ids must lie in [0, {self.num_envs})")
        if not repeats and torch.unique(ids).numel() != ids.numel():
            raise ValueError(f"{who}: env_ids must not repeat")
        return ids

    def _env_list(self, who: str, env_ids, checked: bool = False):
        """env_ids as the library's entry points take a list: (pointer, count, the int32 tensor behind the pointer).  None is every
        env: (null, 0, None).  An empty list gives None, and the caller makes no call.  checked: env_ids already went through _ids."""
        import torch
        if env_ids is None:
            return None, 0, None
        ids = env_ids if checked else self._ids(env_ids, who)
        k = ids.numel()
        if k == 0:
            return None
        ids32 = ids.to(torch.int32).contiguous()
        return C.c_void_p(ids32.data_ptr()), k, ids32

    def _call_envs(self, fn: str, who: str, env_ids, *args, checked: bool = False, hold: tuple = ()) -> None:
        """The library's env-list entry point `fn`(handle, ids, count, *args, stream) for the method `who`: env_ids None runs every
        env, an empty list nothing.  `hold`: the tensors `args` point into; with the ids they are `who`'s held inputs."""
        lst = self._env_list(who, env_ids, checked)
        if lst is None:
            return
        ptr, k, ids32 = lst
        self._held[who] = (*hold, ids32)
        _lib.check(getattr(_lib.lib(), fn)(self._h, ptr, k, *args, self._stream()))

    def _steps(self, who: str, nsteps, below_2_30: bool = False) -> int:
        """nsteps (None: n_substeps) as an int >= 1"""
        nsteps = self.n_substeps if nsteps is None else int(nsteps)
        if below_2_30 and not 1 <= nsteps < 2 ** 30:
            raise ValueError(f"{who}: nsteps must lie in [1, 2^30), got {nsteps}")
        if nsteps < 1:
            raise ValueError(f"{who}: nsteps must be >= 1, got {nsteps}")
        return nsteps

    def _f32(self, what: str, t, shape_txt: str, ok, contiguous: bool, got: bool = False) -> None:
        """Refuses `t` unless it is a float32 tensor on the env's device that `ok` takes (a shape, or a predicate of the tensor)
        and, if asked, contiguous.  what: how the message opens ("<method> expects <name> as"); got: it ends with what `t` is."""
        import torch
        dev = self.qvel.device
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev or not (ok(t) if callable(ok) else tuple(t.shape) == ok) \
                or (contiguous and not t.is_contiguous()):
            is_ = "" if not got else f", got {tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else f", got {type(t).__name__}"
            raise ValueError(f"{what} a {'contiguous ' if contiguous else ''}float32 tensor of shape {shape_txt} on {dev}{is_}")

    def _site_ids(self, who: str, sites) -> list:
        """site names or ids as ids, checked"""
        ids = []
        for s_ in sites:
            if isinstance(s_, str):
                try:
                    sid = int(self.env.sys.id("site", s_))
                except Exception:
                    raise ValueError(f"{who}: no site {s_!r}") from None
            else:
                sid = int(s_)
            if not 0 <= sid < self.dims.nsite:
                raise ValueError(f"{who}: site ids must lie in [0, {self.dims.nsite}), got {sid}")
            ids.append(sid)
        return ids

    def _outputs(self, who: str, shapes: Dict[str, Any], out, strict: bool, note: str = "") -> Dict[str, Any]:
        """{name: tensor} for `shapes` {name: shape, or (shape, dtype) where it is not float32}, on the env's device: out[name] where
        the caller gave one (refused unless it is a contiguous tensor of that shape, dtype and device), else a new one.  strict: a
        key of `out` that `shapes` does not have is refused (`note` ends that message), else ignored."""
        import torch
        dev = self.qvel.device
        out = out or {}
        if strict and not out.keys() <= shapes.keys():
            raise ValueError(f"{who}: out has {sorted(set(out) - set(shapes))}; it may hold {tuple(shapes)}{note}")
        res = {}
        for f, shape in shapes.items():
            dt = torch.float32
            if type(shape[-1]) is torch.dtype:
                shape, dt = shape
            t = out.get(f)
            if t is None:
                t = torch.empty(shape, dtype=dt, device=dev)
            elif not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{who}: out[{f!r}] must be a contiguous {str(dt).split('.')[-1]} tensor of shape {shape} on {dev}")
            res[f] = t
        return res

    def set_applied(self, xfrc=None, qfrc=None, env_ids=None) -> None:
        """data.replace(xfrc_applied=..., qfrc_applied=...): turns applied forces on (zero everywhere the first time) and writes
        the given rows of the envs `env_ids` (default: all; rows in env_ids order).  xfrc: [k, nbody, 6], per body force[3] and
        torque[3] in the world frame, acting at the body's centre of mass (row 0, the world, is ignored); qfrc: [k, nv].  None
        leaves a field as it is.  The values persist: every later step (each substep), forward, set_state of other envs and
        rollout (all T control steps) applies them."""
        import torch
        ids = self._ids(env_ids, "set_applied")
        k, d = ids.numel(), self.dims
        vals = {}
        for name, x, shape in (("xfrc", xfrc, (k, d.nbody, 6)), ("qfrc", qfrc, (k, d.nv))):
            if x is None:
                continue
            t = torch.as_tensor(x, dtype=torch.float32, device=self.device)
            if tuple(t.shape) != shape:
                raise ValueError(f"set_applied expects {name} of shape {shape}, got {tuple(t.shape)}")
            vals[name] = t
        if self.xfrc_applied is None:
            _lib.check(_lib.lib().rsr_physics_set_applied(self._h, 1))
            views = [self._fetch("rsr_physics_applied_view", fid) for fid in range(len(_lib.APPLIED_FIELDS))]
            self.xfrc_applied = views[0].unflatten(1, (d.nbody, 6))
            self.qfrc_applied = views[1]
        if k == 0:
            return
        if "xfrc" in vals:
            self.xfrc_applied[ids] = vals["xfrc"]
        if "qfrc" in vals:
            self.qfrc_applied[ids] = vals["qfrc"]

    def clear_applied(self) -> None:
        """Turns applied forces off: every later call runs without them (xfrc_applied / qfrc_applied become None)."""
        if self.xfrc_applied is None:
            return
        self.xfrc_applied = self.qfrc_applied = None
        _lib.check(_lib.lib().rsr_physics_set_applied(self._h, 0))

    def _dyn_views(self) -> Dict[str, Any]:
        if self._dyn is None:
            import torch
            d = self.dims
            dyn = {name: self._fetch("rsr_physics_dynamics_view", fid) for fid, name in enumerate(_lib.DYNAMICS_FIELDS)}
            k = dyn["jac_site_xpos"].shape[1] // 3
            jac = dyn["jac"].unflatten(1, (k, 6, d.nv)) if k else torch.empty((self.num_envs, 0, 6, d.nv), dtype=torch.float32, device=self.device)
            self._dyn = dict(qM=dyn["qM"].unflatten(1, (d.nv, d.nv)), qfrc_bias=dyn["qfrc_bias"], qfrc_passive=dyn["qfrc_passive"],
                             qfrc_actuator=dyn["qfrc_actuator"], jacp=jac[:, :, 0:3], jacr=jac[:, :, 3:6],
                             jac_site_xpos=dyn["jac_site_xpos"].unflatten(1, (k, 3)) if k else torch.empty((self.num_envs, 0, 3), dtype=torch.float32, device=self.device))
        return self._dyn

    # outputs of dynamics(): views of the handle's dynamics buffer, zeros until the first call
    qM = property(lambda self: self._dyn_views()["qM"], doc="[N, nv, nv] joint-space inertia, dense, armature included (mj_fullM)")
    qfrc_bias = property(lambda self: self._dyn_views()["qfrc_bias"], doc="[N, nv] Coriolis, centrifugal and gravity forces")
    qfrc_passive = property(lambda self: self._dyn_views()["qfrc_passive"], doc="[N, nv] -damping * qvel")
    qfrc_actuator = property(lambda self: self._dyn_views()["qfrc_actuator"], doc="[N, nv] gear * actuator_force, actfrcrange clamp included")
    jacp = property(lambda self: self._dyn_views()["jacp"], doc="[N, K, 3, nv] translational Jacobians of the sites of set_jac_sites")
    jacr = property(lambda self: self._dyn_views()["jacr"], doc="[N, K, 3, nv] rotational Jacobians of the sites of set_jac_sites")
    jac_site_xpos = property(lambda self: self._dyn_views()["jac_site_xpos"], doc="[N, K, 3] where those Jacobians were taken")

    def set_jac_sites(self, sites: Optional[Sequence]) -> None:
        """The sites whose Jacobians dynamics() evaluates (mj_jacSite): names or ids, at most _lib.MAX_JAC_SITES; None or []
        clears the table (jacp / jacr get K = 0).  Earlier jacp / jacr / jac_site_xpos views keep their old K: read them again."""
        import numpy as np
        ids = self._site_ids("set_jac_sites", list(sites or []))
        if len(ids) > _lib.MAX_JAC_SITES:
            raise ValueError(f"set_jac_sites expects at most {_lib.MAX_JAC_SITES} sites, got {len(ids)}")
        table = np.asarray(ids, dtype=np.int32)
        _lib.check(_lib.lib().rsr_physics_set_jac_sites(self._h, table.ctypes.data_as(C.c_void_p) if len(ids) else None, len(ids)))
        self._dyn = None

    def dynamics(self, env_ids=None) -> None:
        """The model at the record's current qpos / qvel / ctrl (per-env leaves included), one launch: fills qM, qfrc_bias,
        qfrc_passive, qfrc_actuator and, for the sites of set_jac_sites, jacp / jacr / jac_site_xpos, of the envs `env_ids`
        (default: all).  Meant to be called after step / set_state, before choosing the next ctrl or qfrc_applied: it describes
        the state after the integration, whereas qacc, xquat and the contacts show the step's last forward pass.  Writes nothing
        else (not the record, the side buffer or sensordata).  Applied forces enter none of the outputs:
        qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator (+ the applied forces the caller set)."""
        self._call_envs("rsr_physics_dynamics", "dynamics", env_ids)

    def _con_views(self) -> Dict[str, Any]:
        if self._con is None:
            self._con = {name: self._fetch("rsr_physics_constraint_view", fid) for fid, name in enumerate(_lib.CONSTRAINT_FIELDS)}
        return self._con

    # outputs of constraint_forces(): views of the handle's constraint buffer, zeros until the first call
    qfrc_constraint = property(lambda self: self._con_views()["qfrc_constraint"], doc="[N, nv] J^T efc_force at the solver's final qacc")
    efc_force = property(lambda self: self._con_views()["efc_force"],
                         doc="[N, nefc_max] row forces: equality, dof friction, active limits, contacts x pyramid edges; rows >= nefc are 0")
    efc_counts = property(lambda self: self._con_views()["efc_counts"], doc="[N, 4] nefc, ne, nf, nl (active limits), as float")
    constraint_qacc = property(lambda self: self._con_views()["qacc"], doc="[N, nv] qacc of the pass constraint_forces() ran")

    def constraint_forces(self, env_ids=None) -> None:
        """One mjx.forward pass at the record's current qpos / qvel / ctrl / qacc_warmstart (per-env leaves and, when on, the
        applied forces included), one launch: fills qfrc_constraint, efc_force, efc_counts, constraint_qacc and the contacts of
        contact_forces() of the envs `env_ids` (default: all).  Like dynamics() it describes the state after the last
        integration and writes nothing else: not the record (qacc_warmstart stays), the side buffer, sensordata or the dynamics
        buffer.  Its qacc and contacts are bit for bit those forward() would give on the same record, and
        qM @ constraint_qacc = qfrc_passive - qfrc_bias + qfrc_actuator (+ applied forces) + qfrc_constraint to the solver's
        convergence."""
        self._call_envs("rsr_physics_constraint", "constraint_forces", env_ids)

    def contact_forces(self) -> Dict[str, Any]:
        """The contacts of the last constraint_forces() with their forces (mj_contactForce, in the world frame), per env and
        contact slot as contacts(): ncon [N] (int), dist [N, K], pos [N, K, 3], normal [N, K, 3] (views), geom1 / geom2 [N, K]
        (int), and normal_force [N, K] (>= 0), force [N, K, 3], torque [N, K, 3] (views): the force and the torsional moment
        about the normal that act on geom2's body at `pos`; geom1's body gets the negative.  Slots >= ncon are zeros."""
        import torch
        v = self._con_views()
        c = v["contact"].unflatten(1, (self.ncon_max, 9))
        w = v["contact_wrench"].unflatten(1, (self.ncon_max, 7))
        return dict(ncon=v["ncon"][:, 0].to(torch.int32), dist=c[:, :, 0], pos=c[:, :, 1:4], normal=c[:, :, 4:7],
                    geom1=c[:, :, 7].to(torch.int32), geom2=c[:, :, 8].to(torch.int32),
                    normal_force=w[:, :, 0], force=w[:, :, 1:4], torque=w[:, :, 4:7])

    def _fd_view(self, name: str):
        """[N, ncol, row] view of the transition buffer ("columns") or of one half of the states buffer, fetched on first use"""
        if name not in self._fd:
            d = self.dims
            ncol = 2 * d.nv + d.nu
            self._fd[name] = self._fetch("rsr_physics_transition_view", _lib.TRANSITION_FIELDS.index(name)).unflatten(1, (ncol, -1))
        return self._fd[name]

    def _fd_block(self, rows: str, cols: str):
        """A block of [A B; C D]: the buffer holds one row per column of the matrix, so the block is a transposed view"""
        d, nsd = self.dims, self.nsensordata
        r = slice(0, 2 * d.nv) if rows == "x" else slice(2 * d.nv, 2 * d.nv + nsd)
        c = slice(0, 2 * d.nv) if cols == "x" else slice(2 * d.nv, 2 * d.nv + d.nu)
        return self._fd_view("columns")[:, c, r].transpose(1, 2)

    # outputs of transition_fd(): views of the handle's transition buffer, zeros until the first call.  Rows and columns of x are
    # the tangent space of (qpos, qvel): nv + nv.  fd_C / fd_D follow the sensor table of the moment they are read.
    fd_A = property(lambda self: self._fd_block("x", "x"), doc="[N, 2nv, 2nv] d next (qpos, qvel) / d (qpos, qvel)")
    fd_B = property(lambda self: self._fd_block("x", "u"), doc="[N, 2nv, nu] d next (qpos, qvel) / d ctrl")
    fd_C = property(lambda self: self._fd_block("s", "x"), doc="[N, nsensordata, 2nv] d sensordata / d (qpos, qvel)")
    fd_D = property(lambda self: self._fd_block("s", "u"), doc="[N, nsensordata, nu] d sensordata / d ctrl")
    fd_x = property(lambda self: self._fd_view("states_x").unflatten(2, (2, -1)),
                    doc="[N, ncol, 2, nq+nv+nu] keep_states: the perturbed qpos, qvel, ctrl of each column's two runs")
    fd_y = property(lambda self: self._fd_view("states_y").unflatten(2, (2, -1)),
                    doc="[N, ncol, 2, nq+nv] keep_states: the end state qpos, qvel of each column's two runs")

    def transition_fd(self, env_ids=None, nsteps: Optional[int] = None, eps: float = 1e-3, centered: bool = True,
                      keep_states: bool = False) -> None:
        """mjd_transitionFD: finite differences of step(ctrl, nsteps) (default n_substeps) about the record's current qpos / qvel /
        ctrl, one launch with one wave per (env, column): fills fd_A, fd_B and, with a sensor table, fd_C, fd_D of the envs
        `env_ids` (default: all).  Column k < nv moves qpos in its tangent space (mj_integratePos: a free joint's rotation
        multiplies its quaternion on the right), the next nv move qvel, the last nu move ctrl, each by +-eps (centered) or by +eps
        against the unperturbed step; ctrl is moved wherever it stands, its range is not consulted (MuJoCo nudges it).  Each run
        starts from the record's qacc_warmstart and is bit for bit the step it stands for, per-env leaves and applied forces
        included.  Rows of qpos are mj_differentiatePos of the two end states.  These are differences at `eps`, not derivatives:
        friction loss, limits and contacts make the step piecewise smooth, and the result depends on eps.  keep_states also
        records the runs' inputs and end states (fd_x, fd_y).  Writes nothing else: not the record, the side buffer, sensordata,
        the dynamics or the constraint buffer."""
        nsteps, eps = self._steps("transition_fd", nsteps), _eps("transition_fd", eps)
        flags = (_lib.FD_CENTERED if centered else 0) | (_lib.FD_STATES if keep_states else 0)
        self._call_envs("rsr_physics_transition_fd", "transition_fd", env_ids, nsteps, eps, flags)

    def _inv_views(self) -> Dict[str, Any]:
        if self._inv is None:
            self._inv = {name: self._fetch("rsr_physics_inverse_view", fid) for fid, name in enumerate(_lib.INVERSE_FIELDS)}
        return self._inv

    # outputs of inverse(): views of the handle's inverse buffer, zeros until the first call
    qfrc_inverse = property(lambda self: self._inv_views()["qfrc_inverse"],
                            doc="[N, nv] M a + qfrc_bias - qfrc_passive - qfrc_constraint: every external force, actuators included")
    inverse_qacc = property(lambda self: self._inv_views()["qacc"], doc="[N, nv] the continuous-time acceleration a that inverse() used")
    inverse_qfrc_constraint = property(lambda self: self._inv_views()["qfrc_constraint"], doc="[N, nv] J^T inverse_efc_force")
    inverse_qfrc_actuator = property(lambda self: self._inv_views()["qfrc_actuator"], doc="[N, nv] as qfrc_actuator of dynamics()")
    inverse_efc_force = property(lambda self: self._inv_views()["efc_force"],
                                 doc="[N, nefc_max] row forces at a, rows as efc_force; rows >= nefc are 0")
    inverse_efc_counts = property(lambda self: self._inv_views()["efc_counts"], doc="[N, 4] nefc, ne, nf, nl (active limits), as float")

    def inverse(self, qacc, env_ids=None, discrete: bool = False) -> None:
        """mj_inverse / mjx.inverse at the record's current qpos / qvel / ctrl (per-env leaves included) and the accelerations
        `qacc`, a contiguous float32 tensor [num_envs, nv] on the env's device (row e is env e's, with env_ids too), one launch:
        fills qfrc_inverse, inverse_qacc, inverse_qfrc_constraint, inverse_qfrc_actuator, inverse_efc_force and
        inverse_efc_counts of the envs `env_ids` (default: all).  The pass builds the constraint rows as forward() does and
        evaluates their forces at `qacc`; no solve runs.  qfrc_inverse is the total of everything external, actuators included:
        qfrc_inverse - inverse_qfrc_actuator is what the model does not explain.  discrete: `qacc` is
        (qvel_after - qvel_before) / timestep of one substep, and the integrator's implicit damping is undone first
        (mj_discreteAcc); inverse_qacc shows the result.  The constraints are soft and stiff: an error in `qacc` is multiplied
        by the row stiffness on every active contact or limit row, so differenced fp32 velocities give noisy forces there.
        Like dynamics() it describes the state after the last integration and writes nothing else; applied forces enter none of
        the outputs."""
        shape = (self.num_envs, self.dims.nv)
        self._f32("inverse expects qacc as", qacc, shape, shape, True)
        lst = self._env_list("inverse", env_ids)
        if lst is None:
            return
        ptr, k, ids32 = lst
        self._held["inverse"] = (qacc, ids32)
        _lib.check(_lib.lib().rsr_physics_inverse(self._h, C.c_void_p(qacc.data_ptr()), ptr, k, _lib.INV_DISCRETE if discrete else 0,
                                                  self._stream()))

    def rollout(self, ctrl, nsteps: Optional[int] = None, fields: Sequence[str] = ("qpos", "qvel", "time"), qpos0=None, qvel0=None,
                ctrl0=None, out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """T control steps in one launch: for t < T, ctrl[:, t] then `nsteps` (default n_substeps) x mjx.step.  ctrl is
        [num_envs, T, nu].  With qpos0 / qvel0 / ctrl0, set_state runs first (mjx_env.init).  Returns {field: [N, T, w]} for
        `fields` (ROLLOUT_FIELDS): qpos, qvel, time after each control step; actuator_force, ncon, sensordata of its last forward
        pass.  `out`: caller-owned float32 tensors to fill instead of new ones.  Afterwards the record and the side buffer hold
        what T calls of step would leave."""
        import torch
        nsteps = self._steps("rollout", nsteps)
        c = torch.as_tensor(ctrl, dtype=torch.float32, device=self.device)
        if c.dim() != 3 or c.shape[0] != self.num_envs or c.shape[2] != self.dims.nu or c.shape[1] < 1:
            raise ValueError(f"rollout expects ctrl of shape ({self.num_envs}, T >= 1, {self.dims.nu}), got {tuple(c.shape)}")
        T = int(c.shape[1])
        res, ptrs = self._trajectory_out("rollout", fields, (self.num_envs, T), out, none_ok=True)
        if qpos0 is not None or qvel0 is not None or ctrl0 is not None:
            self.set_state(qpos0, qvel0, ctrl0)
        c = c.contiguous()
        self._held["rollout"] = (c,)
        _lib.check(_lib.lib().rsr_physics_rollout(self._h, C.c_void_p(c.data_ptr()), T, nsteps, C.byref(ptrs), self._stream()))
        return res

    def sample_rollouts(self, ctrl, nsteps: Optional[int] = None, fields: Sequence[str] = ("qpos", "qvel", "time"), env_ids=None,
                        out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """What a sampling planner asks (predictive sampling, MPPI, CEM): from the state each env is in now, K control sequences
        of T control steps, one launch with one wave per (env, sample).  ctrl is a float32 tensor [M, K, T, nu] on the env's
        device, M = len(env_ids) (default: every env, M = num_envs); sample (s, k) starts from the record of env env_ids[s] as it
        stands (qpos, qvel, qacc_warmstart, time), with that env's per-env leaves and applied forces, and runs ctrl[s, k, t] then
        `nsteps` (default n_substeps) x mjx.step for t < T: bit for bit the trajectory rollout() records on a batch whose env
        holds that record row and those leaves.  Returns {field: [M, K, T, w]} for `fields` (ROLLOUT_FIELDS, as rollout), rows in
        env_ids order.  `out`: caller-owned float32 tensors to fill instead of new ones.  Writes nothing else: the record, the
        side buffer, sensordata and every other buffer of the handle stay as they are, so step() goes on from where the batch
        stood.  A field takes 4 * M * K * T * w bytes: asking for fewer fields is the only lever (a cost on sensor values needs
        fields=("sensordata",) alone)."""
        who = "sample_rollouts"
        nsteps = self._steps(who, nsteps)
        ids = None if env_ids is None else self._ids(env_ids, who)
        M, nu = self.num_envs if ids is None else int(ids.numel()), self.dims.nu
        self._f32(f"{who} expects ctrl as", ctrl, f"({M}, K >= 1, T >= 1, {nu})",
                  lambda t: t.dim() == 4 and t.shape[0] == M and t.shape[3] == nu and t.shape[1] >= 1 and t.shape[2] >= 1, False)
        K, T = int(ctrl.shape[1]), int(ctrl.shape[2])
        res, ptrs = self._trajectory_out(who, fields, (M, K, T), out)
        c = ctrl.contiguous()
        self._call_envs("rsr_physics_sample_rollouts", who, ids, C.c_void_p(c.data_ptr()), K, T, nsteps, C.byref(ptrs), checked=True, hold=(c,))
        return res

    def _leaf_shapes(self) -> Dict[str, tuple]:
        """per-env shape of each leaf of _lib.DR_FIELDS (BatchedEnv.set_randomization)"""
        d = self.dims
        return dict(geom_friction=(d.ngeom, 3), body_mass=(d.nbody,), dof_damping=(d.nv,), dof_frictionloss=(d.nv,),
                    body_ipos=(d.nbody, 3), qpos0=(d.nq,), dof_armature=(d.nv,), actuator_gainprm=(d.nu, 3), actuator_biasprm=(d.nu, 3))

    def _sampled_leaves(self, who: str, params, M: int, K: Optional[int]):
        """(_lib.ParamSamples, the tensors it points to, K) of `params` {leaf name: [M, K, ...]}, checked for the method `who`; K:
        what the caller's other inputs say, or None"""
        from .envs import config as cfg
        params = dict(params or {})
        unknown = sorted(set(params) - set(_lib.DR_FIELDS))
        if unknown:
            raise ValueError(f"{who}: not a model leaf: {unknown}; leaves: {_lib.DR_FIELDS}")
        shapes = self._leaf_shapes()
        ps, leaves = _lib.ParamSamples(), []
        for fid, name in enumerate(_lib.DR_FIELDS):
            t = params.get(name)
            if t is None:
                continue
            if fid >= _lib.DR_FIELDS.index("body_ipos") and int(self.dims.env_kind) not in (cfg.ENV_GO2, cfg.ENV_GO2_HANDSTAND):
                raise ValueError(f"{who}: {name} is a per-sample leaf on the Go2 models only")
            tail = tuple(int(w) for w in shapes[name])
            self._f32(f"{who}: params[{name!r}] must be", t, f"({M}, K >= 1, {', '.join(map(str, tail))})",
                      lambda t: t.dim() == 2 + len(tail) and t.shape[0] == M and t.shape[1] >= 1 and tuple(t.shape[2:]) == tail, True)
            if K is not None and int(t.shape[1]) != K:
                raise ValueError(f"{who}: params[{name!r}] has K = {int(t.shape[1])}, the others (or ctrl) K = {K}")
            K = int(t.shape[1])
            ps.leaf[fid] = t.data_ptr()
            leaves.append(t)
        return ps, leaves, K

    def _trajectory_out(self, who: str, fields, lead: tuple, out, extra: Optional[Dict[str, int]] = None, none_ok: bool = False):
        """({field: tensor lead + (w,)}, _lib.RolloutOut) for `fields` of ROLLOUT_FIELDS (and of `extra` {name: width}, which
        RolloutOut does not hold), checked for the method `who`; `out`: caller-owned tensors to use instead of new ones (its other
        keys are ignored); none_ok: no field at all is a request too"""
        extra = extra or {}
        fields = tuple(fields)
        bad = [f for f in fields if f not in ROLLOUT_FIELDS and f not in extra]
        if bad or not (fields or none_ok):
            raise ValueError(f"{who}: unknown{'' if none_ok else ' or no'} fields {bad}; recordable: {ROLLOUT_FIELDS + tuple(extra)}")
        if "sensordata" in fields and self.nsensordata == 0:
            raise ValueError(f"{who}: sensordata requested but no sensors are set (set_sensors)")
        d = self.dims
        width = dict(qpos=d.nq, qvel=d.nv, time=1, actuator_force=d.nu, ncon=1, sensordata=self.nsensordata, **extra)
        res, ptrs = self._outputs(who, {f: tuple(lead) + (width[f],) for f in fields}, out, False), _lib.RolloutOut()
        for f, t in res.items():
            if f not in extra:
                setattr(ptrs, f, t.data_ptr())
        return res, ptrs

    def _rows(self, who: str, name: str, t, M: int, tail: tuple, ranks: tuple):
        """(K or None, T) of the input `name` of the method `who`, a [M, (K,) T, *tail] tensor of one of the ranks `ranks`, checked"""
        self._f32(f"{who} expects {name} as", t, f"({M}, T >= 1, {', '.join(map(str, tail))}) or ({M}, K >= 1, T >= 1, {', '.join(map(str, tail))})",
                  lambda t: t.dim() in ranks and t.shape[0] == M and tuple(t.shape[t.dim() - len(tail):]) == tail
                  and min(t.shape[1:t.dim() - len(tail)]) >= 1, False)
        per = t.dim() == len(tail) + 3
        return (int(t.shape[1]) if per else None), int(t.shape[-len(tail) - 1])

    def param_rollouts(self, ctrl, params, nsteps: Optional[int] = None, fields: Sequence[str] = ("qpos", "qvel", "time"), env_ids=None,
                       out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """What system identification, domain-randomised planning and CEM over model parameters ask: from the state each env is
        in now, K sets of model leaves, each run for T control steps, one launch with one wave per (env, sample) and no replica
        batch.  `params` is {leaf name: contiguous float32 tensor [M, K, ...] on the env's device}: the names and shapes of
        BatchedEnv.set_randomization with K after the env dim, e.g. geom_friction [M, K, ngeom, 3], body_mass [M, K, nbody],
        dof_damping [M, K, nv], actuator_gainprm [M, K, nu, 3] (the last five of _lib.DR_FIELDS on the Go2 models only); a leaf
        that is not given stays the env's own (its per-env value, or the model's).  M = len(env_ids) (default: every env).
        ctrl is a float32 tensor [M, T, nu], one sequence shared by an env's K samples (one logged control sequence), or
        [M, K, T, nu]; K comes from `params`, or from a 4-D ctrl when `params` is empty, and the two must agree.  Sample (s, k)
        starts from the record of env env_ids[s] as it stands (qpos, qvel, qacc_warmstart, time) with that env's applied forces:
        bit for bit the trajectory rollout() records on a batch whose env holds that record row and, through set_randomization,
        row (s, k) of every given leaf.  With no params and a 4-D ctrl this is sample_rollouts.  Returns {field: [M, K, T, w]} for
        `fields` (ROLLOUT_FIELDS, as rollout), rows in env_ids order.  `out`: caller-owned float32 tensors to fill instead of new
        ones.  Writes nothing else: the record, the side buffer, sensordata, every other buffer of the handle and the batch's own
        leaf tensors stay as they are.  A field takes 4 * M * K * T * w bytes: ask for what the loss reads."""
        who = "param_rollouts"
        nsteps = self._steps(who, nsteps)
        ids = None if env_ids is None else self._ids(env_ids, who)
        M, nu = self.num_envs if ids is None else int(ids.numel()), self.dims.nu
        self._f32(f"{who} expects ctrl as", ctrl, f"({M}, T >= 1, {nu}) or ({M}, K >= 1, T >= 1, {nu})",
                  lambda t: t.dim() in (3, 4) and t.shape[0] == M and t.shape[-1] == nu and min(t.shape[1:-1]) >= 1, False)
        per_sample = ctrl.dim() == 4
        T, K = int(ctrl.shape[-2]), int(ctrl.shape[1]) if per_sample else None
        ps, leaves, K = self._sampled_leaves(who, params, M, K)
        if K is None:
            raise ValueError(f"{who}: K is not given: pass sampled leaves in params, or a 4-D ctrl [M, K, T, nu]")
        res, ptrs = self._trajectory_out(who, fields, (M, K, T), out)
        c = ctrl.contiguous()
        self._call_envs("rsr_physics_param_rollouts", who, ids, C.c_void_p(c.data_ptr()), C.byref(ps), K, T, nsteps,
                        _lib.PR_CTRL_PER_SAMPLE if per_sample else 0, C.byref(ptrs), checked=True, hold=(c, *leaves))
        return res

    def feedback_rollouts(self, ctrl, gain, qpos_ref, qvel_ref, params=None, nsteps: Optional[int] = None,
                          fields: Sequence[str] = ("qpos", "qvel", "time"), env_ids=None, clamp: bool = False,
                          out: Optional[Dict[str, Any]] = None, K: Optional[int] = None) -> Dict[str, Any]:
        """What an iLQR / iLQG forward pass, MPPI with a feedback term and CEM over controller gains ask: param_rollouts in closed
        loop.  At the start of control step t each sample computes its control from its own current state (the record's at
        t = 0, the state after control step t - 1 otherwise),
            u = ctrl[.., t] + gain[.., t] @ [qpos (-) qpos_ref[.., t]; qvel - qvel_ref[.., t]],
        (-) in the tangent space of qpos (mj_differentiatePos: nv numbers, a free joint's rotation as a rotation vector, as
        transition_fd takes its differences), accumulated in fp32 from ctrl in index order, and holds it for the step's `nsteps`
        substeps; `clamp` then clips u to actuator_ctrlrange where the actuator is ctrl-limited.  All float32 tensors on the
        env's device, M = len(env_ids) (default: every env): ctrl [M, T, nu], or [M, K, T, nu] per sample (an iLQR line search
        folds alpha * k_t into it); gain [M, T, nu, 2 nv] with qpos_ref [M, T, nq] and qvel_ref [M, T, nv], shared by an env's K
        samples, or all three per sample, [M, K, T, ..] (candidate gain sets).  `params`: per-sample model leaves as
        param_rollouts takes them, or None.  K comes from whichever input is per-sample (they must agree); pass `K` when none is.
        Returns {field: [M, K, T, w]} for `fields`: ROLLOUT_FIELDS as param_rollouts, and "ctrl", the controls that were applied
        [M, K, T, nu] (fed to sample_rollouts they reproduce the trajectories bit for bit).  `out`: caller-owned float32 tensors
        to fill instead of new ones.  Writes nothing else: the record, every buffer of the handle and the batch's own leaf
        tensors stay as they are.  A field takes 4 * M * K * T * w bytes: ask for what the cost reads."""
        who = "feedback_rollouts"
        nsteps = self._steps(who, nsteps)
        ids = None if env_ids is None else self._ids(env_ids, who)
        d = self.dims
        M, nu, nv, nq = self.num_envs if ids is None else int(ids.numel()), int(d.nu), int(d.nv), int(d.nq)
        rows = lambda name, t, tail, ranks: self._rows(who, name, t, M, tail, ranks)
        Kc, T = rows("ctrl", ctrl, (nu,), (3, 4))
        Kg, Tg = rows("gain", gain, (nu, 2 * nv), (4, 5))
        fb_rank = gain.dim() - 1                         # the refs' rank: [M, T, w] or [M, K, T, w]
        Kq, Tq = rows("qpos_ref", qpos_ref, (nq,), (fb_rank,))
        Kv, Tv = rows("qvel_ref", qvel_ref, (nv,), (fb_rank,))
        if (Tg, Tq, Tv) != (T, T, T):
            raise ValueError(f"{who}: gain, qpos_ref and qvel_ref have T = {Tg}, {Tq}, {Tv}, ctrl T = {T}")
        for name, k in (("ctrl", Kc), ("gain", Kg), ("qpos_ref", Kq), ("qvel_ref", Kv)):
            if k is not None and K is not None and k != int(K):
                raise ValueError(f"{who}: {name} has K = {k}, the others (or the K given) K = {int(K)}")
            K = k if k is not None else K
        if K is not None and int(K) < 1:
            raise ValueError(f"{who}: K must be >= 1, got {K}")
        ps, leaves, K = self._sampled_leaves(who, params, M, None if K is None else int(K))
        if K is None:
            raise ValueError(f"{who}: K is not given: pass it, or a per-sample ctrl, gain or leaf")
        res, ptrs = self._trajectory_out(who, fields, (M, K, T), out, extra=dict(ctrl=nu))
        c, g, qr, vr = ctrl.contiguous(), gain.contiguous(), qpos_ref.contiguous(), qvel_ref.contiguous()
        fb = _lib.Feedback(g.data_ptr(), qr.data_ptr(), vr.data_ptr())
        flags = (_lib.FB_CTRL_PER_SAMPLE if Kc is not None else 0) | (_lib.FB_PER_SAMPLE if Kg is not None else 0) | (_lib.FB_CLAMP if clamp else 0)
        applied = C.c_void_p(res["ctrl"].data_ptr()) if "ctrl" in res else None
        self._call_envs("rsr_physics_feedback_rollouts", who, ids, C.c_void_p(c.data_ptr()), C.byref(fb), C.byref(ps), K, T, nsteps, flags,
                        C.byref(ptrs), applied, checked=True, hold=(c, g, qr, vr, *leaves))
        return res

    def cost_rollouts(self, ctrl, cost, feedback=None, params=None, nsteps: Optional[int] = None, fields: Sequence[str] = (),
                      env_ids=None, clamp: bool = False, out: Optional[Dict[str, Any]] = None, K: Optional[int] = None,
                      step_cost: bool = False, terms: bool = False, residual: bool = False) -> Dict[str, Any]:
        """What every sampling planner, an iLQR line search and system identification end in: the rollouts of param_rollouts
        (`feedback` None: open loop) or feedback_rollouts (`feedback` a dict with gain, qpos_ref, qvel_ref as that method takes
        them), with the running cost of every sample formed on the device, [M, K] numbers instead of [M, K, T, w] trajectories.
        ctrl, params, nsteps, env_ids (here an env may be listed more than once), clamp and K are feedback_rollouts'; the
        trajectories are the same bit for bit.  `cost` is a dict of float32 tensors on the env's device, rows by env and control
        step, shared by an env's K samples: the weights
        w_qpos [M, T, nv], w_qvel [M, T, nv], w_ctrl [M, T, nu], w_sensor [M, T, nsensordata] (a weight not given: that term is
        off; at least one must be) and the references qpos_ref [M, T, nq] (needed by w_qpos and by `residual`), qvel_ref
        [M, T, nv], ctrl_ref [M, T, nu], sensor_ref [M, T, nsensordata] (not given: zeros).  At the end of control step t
            c_t = 1/2 (w_qpos . dq^2 + w_qvel . dv^2 + w_ctrl . du^2 + w_sensor . ds^2),
        dq = qpos (-) qpos_ref[., t] in the tangent space (exactly 0 on the reference), dv = qvel - qvel_ref[., t], du = the
        control that was applied - ctrl_ref[., t], ds = that step's sensordata - sensor_ref[., t]; a terminal cost is a heavier
        row T - 1.  fp32 in a fixed order (include/rsr_physics.h): a sample's numbers do not depend on M, K, its slot or on what
        else is asked for.  Returns {"cost": [M, K]} and, when asked, "step_cost" [M, K, T], "terms" [M, K, 4] (the sums over t
        of the qpos, qvel, ctrl and sensor terms), "dx" [M, K, T, 2 nv] (`residual`: dq | dv, what the cost expansion of
        lqr_backward takes) and `fields` (ROLLOUT_FIELDS and "ctrl", as feedback_rollouts; default none).  `out`: caller-owned
        float32 tensors to fill instead of new ones, by those names.  Writes nothing else: the record, every buffer of the handle
        and the batch's own leaf tensors stay as they are."""
        who = "cost_rollouts"
        nsteps = self._steps(who, nsteps)
        ids = None if env_ids is None else self._ids(env_ids, who, repeats=True)       # (an env may be listed more than once)
        d, nsd = self.dims, self.nsensordata
        M, nu, nv, nq = self.num_envs if ids is None else int(ids.numel()), int(d.nu), int(d.nv), int(d.nq)
        Kc, T = self._rows(who, "ctrl", ctrl, M, (nu,), (3, 4))
        # the cost rows: [M, T, w], by slot
        if not isinstance(cost, dict):
            raise ValueError(f"{who}: cost must be a dict with some of {_lib.COST_WEIGHTS + _lib.COST_REFS}, got {type(cost).__name__}")
        unknown = sorted(set(cost) - set(_lib.COST_WEIGHTS + _lib.COST_REFS))
        if unknown:
            raise ValueError(f"{who}: cost has {unknown}; it may hold {_lib.COST_WEIGHTS + _lib.COST_REFS}")
        cost = {k: v for k, v in cost.items() if v is not None}
        if not any(w in cost for w in _lib.COST_WEIGHTS):
            raise ValueError(f"{who}: cost gives no weight: at least one of {_lib.COST_WEIGHTS} is needed")
        if "qpos_ref" not in cost and ("w_qpos" in cost or residual):
            raise ValueError(f"{who}: cost['qpos_ref'] is needed by {'w_qpos' if 'w_qpos' in cost else 'residual=True'}")
        if nsd == 0 and ("w_sensor" in cost or "sensor_ref" in cost):
            raise ValueError(f"{who}: cost['w_sensor'] / cost['sensor_ref'] given but no sensors are set (set_sensors)")
        width = dict(qpos_ref=nq, qvel_ref=nv, ctrl_ref=nu, sensor_ref=nsd, w_qpos=nv, w_qvel=nv, w_ctrl=nu, w_sensor=nsd)
        cs, rows = _lib.Cost(), []
        for name, t in cost.items():
            shape = (M, T, width[name])
            self._f32(f"{who} expects cost[{name!r}] as", t, str(shape), shape, False)
            t = t.contiguous()
            setattr(cs, name, t.data_ptr())
            rows.append(t)
        # the gain rows, as feedback_rollouts takes them
        fb, Kg = None, None
        if feedback is not None:
            if not isinstance(feedback, dict) or set(feedback) != {"gain", "qpos_ref", "qvel_ref"} or any(v is None for v in feedback.values()):
                raise ValueError(f"{who}: feedback must be None or a dict with gain, qpos_ref and qvel_ref")
            Kg, Tg = self._rows(who, "feedback['gain']", feedback["gain"], M, (nu, 2 * nv), (4, 5))
            fb_rank = feedback["gain"].dim() - 1
            Kq, Tq = self._rows(who, "feedback['qpos_ref']", feedback["qpos_ref"], M, (nq,), (fb_rank,))
            Kv, Tv = self._rows(who, "feedback['qvel_ref']", feedback["qvel_ref"], M, (nv,), (fb_rank,))
            if (Tg, Tq, Tv) != (T, T, T):
                raise ValueError(f"{who}: feedback's gain, qpos_ref and qvel_ref have T = {Tg}, {Tq}, {Tv}, ctrl T = {T}")
            if (Kq, Kv) != (Kg, Kg):
                raise ValueError(f"{who}: feedback's gain, qpos_ref and qvel_ref have K = {Kg}, {Kq}, {Kv}")
            g, qr, vr = (feedback[k].contiguous() for k in ("gain", "qpos_ref", "qvel_ref"))
            fb = _lib.Feedback(g.data_ptr(), qr.data_ptr(), vr.data_ptr())
            rows += [g, qr, vr]
        elif clamp:
            raise ValueError(f"{who}: clamp=True needs feedback")
        for name, k in (("ctrl", Kc), ("feedback", Kg)):
            if k is not None and K is not None and k != int(K):
                raise ValueError(f"{who}: {name} has K = {k}, the others (or the K given) K = {int(K)}")
            K = k if k is not None else K
        if K is not None and int(K) < 1:
            raise ValueError(f"{who}: K must be >= 1, got {K}")
        ps, leaves, K = self._sampled_leaves(who, params, M, None if K is None else int(K))
        if K is None:
            raise ValueError(f"{who}: K is not given: pass it, or a per-sample ctrl, gain or leaf")
        res, ptrs = self._trajectory_out(who, fields, (M, K, T), out, extra=dict(ctrl=nu), none_ok=True)
        shapes = dict(cost=(M, K))
        shapes.update({k: s for k, s, on in (("step_cost", (M, K, T), step_cost), ("terms", (M, K, 4), terms),
                                             ("dx", (M, K, T, 2 * nv), residual)) if on})
        mine = self._outputs(who, shapes, out, False)
        co = _lib.CostOut(**{k: t.data_ptr() for k, t in mine.items()})
        if "ctrl" in res:
            co.ctrl = res["ctrl"].data_ptr()
        c = ctrl.contiguous()
        flags = (_lib.FB_CTRL_PER_SAMPLE if Kc is not None else 0) | (_lib.FB_PER_SAMPLE if Kg is not None else 0) | (_lib.FB_CLAMP if clamp else 0)
        self._call_envs("rsr_physics_cost_rollouts", who, ids, C.c_void_p(c.data_ptr()), None if fb is None else C.byref(fb), C.byref(ps),
                        C.byref(cs), K, T, nsteps, flags, C.byref(ptrs), C.byref(co), checked=True, hold=(c, *rows, *leaves))
        return {**mine, **res}

    def cost_expand(self, cost, dx=None, ctrl=None, sensordata=None, columns=None, out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """The cost model of an iLQR iteration from the one statement of the cost: the `cost` dict of cost_rollouts expanded to
        second order about a nominal run, into exactly what lqr_backward takes:
            phys.lqr_backward(fd["columns"], **phys.cost_expand(cost, dx=..., ctrl=..., sensordata=..., columns=fd["columns"])).
        M independent problems, one launch with one wave per (slot, step); nothing of the env is read: the handle gives nv and
        nu, M and T come from the cost rows and ny from w_sensor.  All float32 tensors on the env's device, nx = 2 nv:
        cost: the weights w_qpos, w_qvel [M, T, nv], w_ctrl [M, T, nu], w_sensor [M, T, ny] (1 <= ny <= 64; a weight not given:
        that term is off; at least one must be) and the references ctrl_ref [M, T, nu], sensor_ref [M, T, ny] (not given: zeros);
        qpos_ref and qvel_ref are accepted and ignored, so that the same dict serves both calls: the state residual arrives
        formed, as dx.  dx [M, T, nx]: dq | dv at the end of control step t on the nominal run, the "dx" rows of
        cost_rollouts(..., residual=True) for the nominal sample (differentiate_state gives the same from states); needed by
        w_qpos / w_qvel.  ctrl [M, T, nu]: the control that was applied; needed by w_ctrl.  sensordata [M, T, ny] and columns
        [M, T, nx + nu, w], w >= nx + ny (trajectory_fd(...)["columns"] as it is: its C and D blocks are the sensor entries of
        the rows): needed by w_sensor.  An input its terms do not need is not read.  Returns lx [M, T+1, nx], lu [M, T, nu],
        lxx [M, T+1, nx, nx], luu [M, T, nu, nu], lux [M, T, nu, nx], every element written: the state terms of cost row t land
        on index t + 1 (row T is the terminal cost), its ctrl and sensor terms on index t, the sensor terms through the
        Gauss-Newton products C^T W C, D^T W C, D^T W D and the gradients C^T W ds, D^T W ds.  The expansion is exact for the
        ctrl, qvel, hinge, slide and translation terms; for a free joint's rotation the Jacobian of dq is taken as the identity,
        which is first order in the rotation error (trajectory_fd perturbs in the same local frame), and the sensors' second
        derivatives are dropped.  fp32 in a fixed order (include/rsr_physics.h): a problem's numbers depend on its own inputs
        alone, bit for bit; lxx and luu are symmetric bit for bit; with w_sensor off the outputs are the plain products and
        exactly diagonal matrices.  `out`: caller-owned float32 tensors under those names to fill instead of new ones.  Writes
        nothing else."""
        who = "cost_expand"
        d = self.dims
        nv, nu = int(d.nv), int(d.nu)
        nx, ncol = 2 * nv, 2 * nv + nu
        names = _lib.COST_WEIGHTS + _lib.COST_REFS
        if not isinstance(cost, dict):
            raise ValueError(f"{who}: cost must be a dict with some of {names}, got {type(cost).__name__}")
        unknown = sorted(set(cost) - set(names))
        if unknown:
            raise ValueError(f"{who}: cost has {unknown}; it may hold {names}")
        cost = {k: v for k, v in cost.items() if v is not None and k not in ("qpos_ref", "qvel_ref")}
        given = [w for w in _lib.COST_WEIGHTS if w in cost]
        if not given:
            raise ValueError(f"{who}: cost gives no weight: at least one of {_lib.COST_WEIGHTS} is needed")
        first = cost[given[0]]
        self._f32(f"{who} expects cost[{given[0]!r}] as", first, "(M >= 1, T >= 1, width)",
                  lambda t: t.dim() == 3 and t.shape[0] >= 1 and t.shape[1] >= 1, False)
        M, T = int(first.shape[0]), int(first.shape[1])
        if M * (T + 1) >= 2 ** 31:
            raise ValueError(f"{who}: M * (T + 1) must stay below 2^31")
        ny = 0
        if "w_sensor" in cost:
            self._f32(f"{who} expects cost['w_sensor'] as", cost["w_sensor"], f"({M}, {T}, 1 <= ny <= {_lib.MAX_SENSORDATA})",
                      lambda t: t.dim() == 3 and 1 <= t.shape[2] <= _lib.MAX_SENSORDATA, False)
            ny = int(cost["w_sensor"].shape[2])
        width = dict(ctrl_ref=nu, sensor_ref=ny, w_qpos=nv, w_qvel=nv, w_ctrl=nu, w_sensor=ny)
        cs, held = _lib.Cost(), []
        for name, t in cost.items():
            if name == "sensor_ref" and "w_sensor" not in cost:      # (its term is off: not read)
                continue
            shape = (M, T, width[name])
            self._f32(f"{who} expects cost[{name!r}] as", t, str(shape), shape, False)
            t = t.contiguous()
            setattr(cs, name, t.data_ptr())
            held.append(t)
        nom = _lib.CostNominal()
        needs = (("dx", dx, (M, T, nx), ("w_qpos", "w_qvel")), ("ctrl", ctrl, (M, T, nu), ("w_ctrl",)),
                 ("sensordata", sensordata, (M, T, ny), ("w_sensor",)))
        for name, t, shape, by in needs:
            by = [w for w in by if w in cost]
            if by:
                self._f32(f"{who} expects {name} (needed by {by[0]}) as", t, f"{shape} (M and T as the cost rows have them)", shape, True)
                setattr(nom, name, t.data_ptr())
                held.append(t)
        col_ptr, w = None, 0
        if "w_sensor" in cost:
            self._f32(f"{who} expects columns (needed by w_sensor) as", columns, f"({M}, {T}, {ncol}, w >= {nx + ny})",
                      lambda t: t.dim() == 4 and tuple(t.shape[:3]) == (M, T, ncol) and t.shape[3] >= nx + ny, True)
            col_ptr, w = C.c_void_p(columns.data_ptr()), int(columns.shape[3])
            held.append(columns)
        res = self._outputs(who, dict(lx=(M, T + 1, nx), lu=(M, T, nu), lxx=(M, T + 1, nx, nx), luu=(M, T, nu, nu), lux=(M, T, nu, nx)), out, True)
        ptrs = _lib.CostExpansion(**{f: t.data_ptr() for f, t in res.items()})
        self._held[who] = tuple(held)
        _lib.check(_lib.lib().rsr_physics_cost_expand(self._h, M, T, col_ptr, w, ny, C.byref(cs), C.byref(nom), C.byref(ptrs), self._stream()))
        return res

    def trajectory_fd(self, ctrl, nsteps: Optional[int] = None, eps: float = 1e-3, centered: bool = True, env_ids=None,
                      nominal: bool = True, out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """What the backward pass of iLQR, a time-varying LQR, linearised MPC and an EKF smoother ask: transition_fd at every
        control step of a nominal trajectory, in two launches and without advancing the env.  ctrl is a float32 tensor
        [M, T, nu] on the env's device, M = len(env_ids) (default: every env; an env may be listed more than once, e.g. with
        several candidate plans).  From the record of env env_ids[s] as it stands (qpos, qvel, qacc_warmstart, time), with that
        env's per-env leaves and applied forces, the nominal run applies ctrl[s, t] then `nsteps` (default n_substeps) x
        mjx.step for t < T: bit for bit what sample_rollouts records with K = 1.  Then, one wave per (slot, t, column), the
        finite differences of transition_fd (same columns, `eps`, `centered`) about the state before control step t, the warm
        start the nominal run carried there included: bit for bit what T rounds of transition_fd() then step(ctrl[:, t]) give.
        Returns a dict: columns [M, T, ncol, 2 nv + nsensordata] (ncol = 2 nv + nu, one tight row per perturbed coordinate) and
        its zero-copy views A [M, T, 2nv, 2nv], B [M, T, 2nv, nu], C [M, T, nsensordata, 2nv], D [M, T, nsensordata, nu], oriented
        as fd_A .. fd_D; with `nominal`, qpos [M, T+1, nq] and qvel [M, T+1, nv], row 0 the start state and row t + 1 the state
        after control step t.  `out`: caller-owned float32 tensors ("columns", "qpos", "qvel") to fill instead of new ones.
        Writes nothing else but a scratch buffer of the handle: the record, the side buffer, sensordata and every other buffer
        of the handle stay as they are.  Two calls on one Physics must not overlap on different streams (they share the scratch)."""
        who = "trajectory_fd"
        nsteps, eps = self._steps(who, nsteps, below_2_30=True), _eps(who, eps)
        ids = None if env_ids is None else self._ids(env_ids, who, repeats=True)
        d = self.dims
        M, nu, nv, nq, nsd = self.num_envs if ids is None else int(ids.numel()), int(d.nu), int(d.nv), int(d.nq), self.nsensordata
        self._f32(f"{who} expects ctrl as", ctrl, f"({M}, T >= 1, {nu})",
                  lambda t: t.dim() == 3 and t.shape[0] == M and t.shape[2] == nu and t.shape[1] >= 1, False)
        T, ncol, w = int(ctrl.shape[1]), 2 * nv + nu, 2 * nv + nsd
        if T * nsteps >= 2 ** 31 or M * T * ncol >= 2 ** 31:
            raise ValueError(f"{who}: T * nsteps and M * T * ncol must stay below 2^31")
        shapes = dict(columns=(M, T, ncol, w))
        if nominal:
            shapes.update(qpos=(M, T + 1, nq), qvel=(M, T + 1, nv))
        res = self._outputs(who, shapes, out, True, "" if nominal else " (nominal=False)")
        ptrs = _lib.TrajectoryFdOut(**{f: t.data_ptr() for f, t in res.items()})
        c = ctrl.contiguous()
        self._call_envs("rsr_physics_trajectory_fd", who, ids, C.c_void_p(c.data_ptr()), T, nsteps, eps, _lib.FD_CENTERED if centered else 0,
                        C.byref(ptrs), checked=True, hold=(c,))
        # the buffer holds one row per column of [A B; C D]: the blocks are transposed views, as fd_A .. fd_D
        col, x, u, sn = res["columns"], slice(0, 2 * nv), slice(2 * nv, ncol), slice(2 * nv, w)
        res.update(A=col[:, :, x, x].transpose(2, 3), B=col[:, :, u, x].transpose(2, 3), C=col[:, :, x, sn].transpose(2, 3),
                   D=col[:, :, u, sn].transpose(2, 3))
        return res

    def lqr_backward(self, columns, lx, lu, lxx, luu, lux=None, mu=0.0, state_reg: bool = False, values: bool = False,
                     out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """The backward pass of iLQR / time-varying LQR, the step between trajectory_fd and feedback_rollouts: the Riccati
        recursion of Tassa et al. 2012 (the unregularised Q in the value update) on M independent problems, one launch with one
        wave per slot and T steps inside it.  Nothing of the env is read: the handle gives nv and nu, and M is whatever the
        buffers hold.  All float32 tensors on the env's device, contiguous, nx = 2 nv, ncol = nx + nu:
        columns [M, T, ncol, w], w >= nx: trajectory_fd(...)["columns"] as it is (w = 2 nv + nsensordata; the sensor entries of
        a row are never read), i.e. A_t = columns[:, t, :nx, :nx]^T, B_t = columns[:, t, nx:, :nx]^T in the tangent space;
        lx [M, T+1, nx], lxx [M, T+1, nx, nx] (row T: the terminal cost), lu [M, T, nu], luu [M, T, nu, nu], lux [M, T, nu, nx] or
        None (zero); lxx and luu symmetric.  mu: a float or a tensor [M], the regularisation of each slot: Quu + mu I, or with
        `state_reg` Quu + mu B^T B and Qux + mu B^T A.  Returns gain [M, T, nu, nx] (what feedback_rollouts takes as `gain`),
        k [M, T, nu] (an iLQR line search passes ctrl + alpha * k per sample), dV [M, 2] (the expected cost change at step alpha
        is alpha dV[0] + alpha^2 dV[1]), status [M] (-1, or the step t whose Quu~ had a Cholesky pivot <= 0 or not finite: that
        slot stopped there with dV = 0, its rows t' > t written and its rows t' <= t left alone; raise its mu and call again)
        and, with `values`, Vx [M, T+1, nx] and Vxx [M, T+1, nx, nx].  `out`: caller-owned float32 tensors under those names to
        fill instead of new ones.  A slot's result depends on that slot's inputs alone, bit for bit.  Writes nothing else."""
        who = "lqr_backward"
        M, T, w, mu_t, res = self._lqr_io(who, columns, lx, lu, lxx, luu, lux, mu, values, out)
        ptrs = _lib.LqrOut(**{dict(dV="dv", Vx="vx", Vxx="vxx").get(f, f): t.data_ptr() for f, t in res.items()})
        cost = _lib.LqrCost(lx.data_ptr(), lu.data_ptr(), lxx.data_ptr(), luu.data_ptr(), None if lux is None else lux.data_ptr())
        self._held[who] = (columns, lx, lu, lxx, luu, lux, mu_t)
        _lib.check(_lib.lib().rsr_physics_lqr_backward(self._h, M, T, C.c_void_p(columns.data_ptr()), w, C.byref(cost),
                                                       C.c_void_p(mu_t.data_ptr()), _lib.LQR_REG_STATE if state_reg else 0,
                                                       C.byref(ptrs), self._stream()))
        return res

    def _lqr_io(self, who: str, columns, lx, lu, lxx, luu, lux, mu, values: bool, out, extra=None):
        """What lqr_backward and lqr_backward_box share ahead of the C call: the inputs checked, mu as a tensor [M] and the outputs
        (`extra`: further {name: shape} a caller may also pass in `out`).  Returns M, T, w, mu_t and the outputs."""
        import torch
        d, dev = self.dims, self.qvel.device
        nv, nu = int(d.nv), int(d.nu)
        nx, ncol = 2 * nv, 2 * nv + nu

        self._f32(f"{who} expects columns as", columns, f"(M >= 1, T >= 1, {ncol}, w >= {nx})",
                  lambda t: t.dim() == 4 and t.shape[0] >= 1 and t.shape[1] >= 1 and t.shape[2] == ncol and t.shape[3] >= nx, True)
        M, T, w = int(columns.shape[0]), int(columns.shape[1]), int(columns.shape[3])
        if M * (T + 1) >= 2 ** 31:
            raise ValueError(f"{who}: M * (T + 1) must stay below 2^31")
        shapes = dict(lx=(M, T + 1, nx), lu=(M, T, nu), lxx=(M, T + 1, nx, nx), luu=(M, T, nu, nu), lux=(M, T, nu, nx))
        for name, t in dict(lx=lx, lu=lu, lxx=lxx, luu=luu, lux=lux).items():
            if t is not None or name != "lux":
                self._f32(f"{who} expects {name} as", t, f"{shapes[name]} (M and T as columns has them)", shapes[name], True)
        if torch.is_tensor(mu):
            self._f32(f"{who} expects mu as", mu, f"({M},), or a float", (M,), True)
            mu_t = mu
        else:
            try:
                mu_t = torch.full((M,), float(mu), dtype=torch.float32, device=dev)
            except (TypeError, ValueError):
                raise ValueError(f"{who} expects mu as a float or a float32 tensor of shape ({M},) on {dev}") from None
        oshapes = dict(gain=(M, T, nu, nx), k=(M, T, nu), dV=(M, 2), status=(M,))
        if values:
            oshapes.update(Vx=(M, T + 1, nx), Vxx=(M, T + 1, nx, nx))
        oshapes.update(extra(M, T) if extra else {})
        return M, T, w, mu_t, self._outputs(who, oshapes, out, True, "" if values else " (values=False)")

    def lqr_backward_box(self, columns, lx, lu, lxx, luu, lo, hi, lux=None, mu=0.0, state_reg: bool = False, values: bool = False,
                         max_iter: int = 32, report: bool = False, out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """The control-limited backward pass (box-DDP: Tassa, Mansard and Todorov 2014), the one that agrees with
        feedback_rollouts(..., clamp=True): lqr_backward with k_t the minimiser of the step's quadratic model over
        lo_t <= k_t <= hi_t, and the gain rows of the clamped controls zero, so that k points into the feasible set, the gain
        promises no feedback the clamp swallows and dV is a change the rollout can deliver.  Inputs, `mu`, `state_reg`, `values`,
        `out` and the layout are lqr_backward's.  lo, hi [M, T, nu]: the bounds on the control *change*, ctrlrange - u_nom
        (ctrl_bounds(u_nom) gives them; -inf / +inf: no bound).  The QP of a step is solved on the device inside the recursion
        by projected Newton steps, at most `max_iter` of them (1 .. 64; include/rsr_physics.h states the iteration line by
        line).  Returns lqr_backward's dict and, with `report`, clamped [M, T, nu] (-1 at lo, +1 at hi, 0 free) and qp [M, T, 2]
        (Newton steps taken, and a code: 0 converged, 1 every control clamped, 2 max_iter reached, 3 the line search found no
        descent).  status [M] is -1, or the step t at which a Cholesky pivot was bad or the bounds were not ordered (lo > hi, or
        a NaN).  With infinite bounds, and with bounds no step reaches, every output is lqr_backward's bit for bit.  Writes
        nothing else."""
        who = "lqr_backward_box"
        nu = int(self.dims.nu)
        if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 1 <= max_iter <= 64:
            raise ValueError(f"{who}: max_iter must be an int in [1, 64], got {max_iter!r}")
        extra = (lambda M, T: dict(clamped=(M, T, nu), qp=(M, T, 2))) if report else None
        M, T, w, mu_t, res = self._lqr_io(who, columns, lx, lu, lxx, luu, lux, mu, values, out, extra)
        for name, t in (("lo", lo), ("hi", hi)):
            self._f32(f"{who} expects {name} as", t, f"{(M, T, nu)} (M and T as columns has them)", (M, T, nu), True)
        names = dict(dV="dv", Vx="vx", Vxx="vxx")
        ptrs = _lib.LqrOut(**{names.get(f, f): t.data_ptr() for f, t in res.items() if f not in ("clamped", "qp")})
        cost = _lib.LqrCost(lx.data_ptr(), lu.data_ptr(), lxx.data_ptr(), luu.data_ptr(), None if lux is None else lux.data_ptr())
        box = _lib.LqrBox(lo.data_ptr(), hi.data_ptr(), res["clamped"].data_ptr() if report else None, res["qp"].data_ptr() if report else None)
        self._held[who] = (columns, lx, lu, lxx, luu, lux, mu_t, lo, hi)
        _lib.check(_lib.lib().rsr_physics_lqr_box(self._h, M, T, C.c_void_p(columns.data_ptr()), w, C.byref(cost), C.byref(box),
                                                  C.c_void_p(mu_t.data_ptr()), max_iter, _lib.LQR_REG_STATE if state_reg else 0,
                                                  C.byref(ptrs), self._stream()))
        return res

    def ctrl_bounds(self, u_nom):
        """(lo, hi) for lqr_backward_box about the nominal controls u_nom [M, T, nu] (float32, on the env's device): float32
        [M, T, nu], contiguous, actuator_ctrlrange - u_nom where the actuator is ctrl-limited (what feedback_rollouts' clamp
        clips to), -inf / +inf elsewhere.  Plain torch; nothing of the env's state is read."""
        import numpy as np
        import torch
        nu = int(self.dims.nu)
        self._f32("ctrl_bounds expects u_nom as", u_nom, f"(M, T, {nu})", lambda t: t.dim() == 3 and t.shape[2] == nu, False)
        A = self.env.sys.arrays
        rng = np.asarray(A["actuator_ctrlrange"], np.float32).reshape(nu, 2)
        lim = np.asarray(A["actuator_ctrllimited"]).reshape(nu) != 0
        lo_r = torch.as_tensor(np.where(lim, rng[:, 0], -np.inf).astype(np.float32), device=u_nom.device)
        hi_r = torch.as_tensor(np.where(lim, rng[:, 1], np.inf).astype(np.float32), device=u_nom.device)
        return (lo_r - u_nom).contiguous(), (hi_r - u_nom).contiguous()

    def kalman_smooth(self, columns, dy, r, q, P0, x0=None, smooth: bool = True, covariances: bool = False,
                      out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """A linear time-varying Kalman filter with a Rauch-Tung-Striebel smoother over a log, the consumer of trajectory_fd's
        sensor Jacobians: M independent problems, one launch with one wave per slot and the T steps inside it.  The state is
        the deviation dx_t from the nominal run in the tangent space, nx = 2 nv (an error-state / linearised EKF):
        dx_{t+1} = A_t dx_t + w_t, dy_t = C_t dx_t + v_t.  Nothing of the env is read: the handle gives nv and nu, and M is
        whatever the buffers hold.  All float32 tensors on the env's device, contiguous, ncol = nx + nu:
        columns [M, T, ncol, w]: trajectory_fd(...)["columns"] as it is, ny = w - nx sensor entries (1 <= ny <= 64; the B and D
        rows are never read); dy [M, T, ny]: the measured sensordata minus the nominal run's (sample_rollouts with K = 1 on the
        same record); r [M, T, ny] or [M, ny]: the measurement variances, +inf where a sample is missing (skipped exactly);
        q [M, T, nx] or [M, nx]: the process-noise variances, finite and >= 0; P0 [M, nx, nx], symmetric, and x0 [M, nx] or None
        (zeros): the prior on dx_0.  The measurement update takes one sensor entry at a time (R is diagonal), so no ny x ny
        matrix is factorised.  Returns xf [M, T+1, nx] and Pf [M, T+1, nx, nx] (row t: after step t's measurements; row T: a
        prediction), nll [M] (the innovation negative log-likelihood), status [M, 2] (filter, smoother: -1, or the step that
        failed: a variance r that is neither +inf nor finite and > 0, an innovation variance that is not finite and > 0, or a
        Cholesky pivot of the smoother's predicted covariance that is; that slot stopped there with the rows before the failure
        written, nll = 0 after a filter failure and no smoother; the other slots are unaffected) and, with `smooth`, xs
        [M, T+1, nx], and Ps [M, T+1, nx, nx] with `covariances`.  `out`: caller-owned float32 tensors under those names to fill
        instead of new ones.  A slot's result depends on that slot's inputs alone, bit for bit; smooth=False gives the same xf,
        Pf and nll bit for bit.  Writes nothing else: adopt xs[:, 0] with integrate_state and set_state."""
        import torch
        who = "kalman_smooth"
        d = self.dims
        nv, nu = int(d.nv), int(d.nu)
        nx, ncol = 2 * nv, 2 * nv + nu
        if covariances and not smooth:
            raise ValueError(f"{who}: covariances=True needs smooth=True")
        self._f32(f"{who} expects columns as", columns, f"(M >= 1, T >= 1, {ncol}, {nx} < w <= {nx + _lib.MAX_SENSORDATA})",
                  lambda t: t.dim() == 4 and t.shape[0] >= 1 and t.shape[1] >= 1 and t.shape[2] == ncol
                  and nx < t.shape[3] <= nx + _lib.MAX_SENSORDATA, True)
        M, T, w = int(columns.shape[0]), int(columns.shape[1]), int(columns.shape[3])
        ny = w - nx
        if M * (T + 1) >= 2 ** 31:
            raise ValueError(f"{who}: M * (T + 1) must stay below 2^31")
        self._f32(f"{who} expects dy as", dy, f"{(M, T, ny)} (M, T and ny as columns has them)", (M, T, ny), True)
        wide = {}
        for name, t, n in (("r", r, ny), ("q", q, nx)):
            self._f32(f"{who} expects {name} as", t, f"{(M, T, n)} or {(M, n)}",
                      lambda t, n=n: tuple(t.shape) in ((M, T, n), (M, n)), True)
            wide[name] = t if t.dim() == 3 else t[:, None, :].expand(M, T, n).contiguous()
        self._f32(f"{who} expects P0 as", P0, (M, nx, nx), (M, nx, nx), True)
        if x0 is not None:
            self._f32(f"{who} expects x0 as", x0, f"{(M, nx)}, or None", (M, nx), True)
        oshapes = dict(xf=(M, T + 1, nx), Pf=(M, T + 1, nx, nx))
        if smooth:
            oshapes.update(xs=(M, T + 1, nx))
        if covariances:
            oshapes.update(Ps=(M, T + 1, nx, nx))
        oshapes.update(nll=(M,), status=(M, 2))
        res = self._outputs(who, oshapes, out, True, f" (smooth={smooth}, covariances={covariances})")
        ptrs = _lib.KalmanOut(**{dict(Pf="pf", Ps="ps").get(f, f): t.data_ptr() for f, t in res.items()})
        ins = _lib.KalmanIn(dy.data_ptr(), wide["r"].data_ptr(), wide["q"].data_ptr(), None if x0 is None else x0.data_ptr(), P0.data_ptr())
        self._held[who] = (columns, dy, r, q, wide["r"], wide["q"], P0, x0)
        _lib.check(_lib.lib().rsr_physics_kalman(self._h, M, T, C.c_void_p(columns.data_ptr()), w, ny, C.byref(ins), 0,
                                                 C.byref(ptrs), self._stream()))
        return res

    def integrate_state(self, qpos, qvel, dx):
        """A tangent-space deviation applied to a state: (qpos', qvel') = (mj_integratePos(qpos, dx[..., :nv]) with dt = 1,
        qvel + dx[..., nv:]), in torch, for any leading dims (qpos [..., nq], qvel [..., nv], dx [..., 2 nv], the same leading
        dims).  A free joint's rotation dofs are a body-frame rotation vector, q' = q * exp(v / 2), and its quaternion is
        normalised.  It is how a smoothed dx_0 of kalman_smooth becomes the state set_state takes; nothing of the batch is read
        but the model's joint table, and nothing is written."""
        import torch
        who = "integrate_state"
        nq, nv = int(self.dims.nq), int(self.dims.nv)
        for name, t, n in (("qpos", qpos, nq), ("qvel", qvel, nv), ("dx", dx, 2 * nv)):
            if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() < 1 or t.shape[-1] != n:
                raise ValueError(f"{who} expects {name} as a floating-point tensor of shape (..., {n})")
        if not (qpos.shape[:-1] == qvel.shape[:-1] == dx.shape[:-1]):
            raise ValueError(f"{who}: qpos, qvel and dx must have the same leading dims")
        A = self.env.sys.arrays
        dq = dx[..., :nv]
        out = qpos.clone()
        for j in range(len(A["jnt_type"])):
            jt, qa, da = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
            if jt == 0:                                   # free: translation, then q * exp(v / 2)
                out[..., qa:qa + 3] = qpos[..., qa:qa + 3] + dq[..., da:da + 3]
                v = dq[..., da + 3:da + 6]
                ang = v.norm(dim=-1, keepdim=True)
                h = 0.5 * ang
                f = torch.where(ang > 0, torch.sin(h) / torch.where(ang > 0, ang, torch.ones_like(ang)), torch.full_like(ang, 0.5))
                bw, bv = torch.cos(h), v * f
                aw, av = qpos[..., qa + 3:qa + 4], qpos[..., qa + 4:qa + 7]
                qn = torch.cat([aw * bw - (av * bv).sum(-1, keepdim=True), aw * bv + bw * av + torch.linalg.cross(av, bv, dim=-1)], dim=-1)
                out[..., qa + 3:qa + 7] = qn / qn.norm(dim=-1, keepdim=True)
            elif jt in (2, 3):                            # slide, hinge
                out[..., qa] = qpos[..., qa] + dq[..., da]
            else:
                raise ValueError(f"{who}: joint {j} has type {jt}; only free, slide and hinge joints are supported")
        return out, qvel + dx[..., nv:]

    def differentiate_state(self, qpos, qvel, qpos_ref, qvel_ref):
        """The inverse of integrate_state: the tangent-space deviation dx [..., 2 nv] = (mj_differentiatePos(qpos_ref -> qpos)
        with dt = 1 | qvel - qvel_ref) of a state from a reference, in torch, for any leading dims (qpos, qpos_ref [..., nq],
        qvel, qvel_ref [..., nv], the same leading dims): dq | dv as cost_rollouts(..., residual=True) forms them, for a caller who
        has states but no rollout (a terminal row of their own for cost_expand, say).  A free joint's rotation dofs are the
        body-frame rotation vector of conj(q_ref) q, exactly 0 where the two quaternions are equal.  Nothing of the batch is read
        but the model's joint table, and nothing is written."""
        import math
        import torch
        who = "differentiate_state"
        nq, nv = int(self.dims.nq), int(self.dims.nv)
        for name, t, n in (("qpos", qpos, nq), ("qvel", qvel, nv), ("qpos_ref", qpos_ref, nq), ("qvel_ref", qvel_ref, nv)):
            if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() < 1 or t.shape[-1] != n:
                raise ValueError(f"{who} expects {name} as a floating-point tensor of shape (..., {n})")
        if not (qpos.shape[:-1] == qvel.shape[:-1] == qpos_ref.shape[:-1] == qvel_ref.shape[:-1]):
            raise ValueError(f"{who}: qpos, qvel, qpos_ref and qvel_ref must have the same leading dims")
        A = self.env.sys.arrays
        dq = qpos.new_zeros(qpos.shape[:-1] + (nv,))
        for j in range(len(A["jnt_type"])):
            jt, qa, da = int(A["jnt_type"][j]), int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
            if jt == 0:                                   # free: translation, then the rotation vector of conj(q_ref) q
                dq[..., da:da + 3] = qpos[..., qa:qa + 3] - qpos_ref[..., qa:qa + 3]
                w1, x1, y1, z1 = qpos_ref[..., qa + 3], -qpos_ref[..., qa + 4], -qpos_ref[..., qa + 5], -qpos_ref[..., qa + 6]
                w2, x2, y2, z2 = (qpos[..., qa + 3 + k] for k in range(4))
                # (each component sums its two w terms first, then its cross pair: at equal quaternions each pair cancels exactly)
                w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
                v = torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 - x1 * z2 + z1 * x2,
                                 w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2], -1)
                sn = v.norm(dim=-1)
                ang = 2.0 * torch.atan2(sn, w)
                ang = torch.where(ang > math.pi, ang - 2.0 * math.pi, ang)
                f = torch.where(sn > 0, ang / torch.where(sn > 0, sn, torch.ones_like(sn)), torch.zeros_like(sn))
                dq[..., da + 3:da + 6] = v * f[..., None]
            elif jt in (2, 3):                            # slide, hinge
                dq[..., da] = qpos[..., qa] - qpos_ref[..., qa]
            else:
                raise ValueError(f"{who}: joint {j} has type {jt}; only free, slide and hinge joints are supported")
        return torch.cat([dq, qvel - qvel_ref], dim=-1)

    def ik(self, sites, target_pos, target_quat=None, pos_weight=1.0, rot_weight=None, dofs=None, qpos0=None, damping=1e-3,
           iters: int = 20, tol_pos: float = 1e-4, tol_rot: float = 1e-3, max_step: float = 0.3, limits: bool = True,
           env_ids=None, out: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """Inverse kinematics on site pose targets: which qpos puts these sites there.  Damped least squares (Levenberg-Marquardt
        with a fixed damping) on M independent problems, one launch with one wave per slot and every iteration inside it.
        M = len(env_ids) (default: every env; an env may be listed more than once): slot s takes its model, its per-env leaves
        and its default start from env env_ids[s].  All tensors float32, contiguous, on the env's device.
        sites: 1 to _lib.MAX_JAC_SITES site names or ids, K of them, one table for every slot (independent of set_jac_sites);
        target_pos [M, K, 3]; target_quat [M, K, 4] (w, x, y, z; normalised on the device) or None; pos_weight, rot_weight: a
        float or K floats >= 0, 0 = off (rot_weight defaults to 0 without target_quat, to 1 with it; a positive rot_weight
        without target_quat and all weights zero are errors); dofs: None for every hinge and slide dof, or dof indices, or a
        bool mask [nv] (free-joint dofs allowed); qpos0 [M, nq] or None: the record's qpos; damping: a float > 0 or a tensor
        [M] read on the device; iters >= 0; tol_pos, tol_rot >= 0 (0: every iteration runs); max_step >= 0 (0: no cap on
        max|dq|); limits: clamp hinge / slide joints to jnt_range where jnt_limited, after every step.
            q = start
            for it = 0, 1, ...:
                kinematics(q)                       # normalises free-joint quaternions in q
                e_k = p*_k - p_k;  r_k = rotation vector of R*_k R_k^T (world frame, the short way round)
                perr = max_k |e_k| (pos_weight_k > 0);  rerr = max_k |r_k| (rot_weight_k > 0)
                if it == iters or (perr <= tol_pos and rerr <= tol_rot): stop     # status 0 if the tolerances hold, else 1
                J = rows pos_weight_k jacp_k, rot_weight_k jacr_k, columns outside dofs zeroed;  b = the weighted errors
                dq = (J^T J + damping I)^-1 J^T b;  if max|dq| > max_step > 0: dq *= max_step / max|dq|
                q = mj_integratePos(q, dq);  if limits: clamp
        Returns qpos [M, nq], err [M, 2] (perr, rerr at the returned qpos), info [M, 2] int32 (iterations taken, status; status
        2: the damping was not finite and positive or dq was not finite, the slot stopped at its last q, the other slots are
        unaffected).  iters=0 is a forward-kinematics query: the start and its error.  `out`: caller-owned tensors under those
        names to fill instead of new ones.  A slot's result depends on that slot's inputs alone, bit for bit.  Nothing else is
        written, not the record and no buffer of the handle: adopt a result with set_state(qpos=res["qpos"], ...)."""
        import math
        import numpy as np
        import torch
        who = "ik"
        d, dev = self.dims, self.qvel.device
        nv, nq = int(d.nv), int(d.nq)
        ids = None if env_ids is None else self._ids(env_ids, who, repeats=True)
        M = self.num_envs if ids is None else int(ids.numel())
        site_ids = self._site_ids(who, [sites] if isinstance(sites, (str, int)) else list(sites))
        K = len(site_ids)
        if not 1 <= K <= _lib.MAX_JAC_SITES:
            raise ValueError(f"{who} expects 1 to {_lib.MAX_JAC_SITES} sites, got {K}")
        for name, t, shape in (("target_pos", target_pos, (M, K, 3)), ("target_quat", target_quat, (M, K, 4)), ("qpos0", qpos0, (M, nq))):
            if t is not None or name == "target_pos":
                self._f32(f"{who} expects {name} as", t, shape, shape, True, got=True)

        def weights(name, w):
            try:
                v = np.asarray(w, dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError(f"{who} expects {name} as a float or {K} floats") from None
            v = np.full(K, v[0]) if v.size == 1 else v
            if v.shape != (K,) or not np.isfinite(v).all() or (v < 0).any():
                raise ValueError(f"{who} expects {name} as a float or {K} floats, finite and >= 0")
            return v

        wp = weights("pos_weight", pos_weight)
        wr = weights("rot_weight", (0.0 if target_quat is None else 1.0) if rot_weight is None else rot_weight)
        if (wr > 0).any() and target_quat is None:
            raise ValueError(f"{who}: a positive rot_weight needs target_quat")
        if not ((wp > 0).any() or (wr > 0).any()):
            raise ValueError(f"{who}: every weight is zero")
        if dofs is None:
            A = self.env.sys.arrays
            sel = [int(A["jnt_dofadr"][j]) for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) in (2, 3)]
        else:
            dd = np.asarray(dofs.cpu() if torch.is_tensor(dofs) else dofs)
            if dd.dtype == np.bool_:
                if dd.shape != (nv,):
                    raise ValueError(f"{who} expects dofs as dof indices or a bool mask of shape ({nv},)")
                sel = [int(i) for i in np.nonzero(dd)[0]]
            else:
                if dd.ndim != 1 or not np.issubdtype(dd.dtype, np.integer) or ((dd < 0) | (dd >= nv)).any():
                    raise ValueError(f"{who} expects dofs as dof indices in [0, {nv}) or a bool mask of shape ({nv},)")
                sel = [int(i) for i in dd]
        mask = 0
        for i in sel:
            mask |= 1 << i
        if torch.is_tensor(damping):
            self._f32(f"{who} expects damping as", damping, (M,), (M,), True, got=True)
            lam = damping
        else:
            try:
                lam_f = float(damping)
            except (TypeError, ValueError):
                raise ValueError(f"{who} expects damping as a float > 0 or a float32 tensor of shape ({M},) on {dev}") from None
            if not (math.isfinite(lam_f) and lam_f > 0.0):
                raise ValueError(f"{who} expects damping as a float > 0 or a float32 tensor of shape ({M},) on {dev}")
            lam = torch.full((M,), lam_f, dtype=torch.float32, device=dev)
        iters = int(iters)
        if iters < 0:
            raise ValueError(f"{who}: iters must be >= 0, got {iters}")
        tol_pos, tol_rot, max_step = float(tol_pos), float(tol_rot), float(max_step)
        for name, v in (("tol_pos", tol_pos), ("tol_rot", tol_rot), ("max_step", max_step)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{who}: {name} must be finite and >= 0, got {v}")
        oshapes = dict(qpos=((M, nq), torch.float32), err=((M, 2), torch.float32), info=((M, 2), torch.int32))
        res = self._outputs(who, oshapes, out, True)
        ptrs = _lib.IkOut(**{f: t.data_ptr() for f, t in res.items()})
        task = _lib.IkTask(nsite=K, dofs=mask)
        for k in range(K):
            task.sites[k], task.pos_weight[k], task.rot_weight[k] = site_ids[k], float(wp[k]), float(wr[k])
        ins = _lib.IkIn(target_pos.data_ptr(), None if target_quat is None else target_quat.data_ptr(),
                        None if qpos0 is None else qpos0.data_ptr(), lam.data_ptr())
        opt = _lib.IkOpt(iters, tol_pos, tol_rot, max_step, 1 if limits else 0)
        if M == 0:
            return res
        self._call_envs("rsr_physics_ik", who, ids, C.byref(task), C.byref(ins), C.byref(opt), C.byref(ptrs), checked=True,
                        hold=(target_pos, target_quat, qpos0, lam))
        return res

    def forward(self) -> None:
        """mjx.forward on every env: refreshes xpos, xquat, site_xpos, qacc (and qacc_warmstart), actuator_force and the contacts
        from the record's qpos / qvel / ctrl / qacc_warmstart."""
        _lib.check(_lib.lib().rsr_physics_forward(self._h, self._stream()))

    def step(self, ctrl=None, nsteps: Optional[int] = None) -> None:
        """Writes `ctrl` [num_envs, nu] (None: keep the record's) and runs `nsteps` (default n_substeps) x mjx.step."""
        import torch
        nsteps = self._steps("step", nsteps)
        ptr = None
        if ctrl is not None:
            c = torch.as_tensor(ctrl, dtype=torch.float32, device=self.device)
            if c.shape != (self.num_envs, self.dims.nu):
                raise ValueError(f"step expects ctrl of shape ({self.num_envs}, {self.dims.nu}), got {tuple(c.shape)}")
            c = c.contiguous()
            self._held["step"] = (c,)
            ptr = C.c_void_p(c.data_ptr())
        _lib.check(_lib.lib().rsr_physics_step(self._h, ptr, nsteps, self._stream()))

    def set_state(self, qpos=None, qvel=None, ctrl=None, env_ids=None) -> None:
        """mjx_env.init: writes the given fields of the envs `env_ids` (default: all; rows in env_ids order), zeroes their
        qacc_warmstart (and their applied forces, when on) and runs mjx.forward on those envs only.  The other envs' record and physics outputs are not touched."""
        import torch
        ids = self._ids(env_ids, "set_state")
        k = ids.numel()
        if k == 0:
            return
        vals = {}
        for name, x, width in (("qpos", qpos, self.dims.nq), ("qvel", qvel, self.dims.nv), ("ctrl", ctrl, self.dims.nu)):
            if x is None:
                continue
            t = torch.as_tensor(x, dtype=torch.float32, device=self.device)
            if t.shape != (k, width):
                raise ValueError(f"set_state expects {name} of shape ({k}, {width}), got {tuple(t.shape)}")
            vals[name] = t
        rec = {"qpos": self.qpos, "qvel": self.qvel, "ctrl": self.ctrl}
        for name, t in vals.items():
            rec[name][ids] = t
        self.qacc_warmstart[ids] = 0.0
        if self.xfrc_applied is not None:           # a fresh Data (mjx_env.init) has no applied forces
            self.xfrc_applied[ids] = 0.0
            self.qfrc_applied[ids] = 0.0
        if env_ids is None:
            self.forward()
        else:
            self._call_envs("rsr_physics_forward_envs", "set_state", ids, checked=True)

    def contacts(self) -> Dict[str, Any]:
        """Active contacts of the last forward pass, per env: ncon [N] and ncon_dropped [N] (int), and per contact slot
        (ncon_max of them; slots >= ncon are zeros with geoms -1): dist [N, K], pos [N, K, 3], normal [N, K, 3] (views),
        geom1 / geom2 [N, K] (int)."""
        import torch
        c = self._side["contact"].unflatten(1, (self.ncon_max, 9))
        return dict(ncon=self._side["ncon"][:, 0].to(torch.int32), ncon_dropped=self._side["ncon_dropped"][:, 0].to(torch.int32),
                    dist=c[:, :, 0], pos=c[:, :, 1:4], normal=c[:, :, 4:7],
                    geom1=c[:, :, 7].to(torch.int32), geom2=c[:, :, 8].to(torch.int32))
