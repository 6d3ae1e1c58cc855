"""Physics-level access to an env batch: the two calls every reference env is written against (_src/mjx_env.py:30-73).

    mjx_env.init(model, qpos, qvel, ctrl)      ->  Physics.set_state(qpos, qvel, ctrl)   (one mjx.forward)
    mjx_env.step(model, data, ctrl, n_substeps) ->  Physics.step(ctrl, nsteps)           (nsteps x mjx.step)

`Physics(env)` shares the batch of a BatchedEnv (Airbot cube / sf / T-shape, Go2 joystick, handstand / footstand): the same model,
the same per-env domain randomisation, the same record and the same stream.  The pipeline fields it exposes are the record's own
views, so a following `env.step` continues from whatever state these calls leave (rsr_physics_step / rsr_physics_forward,
include/rsr_physics.h).  As in MJX's Data, the position-dependent outputs (xpos, xquat, site_xpos, contacts) after a step are those
of the last forward pass, before the final integration.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional

from . import _lib


class _DevArray:
    """__cuda_array_interface__ of a strided float32 region of library-owned device memory (the physics side buffer)."""

    def __init__(self, ptr: int, shape, strides_elems):
        self.__cuda_array_interface__ = dict(shape=tuple(int(s) for s in shape), typestr="<f4", data=(int(ptr), False), version=2,
                                             strides=tuple(4 * int(s) for s in strides_elems))


class Physics:
    """Physics-only stepping, forward and state setting on the envs of `env` (a BatchedEnv)."""

    def __init__(self, env):
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
        side = {}
        for fid, name in enumerate(_lib.PHYS_FIELDS):
            ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
            _lib.check(_lib.lib().rsr_physics_view(self._h, fid, C.byref(ptr), shape, stride))
            side[name] = torch.as_tensor(_DevArray(ptr.value, (shape[0], shape[1]), (stride[0], stride[1])), device=self.device)
        self._side = side
        self.qacc = side["qacc"]
        self.actuator_force = side["actuator_force"]
        self.xquat = side["xquat"].unflatten(1, (d.nbody, 4))

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

    def forward(self) -> None:
        """mjx.forward on every env: refreshes xpos, xquat, site_xpos, qacc (and qacc_warmstart), actuator_force and the contacts
        from the record's qpos / qvel / ctrl / qacc_warmstart."""
        _lib.check(_lib.lib().rsr_physics_forward(self._h, self._stream()))

    def step(self, ctrl=None, nsteps: Optional[int] = None) -> None:
        """Writes `ctrl` [num_envs, nu] (None: keep the record's) and runs `nsteps` (default n_substeps) x mjx.step."""
        import torch
        nsteps = self.n_substeps if nsteps is None else int(nsteps)
        if nsteps < 1:
            raise ValueError(f"step: nsteps must be >= 1, got {nsteps}")
        ptr = None
        if ctrl is not None:
            c = torch.as_tensor(ctrl, dtype=torch.float32, device=self.device)
            if c.shape != (self.num_envs, self.dims.nu):
                raise ValueError(f"step expects ctrl of shape ({self.num_envs}, {self.dims.nu}), got {tuple(c.shape)}")
            c = c.contiguous()
            self._ctrl_in = c                      # kept alive until the next call (the launch is asynchronous)
            ptr = C.c_void_p(c.data_ptr())
        _lib.check(_lib.lib().rsr_physics_step(self._h, ptr, nsteps, self._stream()))

    def set_state(self, qpos=None, qvel=None, ctrl=None, env_ids=None) -> None:
        """mjx_env.init: writes the given fields of the envs `env_ids` (default: all; rows in env_ids order), zeroes their
        qacc_warmstart and runs mjx.forward on those envs only.  The other envs' record and physics outputs are not touched."""
        import torch
        if env_ids is None:
            ids = torch.arange(self.num_envs, device=self.device, dtype=torch.int64)
        else:
            ids = torch.as_tensor(env_ids, device=self.device).to(torch.int64).reshape(-1)
            if ids.numel() == 0:
                return
            if bool(((ids < 0) | (ids >= self.num_envs)).any()):
                raise ValueError(f"set_state: env_ids must lie in [0, {self.num_envs})")
            if torch.unique(ids).numel() != ids.numel():
                raise ValueError("set_state: env_ids must not repeat")
        k = ids.numel()
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
        if env_ids is None:
            self.forward()
        else:
            ids32 = ids.to(torch.int32).contiguous()
            self._ids_in = ids32
            _lib.check(_lib.lib().rsr_physics_forward_envs(self._h, C.c_void_p(ids32.data_ptr()), k, self._stream()))

    def contacts(self) -> Dict[str, Any]:
        """Active contacts of the last forward pass, per env: ncon [N] and ncon_dropped [N] (int), and per contact slot
        (ncon_max of them; slots >= ncon are zeros with geoms -1): dist [N, K], pos [N, K, 3], normal [N, K, 3] (views),
        geom1 / geom2 [N, K] (int)."""
        import torch
        c = self._side["contact"].unflatten(1, (self.ncon_max, 9))
        return dict(ncon=self._side["ncon"][:, 0].to(torch.int32), ncon_dropped=self._side["ncon_dropped"][:, 0].to(torch.int32),
                    dist=c[:, :, 0], pos=c[:, :, 1:4], normal=c[:, :, 4:7],
                    geom1=c[:, :, 7].to(torch.int32), geom2=c[:, :, 8].to(torch.int32))
