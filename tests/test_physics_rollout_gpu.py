"""Batched rollouts and site sensors (rsr_physics_rollout / rsr_physics_set_sensors, Physics.rollout / set_sensors) on every built
family: a rollout is T physics steps bit for bit, the IMU sensors are the env's own privileged_state values, the frame sensors
match an fp64 host restatement, and the masks and argument checks hold."""
import ctypes as C

import numpy as np
import pytest

from physics_support import ALL, FAMILIES, GO2_EXTRA, PIPE, assert_bitwise, handle_views, make, pair, sensor_spec
from rsr_mjx_amd import prng


def _ctrl(envdef, A, rng, T):
    arr = envdef.sys.arrays["actuator_ctrlrange"]
    lo, hi = arr[:, 0], arr[:, 1]
    return (lo + (hi - lo) * rng.uniform(size=(A.num_envs, T, A.dims.nu))).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_rollout_is_repeated_step_bit_for_bit(kind):
    import torch
    from rsr_mjx_amd.physics import Physics
    n, T = 1024, 16
    envdef, A, B, scale, rng = pair(kind, n)
    spec = sensor_spec(kind, envdef)
    pa, pb = Physics(A, sensors=spec), Physics(B, sensors=spec)
    ctrl = torch.as_tensor(_ctrl(envdef, A, rng, T), device=A.device)
    keep = {k: B.view(k).clone() for k in ("obs", "reward", "done", "metrics", "first_qpos", "info_go2", "stats", "privileged_obs")}
    ref = {f: [] for f in ALL}
    for t in range(T):
        pa.step(ctrl[:, t], pa.n_substeps)
        ref["qpos"].append(pa.qpos.clone()); ref["qvel"].append(pa.qvel.clone()); ref["time"].append(pa.time[:, None].clone())
        ref["actuator_force"].append(pa.actuator_force.clone()); ref["ncon"].append(handle_views(pa, "side")["ncon"].clone())
        ref["sensordata"].append(pa.sensordata.clone())
    out = pb.rollout(ctrl, fields=ALL)
    torch.cuda.synchronize()
    assert pb.nsensordata == sum({"framequat": 4}.get(s[1], 3) for s in spec)
    for f in ALL:
        assert_bitwise(f"{kind} rollout {f}", out[f], torch.stack(ref[f], 1))
    for k in PIPE:
        assert_bitwise(f"{kind} record {k}", B.view(k), A.view(k))
    for k in ("qacc", "actuator_force", "xquat", "ncon", "contact", "ncon_dropped", "sensordata"):
        assert_bitwise(f"{kind} side {k}", handle_views(pb, "side")[k], handle_views(pa, "side")[k])
    for k, v in keep.items():                    # the env's bookkeeping is left alone
        assert_bitwise(f"{kind} untouched {k}", B.view(k), v)
    assert_bitwise(f"{kind} whole record", B.record, A.record)
    # env.step continues from the state the rollout left
    act = np.clip(rng.normal(size=(n, A.dims.nu)) * scale, -1, 1).astype(np.float32)
    A.step(None, act)
    B.step(None, act)
    torch.cuda.synchronize()
    assert_bitwise(f"{kind} env.step after rollout", B.record, A.record)


# privileged_state columns (go2/joystick.py:341-366): gyro, accelerometer, (gravity), local linvel, global angvel, ..., feet
# global linvel (FR, FL, RR, RL)
_PRIV = {"gyro": 48, "accelerometer": 51, "local_linvel": 57, "global_angvel": 60,
         "FR_global_linvel": 103, "FL_global_linvel": 106, "RR_global_linvel": 109, "RL_global_linvel": 112}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["go2flat", "go2rough"])
def test_sensors_are_the_envs_own_values(kind):
    """Teacher-forced as in test_physics_step_is_bit_identical_to_env_step: a T = 1 rollout with the env's ctrl from the env's
    state.  The sensor stage shares the env's arithmetic (go2_sensors' expressions for gyro / velocimeter, go2_accelerometer for
    the IMU, the site velocities themselves for the frame velocities), so all of these are compared bit for bit."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 1024
    envdef, A, B, scale, rng = pair(kind, n)
    A.step(None, np.clip(rng.normal(size=(n, A.dims.nu)) * scale, -1, 1).astype(np.float32))
    ctrl1 = A.view("ctrl").clone()
    phys = Physics(B, sensors=envdef.sensors)
    out = phys.rollout(ctrl1[:, None, :], nsteps=phys.n_substeps, fields=("sensordata", "qpos"))
    torch.cuda.synchronize()
    assert_bitwise(f"{kind} qpos", out["qpos"][:, 0], A.view("qpos"))
    priv = A.view("privileged_obs")
    for name, col in _PRIV.items():
        assert_bitwise(f"{kind} {name}", phys.sensor(name, out["sensordata"])[:, 0], priv[:, col:col + 3])
    assert_bitwise(f"{kind} current sensordata", phys.sensordata, out["sensordata"][:, 0])


def _quat2mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _site_frames(sys, qpos, qvel):
    """fp64 site positions, frames, quaternions and world velocities (object velocity at the site)."""
    from rsr_mjx_amd import mjcf
    A = sys.arrays
    kin = mjcf.forward_kinematics(sys, qpos)
    res = []
    for sid in range(sys.nsite):
        b = int(A["site_bodyid"][sid])
        q = mjcf.quat_mul(kin["xquat"][b], A["site_quat"][sid])
        R = _quat2mat(q / np.linalg.norm(q))
        p = kin["xpos"][b] + kin["xmat"][b] @ A["site_pos"][sid]
        jp, jr = mjcf.body_jacobian(sys, kin, p, b)
        res.append(dict(p=p, R=R, q=q, v=jp @ qvel, w=jr @ qvel))
    return res


def _expected(sys, spec, fr):
    vals = []
    for item in spec:
        typ, site = item[1], sys.id("site", item[2])
        f = fr[site]
        if typ == "framepos":
            if len(item) == 4:
                r = fr[sys.id("site", item[3])]
                vals.append(r["R"].T @ (f["p"] - r["p"]))
            else:
                vals.append(f["p"])
        elif typ == "framexaxis":
            vals.append(f["R"][:, 0])
        elif typ == "framezaxis":
            vals.append(f["R"][:, 2])
        elif typ == "framequat":
            vals.append(f["q"])
        elif typ == "framelinvel":
            vals.append(f["v"])
        elif typ == "frameangvel":
            vals.append(f["w"])
        elif typ == "gyro":
            vals.append(f["R"].T @ f["w"])
        elif typ == "velocimeter":
            vals.append(f["R"].T @ f["v"])
        else:
            vals.append(np.full(3, np.nan))       # accelerometer: covered by test_sensors_are_the_envs_own_values
    return np.concatenate(vals)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["go2flat", "cube", "tshape"])
def test_frame_sensors_against_fp64(kind):
    """nsteps = 1: the sensors of row t belong to the state of row t - 1 (the initial state for t = 0).  Positions, axes and
    quaternions within 1e-5 absolute; velocities within 1e-4 * max(1, |x|) (fp32 kinematics of a 13-body chain)."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n, T = 1024, 4
    envdef, A, _, scale = make(kind, n, False)
    A.reset(prng.split(prng.PRNGKey(21), n))
    rng = np.random.default_rng(21)
    for _ in range(2):
        A.step(None, np.clip(rng.normal(size=(n, A.dims.nu)) * scale, -1, 1).astype(np.float32))
    spec = [s for s in (envdef.sensors + GO2_EXTRA if kind == "go2flat" else sensor_spec(kind, envdef)) if s[1] != "accelerometer"]
    phys = Physics(A, sensors=spec)
    q0, v0 = phys.qpos.clone(), phys.qvel.clone()
    out = phys.rollout(torch.as_tensor(_ctrl(envdef, A, rng, T), device=A.device), nsteps=1, fields=("qpos", "qvel", "sensordata"))
    torch.cuda.synchronize()
    qpos = torch.cat([q0[:, None], out["qpos"][:, :-1]], 1).cpu().numpy().astype(np.float64)
    qvel = torch.cat([v0[:, None], out["qvel"][:, :-1]], 1).cpu().numpy().astype(np.float64)
    sd = out["sensordata"].cpu().numpy().astype(np.float64)
    kinds = np.concatenate([[s[1]] * {"framequat": 4}.get(s[1], 3) for s in spec])
    vel = np.isin(kinds, ["framelinvel", "frameangvel", "gyro", "velocimeter"])
    worst_pos, worst_vel = 0.0, 0.0
    for e in range(0, n, 64):
        for t in range(T):
            exp = _expected(envdef.sys, spec, _site_frames(envdef.sys, qpos[e, t], qvel[e, t]))
            d = np.abs(sd[e, t] - exp)
            worst_pos = max(worst_pos, float(d[~vel].max()))
            worst_vel = max(worst_vel, float((d[vel] / np.maximum(1.0, np.abs(exp[vel]))).max()))
    print(kind, f"frame sensors vs fp64: pos/axes/quat max abs {worst_pos:.2e}, velocities max rel {worst_vel:.2e}")
    assert worst_pos <= 1e-5 and worst_vel <= 1e-4, (worst_pos, worst_vel)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_masks_and_errors(kind):
    import torch
    from rsr_mjx_amd import _lib
    from rsr_mjx_amd.physics import Physics
    n, T = 1024, 5
    envdef, A, B, scale, rng = pair(kind, n)
    _, Cb, _, _ = make(kind, n, kind != "tshape")
    Cb.record.copy_(A.record)
    spec = sensor_spec(kind, envdef)
    ctrl = torch.as_tensor(_ctrl(envdef, A, rng, T), device=A.device)
    pa, pb, pc = Physics(A, sensors=spec), Physics(B, sensors=spec), Physics(Cb)
    # fields left NULL are not written: sentinels survive; a subset records what recording everything records
    d = A.dims
    width = dict(qpos=d.nq, qvel=d.nv, time=1, actuator_force=d.nu, ncon=1, sensordata=pa.nsensordata)
    sentinel = {f: torch.full((n, T, w), -7.25, device=A.device) for f, w in width.items()}
    full = pa.rollout(ctrl, fields=ALL)
    sub = pb.rollout(ctrl, fields=("qvel", "sensordata"), out={"qvel": sentinel["qvel"], "sensordata": sentinel["sensordata"]})
    torch.cuda.synchronize()
    assert sub["qvel"] is sentinel["qvel"]
    assert_bitwise("subset qvel", sub["qvel"], full["qvel"])
    assert_bitwise("subset sensordata", sub["sensordata"], full["sensordata"])
    for f in ("qpos", "time", "actuator_force", "ncon"):
        assert (sentinel[f] == -7.25).all(), f
    assert_bitwise("subset record", B.record, A.record)
    # with no sensors set, a step leaves exactly what it leaves with sensors set (but for sensordata)
    c1 = ctrl[:, 0]
    Cb.record.copy_(A.record)
    pa.step(c1)
    pc.step(c1)
    torch.cuda.synchronize()
    assert_bitwise("no-sensor step record", Cb.record, A.record)
    for k in ("qacc", "actuator_force", "xquat", "ncon", "contact", "ncon_dropped"):
        assert_bitwise(f"no-sensor step side {k}", handle_views(pc, "side")[k], handle_views(pa, "side")[k])
    assert pc.nsensordata == 0 and pc.sensordata.shape == (n, 0)
    # clearing the table
    pb.set_sensors(None)
    assert pb.nsensordata == 0
    with pytest.raises(ValueError):
        pb.rollout(ctrl, fields=("sensordata",))
    # argument errors, Python side
    with pytest.raises(ValueError):
        pa.rollout(ctrl[:, :, :-1])
    with pytest.raises(ValueError):
        pa.rollout(ctrl[:1])
    with pytest.raises(ValueError):
        pa.rollout(ctrl, nsteps=0)
    with pytest.raises(ValueError):
        pa.rollout(ctrl, fields=("qacc",))
    with pytest.raises(ValueError):
        pa.rollout(ctrl, fields=("qpos",), out={"qpos": torch.empty((n, T + 1, d.nq), device=A.device)})
    with pytest.raises(ValueError):
        pa.set_sensors([("x", "gyro", "no_such_site")])
    # and the library's own checks
    L = _lib.lib()
    cp = C.c_void_p(ctrl.data_ptr())
    o = _lib.RolloutOut()
    o.sensordata = sentinel["sensordata"].data_ptr()
    assert L.rsr_physics_rollout(pc._h, cp, T, 1, C.byref(o), None) == -1           # sensordata without a table
    assert L.rsr_physics_rollout(pa._h, cp, 0, 1, None, None) == -1
    assert L.rsr_physics_rollout(pa._h, cp, T, 0, None, None) == -1
    assert L.rsr_physics_rollout(pa._h, None, T, 1, None, None) == -1
    bad = lambda rows: (C.c_int32 * (4 * len(rows)))(*[v for r in rows for v in r])
    nsite = envdef.sys.nsite
    assert L.rsr_physics_set_sensors(pa._h, bad([(0, nsite, -1, 0)]), 1) == -1                  # site out of range
    assert L.rsr_physics_set_sensors(pa._h, bad([(9, 0, -1, 0)]), 1) == -1                      # unknown type
    assert L.rsr_physics_set_sensors(pa._h, bad([(0, 0, 0, 0)]), 1) == -1                       # ref on a gyro
    assert L.rsr_physics_set_sensors(pa._h, bad([(0, 0, -1, 1)]), 1) == -1                      # address gap
    assert L.rsr_physics_set_sensors(pa._h, bad([(6, 0, -1, 4 * i) for i in range(17)]), 17) == -1   # 68 floats
    # an accelerometer off the tracked body (Airbot: there is none; Go2: a foot) is RSR_ERR_UNSUPPORTED
    foot = envdef.sys.id("site", "FR") if kind == "go2flat" else 0
    assert L.rsr_physics_set_sensors(pa._h, bad([(2, foot, -1, 0)]), 1) == -2
    torch.cuda.synchronize()
    assert pa.nsensordata == sum({"framequat": 4}.get(s[1], 3) for s in spec)   # a refused table leaves the old one
