"""Rollout and sensor API (rsr_physics_rollout / rsr_physics_set_sensors, rsr_mjx_amd/sensors.py), host side only: the header,
the exports, the argument checks that come before any device work, and the spec -> table conversion.  The kernels are covered
by tests/test_physics_rollout_gpu.py."""
import ctypes as C
import re

import numpy as np
import pytest

from api_support import header


def test_header_declares_rollout_and_sensors():
    h = header()
    for sig in ("int rsr_physics_set_sensors(rsr_physics* p, const int32_t* table, int nsensor);",
                "int rsr_physics_rollout(rsr_physics* p, const float* ctrl, int T, int nsteps, const rsr_rollout_out* out, void* hip_stream);"):
        assert sig in h, sig
    from rsr_mjx_amd import _lib
    body = re.search(r"typedef struct rsr_rollout_out \{([^}]*)\}", h).group(1)
    assert re.findall(r"float\* (\w+);", body) == [f for f, _ in _lib.RolloutOut._fields_]
    enum = re.search(r"enum rsr_sensor_type \{([^}]*)\}", h).group(1)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    assert names == ["RSR_S_" + t.upper() for t in _lib.SENSOR_TYPES] + ["RSR_S_COUNT"]
    assert "#define RSR_MAX_SENSORDATA 64" in h and _lib.MAX_SENSORDATA == 64
    assert _lib.PHYS_FIELDS[-1] == "sensordata" and _lib.PHYS_FIELDS.index("sensordata") == 6


def test_library_exports_and_checks_before_device_work():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    for sym in ("rsr_physics_set_sensors", "rsr_physics_rollout"):
        assert sym in _lib.PHYS_SYMBOLS and getattr(L, sym) is not None
    table = (C.c_int32 * 4)(0, 0, -1, 0)
    assert L.rsr_physics_set_sensors(None, table, 1) == -1
    assert b"null" in L.rsr_last_error()
    assert L.rsr_physics_set_sensors(None, None, 0) == -1
    ctrl = C.c_void_p(16)                     # never dereferenced: the handle check fails first
    out = _lib.RolloutOut()
    assert L.rsr_physics_rollout(None, ctrl, 4, 1, C.byref(out), None) == -1
    assert L.rsr_physics_rollout(None, None, 4, 1, None, None) == -1
    assert b"null" in L.rsr_last_error()


def test_oversize_and_bad_tables_are_refused_on_the_host():
    """A fake handle is never needed: the table checks come before the handle's model is read -- except the ones that need the
    model, which tests/test_physics_rollout_gpu.py exercises on a real handle."""
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    big = (C.c_int32 * (4 * 65))()
    assert L.rsr_physics_set_sensors(None, big, 65) == -1
    assert L.rsr_physics_set_sensors(None, big, -1) == -1


def _go2(name="Go2JoystickFlatTerrain"):
    from rsr_mjx_amd.envs import go2
    return go2.load(name)


def test_spec_to_table_addresses_and_widths():
    from rsr_mjx_amd import _lib, sensors
    env = _go2()
    sys = env.sys
    imu = sys.id("site", "imu")
    table, where = sensors.sensor_table(sys, env.sensors, imu)
    assert table.dtype == np.int32 and table.shape == (17, 4)
    widths = [_lib.SENSOR_WIDTH[s[1]] for s in env.sensors]
    np.testing.assert_array_equal(table[:, 3], np.concatenate([[0], np.cumsum(widths)[:-1]]))
    assert where["orientation"] == (24, 4) and where["FR_global_linvel"] == (28, 3) and where["RL_pos"] == (49, 3)
    row = table[list(where).index("FR_pos")]
    assert tuple(row[:3]) == (_lib.SENSOR_TYPES.index("framepos"), sys.id("site", "FR"), imu)
    assert (table[:, 2][[i for i, s in enumerate(env.sensors) if len(s) == 3]] == -1).all()
    # site ids are accepted as well as names
    t2, _ = sensors.sensor_table(sys, [("a", "gyro", imu)], imu)
    assert tuple(t2[0]) == (0, imu, -1, 0)


@pytest.mark.parametrize("spec, msg", [
    ([("x", "gyro", "no_such_site")], "unknown site"),
    ([("x", "touch", "imu")], "unknown type"),
    ([("x", "gyro", "imu", "FR")], "reference site"),
    ([("x", "framepos", "imu", "nowhere")], "unknown site"),
    ([("x", "accelerometer", "FR")], "accelerometer"),
    ([("x", "gyro", "imu"), ("x", "gyro", "FR")], "twice"),
    ([(f"q{i}", "framequat", "imu") for i in range(17)], "at most 64"),
])
def test_spec_errors(spec, msg):
    from rsr_mjx_amd import sensors
    sys = _go2().sys
    with pytest.raises(ValueError, match=msg):
        sensors.sensor_table(sys, spec, sys.id("site", "imu"))


def test_accelerometer_needs_the_imu_body():
    from rsr_mjx_amd import sensors
    from rsr_mjx_amd.envs import airbot
    sys = _go2().sys
    sensors.sensor_table(sys, [("acc", "accelerometer", "imu")], sys.id("site", "imu"))
    with pytest.raises(ValueError, match="accelerometer"):                 # a model without a tracked body
        sensors.sensor_table(sys, [("acc", "accelerometer", "imu")], None)
    cube = airbot.AirbotPlayBase()
    with pytest.raises(ValueError, match="accelerometer"):
        sensors.sensor_table(cube.sys, [("acc", "accelerometer", "endpoint")], None)


def test_default_sensor_lists():
    from rsr_mjx_amd import sensors
    from rsr_mjx_amd.envs import airbot, go2
    for name, n in (("Go2JoystickFlatTerrain", 52), ("Go2JoystickRoughTerrain", 52), ("Go2Handstand", 55), ("Go2Footstand", 55)):
        env = go2.load(name)
        assert sensors.nsensordata(env.sensors) == n, name
        table, where = sensors.sensor_table(env.sys, env.sensors, env.sys.id("site", "imu"))
        assert table[-1, 3] + 3 == n
        assert ("head_pos" in where) == (n == 55)
    for env in (airbot.AirbotPlayBase(), airbot.AirbotPlaySF(), airbot.AirbotTShape()):
        table, where = sensors.sensor_table(env.sys, env.sensors, None)
        assert list(where) == ["endpoint_pos", "endpoint_linvel"] and sensors.nsensordata(env.sensors) == 6


def test_physics_module_surface():
    from rsr_mjx_amd.physics import ROLLOUT_FIELDS, Physics
    for m in ("rollout", "set_sensors", "sensor"):
        assert callable(getattr(Physics, m))
    assert ROLLOUT_FIELDS == ("qpos", "qvel", "time", "actuator_force", "ncon", "sensordata")
