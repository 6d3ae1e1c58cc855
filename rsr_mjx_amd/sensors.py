"""Site sensors of the physics layer (rsr_physics_set_sensors, include/rsr_physics.h): spec -> table conversion and the default
sensor lists of the built envs.

A spec is a list of (name, type, site, ref_site=None): sites by name (the model's name table), types as in _lib.SENSOR_TYPES.
data.sensordata concatenates the sensors in spec order, as MuJoCo lays out sensor_adr.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

Spec = Sequence[tuple]

# The <sensor> block of the Go2 models the joystick envs compile from (feet-only collisions: flat and rough terrain), 52 floats:
# the IMU's body-frame gyro / velocimeter / accelerometer, its world position, up (z) and forward (x) axes, world velocities and
# orientation, then each foot's world velocity and its position in the IMU frame.
GO2_JOYSTICK_SENSORS: List[tuple] = [
    ("gyro", "gyro", "imu"),
    ("local_linvel", "velocimeter", "imu"),
    ("accelerometer", "accelerometer", "imu"),
    ("position", "framepos", "imu"),
    ("upvector", "framezaxis", "imu"),
    ("forwardvector", "framexaxis", "imu"),
    ("global_linvel", "framelinvel", "imu"),
    ("global_angvel", "frameangvel", "imu"),
    ("orientation", "framequat", "imu"),
] + [(f"{f}_global_linvel", "framelinvel", f) for f in ("FR", "FL", "RR", "RL")] \
  + [(f"{f}_pos", "framepos", f, "imu") for f in ("FR", "FL", "RR", "RL")]

# The full-collision Go2 model of handstand / footstand: the same list plus the head site's world position, 55 floats.
GO2_FULL_SENSORS: List[tuple] = GO2_JOYSTICK_SENSORS + [("head_pos", "framepos", "head")]

# The Airbot models declare no sensors; an example list on the gripper's endpoint site.
AIRBOT_ENDPOINT_SENSORS: List[tuple] = [
    ("endpoint_pos", "framepos", "endpoint"),
    ("endpoint_linvel", "framelinvel", "endpoint"),
]


def _site(sys, name) -> int:
    if isinstance(name, (int, np.integer)):
        sid = int(name)
        if not 0 <= sid < sys.nsite:
            raise ValueError(f"site id {sid} out of range [0, {sys.nsite})")
        return sid
    try:
        return sys.id("site", name)
    except KeyError:
        raise ValueError(f"unknown site {name!r}; the model's sites: {sorted(sys.names['site'])}") from None


def sensor_table(sys, spec: Spec, accel_site: Optional[int] = None) -> Tuple[np.ndarray, Dict[str, Tuple[int, int]]]:
    """(table int32 [nsensor, 4] of rows (type, site, ref site or -1, address), {name: (address, width)}).

    accel_site: the site whose body's acceleration the kernels track (the Go2 IMU), or None where the model has none.  An
    accelerometer must sit on that body; raises ValueError on anything the library would refuse."""
    rows, where, adr = [], {}, 0
    acc = None
    for item in spec:
        if len(item) not in (3, 4):
            raise ValueError(f"sensor spec entries are (name, type, site[, ref_site]), got {item!r}")
        name, typ, site = item[0], item[1], item[2]
        ref = item[3] if len(item) == 4 else None
        if name in where:
            raise ValueError(f"sensor {name!r} given twice")
        if typ not in _lib.SENSOR_WIDTH:
            raise ValueError(f"sensor {name!r}: unknown type {typ!r}; supported: {_lib.SENSOR_TYPES}")
        sid = _site(sys, site)
        rid = -1
        if ref is not None:
            if typ != "framepos":
                raise ValueError(f"sensor {name!r}: only framepos takes a reference site")
            rid = _site(sys, ref)
        if typ == "accelerometer":
            bodies = sys.arrays["site_bodyid"]
            if accel_site is None or bodies[sid] != bodies[accel_site]:
                raise ValueError(f"sensor {name!r}: an accelerometer must sit on the body of the IMU site (the only body whose "
                                 "acceleration the kernels track; Go2 models only)")
            if acc is not None and acc != sid:
                raise ValueError(f"sensor {name!r}: accelerometers on more than one site")
            acc = sid
        w = _lib.SENSOR_WIDTH[typ]
        rows.append((_lib.SENSOR_TYPES.index(typ), sid, rid, adr))
        where[name] = (adr, w)
        adr += w
    if adr > _lib.MAX_SENSORDATA:
        raise ValueError(f"the sensors need {adr} floats; at most {_lib.MAX_SENSORDATA}")
    return np.array(rows, dtype=np.int32).reshape(-1, 4), where


def nsensordata(spec: Spec) -> int:
    return sum(_lib.SENSOR_WIDTH[item[1]] for item in spec)
