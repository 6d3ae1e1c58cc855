"""What the host-side API tests (tests/test_*_api.py, tests/test_physics_calls.py) and tools/physics_wrapper_overhead.py share: the
readers of the header and the sources, a Physics without a handle, and a library that records its calls instead of making them."""
import ctypes as C
import os
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rsr_mjx_amd", "csrc")
HANDLE, STREAM = 0x5150, 0x57                   # placeholders: what a recorded call shows as its handle and its stream
SITES = {"base": 0, "elbow": 1, "tip": 2, "tool": 3}


def header():
    return open(os.path.join(ROOT, "include", "rsr_physics.h")).read()


def read(*parts):
    """a source under rsr_mjx_amd/csrc"""
    return open(os.path.join(CSRC, *parts)).read()


def body(src, name):
    """the definition of `name` in `src`, up to its closing brace"""
    b = src[src.index(name + "("):]
    return b[:b.index("\n}\n")]


def standin(handle=HANDLE, nsensordata=0, num_envs=4, **dims):
    """A Physics without a library handle, for everything its methods do ahead of the C call: `num_envs` envs, small dims (any of
    them overridable), record tensors on the CPU, `nsensordata` columns of sensordata, and of the env a stream and a model with
    the sites SITES, a hinge (dof 0), a slide (dof 1) and a free joint.  handle=None: the real library refuses a call as
    "null handle", which shows that the call's arguments convert."""
    import numpy as np
    import torch
    from rsr_mjx_amd.physics import Physics
    p = Physics.__new__(Physics)
    d = p.dims = types.SimpleNamespace(**{**dict(nu=3, nq=6, nv=5, nsite=4, nbody=3, ngeom=6, env_kind=0, n_frames=2, ncon_max=4), **dims})
    p._h = None if handle is None else C.c_void_p(handle)
    p.num_envs, p.device = num_envs, torch.device("cpu")
    z = lambda w: torch.zeros((num_envs, w))
    p.qpos, p.qvel, p.ctrl, p.qacc_warmstart, p.sensordata = z(d.nq), z(d.nv), z(d.nu), z(d.nv), z(nsensordata)
    p.xfrc_applied = p.qfrc_applied = p._dyn = None
    p._held = {}

    def site_id(kind, name):
        return SITES[name]
    sys = types.SimpleNamespace(id=site_id, arrays=dict(jnt_type=np.array([3, 2, 0]), jnt_dofadr=np.array([0, 1, 2])))
    p.env = types.SimpleNamespace(_stream=lambda: C.c_void_p(STREAM), sys=sys)
    return p


class Recorder:
    """Stands for the loaded library: every symbol is a function that records (symbol, decoded arguments) and returns 0.  A
    c_void_p is decoded to its value (None: null) and a C.byref(struct) to the struct.  peek: {symbol: f(*decoded arguments)},
    run during the call, for memory that does not outlive it; the results collect in `peeked`."""

    def __init__(self, peek=None):
        self.calls, self.peek, self.peeked = [], dict(peek or {}), []

    def __getattr__(self, symbol):
        def fn(*args):
            args = tuple(a.value if isinstance(a, C.c_void_p) else getattr(a, "_obj", a) for a in args)
            self.calls.append((symbol, args))
            if symbol in self.peek:
                self.peeked.append(self.peek[symbol](*args))
            return 0
        return fn


def record(monkeypatch, peek=None):
    """installs a Recorder over _lib.lib and returns it"""
    from rsr_mjx_amd import _lib
    rec = Recorder(peek)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def fields(struct):
    """a ctypes struct as {member: value}, arrays as lists"""
    return {n: (list(v) if isinstance(v, C.Array) else v) for n, v in ((n, getattr(struct, n)) for n, _ in struct._fields_)}


def ints(ptr, n):
    return list((C.c_int32 * n).from_address(ptr))


def floats(ptr, n):
    return list((C.c_float * n).from_address(ptr))


def refused(monkeypatch, method, cases):
    """every (kwargs, message) of `cases` raises ValueError matching the message, and the library sees no call"""
    import pytest
    with monkeypatch.context() as m:
        rec = record(m)
        for kw, msg in cases:
            with pytest.raises(ValueError, match=msg):
                method(**kw)
        assert rec.calls == [], rec.calls
