"""Transition Jacobians along a trajectory (rsr_physics_trajectory_fd, Physics.trajectory_fd), host side only: the ABI, the entry
point's refusals ahead of its first device call, the two kernels' header, and the Python surface with every bad input refused
before the C call.  The kernels are covered by tests/test_trajectory_fd_gpu.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_support import CSRC, ROOT, body as _body, header, ints, read as _read, record, refused, standin
SIG = ("int rsr_physics_trajectory_fd(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, int T, int nsteps, "
       "float eps, int flags, const rsr_trajectory_fd_out* out, void* hip_stream);")


def test_header_declares_the_call_and_the_struct():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat                                             # (the declaration may break its lines)
    assert "typedef struct rsr_trajectory_fd_out { float* columns; float* qpos; float* qvel; } rsr_trajectory_fd_out;" in flat
    doc = h[h.index("/* Transition Jacobians along a trajectory"):h.index("typedef struct rsr_trajectory_fd_out")]
    for word in ("[M, T, nu]", "[M, T+1, nq]", "[M, T+1, nv]", "[M, T, ncol, 2 nv + nsensordata]", "tight", "RSR_MAX_SENSORDATA",
                 "rsr_physics_sample_rollouts with K = 1", "rsr_physics_transition_fd(nsteps, eps, flags)", "rsr_physics_step(",
                 "warm start", "more than once", "RSR_FD_CENTERED", "RSR_FD_STATES", "read only", "untouched", "nominal scratch",
                 "M T (nq + 2 nv) floats", "waits for the device", "rsr_physics_destroy frees it", "must not overlap on different streams",
                 "left alone", "before any device work", "2^30", "2^31"):
        assert word in doc, word
    assert "rsr_physics_trajectory_fd <-" in h[:h.index("typedef")]                      # the opening list
    assert "rsr_trajectory_fd_out" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_trajectory_fd" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_trajectory_fd
    assert fn.argtypes is not None and len(fn.argtypes) == 10 and fn.argtypes[6] is C.c_float
    o = _lib.TrajectoryFdOut()
    assert [n for n, _ in _lib.TrajectoryFdOut._fields_] == ["columns", "qpos", "qvel"] and C.sizeof(o) == 3 * C.sizeof(C.c_void_p)
    assert not (o.columns or o.qpos or o.qvel)
    ids = (C.c_int32 * 2)(0, 1)
    ctrl = (C.c_float * 8)()
    for table, k in ((None, 0), (ids, 2)):
        for out in (None, C.byref(o)):
            assert fn(None, table, k, ctrl, 1, 1, 1e-3, 1, out, None) == -1
            assert b"rsr_physics_trajectory_fd: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every RSR_ERR_ARG check of the entry comes ahead of its first device call (by source order, as a handle needs a device):
    the scratch, then the two launches, each an op of its own with the one argument struct; the scratch grows on demand, waits
    for the device before it is replaced, and goes with the handle."""
    src = _read("physics", "rsr_physics.hip")
    call = _body(src, "int rsr_physics_trajectory_fd")
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "nominal_scratch(", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("nominal_scratch(")
    checks = ("!p)", "!ctrl)", "!out || !out->columns)", "T < 1", "nsteps < 1", "nsteps > INT32_MAX / 2", "std::isfinite(eps)", "eps > 0.0f",
              "flags & ~RSR_FD_CENTERED", "env_count(", "(int64_t)T * nsteps > INT32_MAX", "cells > INT32_MAX", "cells * FL.ncol > INT32_MAX")
    at = [call.index(c) for c in checks]
    assert all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.count("RSR_ERR_ARG") == 8 and call.rindex("RSR_ERR_ARG") < first_dev
    assert "count < 1" in _body(src, "static int env_count")
    assert "const int64_t cells = (int64_t)n * T;" in call and "(size_t)cells * (d.nq + 2 * d.nv)" in call
    # the two launches, in order, on the one Launch: the slots, then every (slot, t, column)
    assert re.findall(r"\bOP_\w+", call) == ["OP_TRAJ_NOMINAL", "OP_TRAJ_FD"] and call.count("physics_launch(") == 2
    assert call.index("physics_args(p, nullptr, env_ids, n, nsteps, hip_stream)") < call.index("x.ph.tj = rsr::TrajArgs{") \
        < call.index("rsr::OP_TRAJ_NOMINAL") < call.index("x.grid = (int)(cells * FL.ncol);") < call.index("rsr::OP_TRAJ_FD")
    assert sorted(set(re.findall(r"\bx\.ph\.(\w+)", call))) == ["tj"] and "counted(" not in call
    # the scratch: kept while it is large enough, replaced after a wait, freed with the handle; the zeroed-once buffers are as they were
    grow = _body(src, "static int nominal_scratch")
    assert grow.index("if (floats <= p->nominal_floats) return RSR_OK;") < min(grow.index(k) for k in dev if k in grow and k != "nominal_scratch(")
    assert grow.index("if (p->nominal) HIPCHK(hipDeviceSynchronize());") < grow.index("hipMalloc(") < grow.index("hipFree(p->nominal)") \
        < grow.index("p->nominal = buf;") < grow.index("p->nominal_floats = floats;")
    assert src.count("nominal_scratch(") == 2 and src.count("p->nominal = ") == 1
    assert "hipFree(p->nominal)" in _body(src, "void rsr_physics_destroy")
    assert "_alloc" not in src and src.count("static int zeroed_once(") == 1


def test_the_kernels_are_a_header_of_their_own():
    kern = _read("physics", "rsr_trajectory.hpp")
    code = re.sub(r"//.*", "", kern)
    assert "void nominal_kernel(" in code and "void trajectory_fd_kernel(" in code and '#include "rsr_transition.hpp"' in code
    nom, fd = code[code.index("void nominal_kernel("):code.index("void trajectory_fd_kernel(")], code[code.index("void trajectory_fd_kernel("):]
    for k in (nom, fd):
        assert k.count("forward<C>(") == 1 and k.count("integrate<C>(") == 1
        for w in ("force_stage<C>(e, ", "load_overrides<C>(m, s, a, e, ", "lrec_lane(lane)", "if constexpr (C::XFRC)", "p.ids ? p.ids[slot] : slot",
                  "if (e < 0 || e >= a.n) return;"):
            assert w in k, w
    for w in ("store_pipeline", "store_side", "asm", "atomic", "p.sd", "p.out"):
        assert w not in kern, w
    named = re.findall(r"\b(kinematics|com_crb_mass|load_mrow|smooth_forces|\w+_factor|\w+_solve|collision|make_constraint|solve)\b", code)
    assert not named, named
    # the nominal run: the record read only, no overlay or feedback stage, the scratch row before each control step
    assert "const float* rec = a.state + (size_t)e * L.rec;" in nom and not re.search(r"\brec\[[^\]]*\]\s*=[^=]", nom)
    assert "overlay_leaves" not in code and "feedback_ctrl" not in code and "sensor_stage" not in nom
    assert "const int total = tj.T * p.nsteps;" in nom and "tj.nominal + ((size_t)slot * tj.T + t) * nominal_row<C>()" in nom
    assert "(size_t)slot * (tj.T + 1) + t" in nom
    # the columns: transition_kernel's devices, the run's start from the scratch row, the record never read, tight rows
    assert "a.state" not in fd and "rec[" not in fd
    for w in ("perturb_state<C>(hot, s, ln, col, dl)", "differentiate_pos<C>(hot, s, lt, yq)", "fd_park_offset<C>()", "sensor_stage<C>(",
              "const int total = 2 * p.nsteps;", "asf(__builtin_bit_cast(int, dlt) + (ln - lane))", "tj.nominal + (size_t)cell * nominal_row<C>()",
              "tj.ctrl[(size_t)cell * C::NU + ln]", "tj.columns + (size_t)b * (2 * C::NV + nsd)", "if (lt < nsd) o[2 * C::NV + lt]"):
        assert w in fd, w
    assert len(re.findall(r"for \(int k = 0; k < total; \+\+k\)", fd)) == 1
    # the dispatch: ops of the physics enum with their struct a field of the launch's, instantiated plain and applied by the one
    # launch lambda, with the transition's LDS for the columns; no source directly under csrc/ knows
    phys = _read("physics", "rsr_physics.hpp")
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert re.findall(r"\bOP_TRAJ_\w+", enum) == ["OP_TRAJ_NOMINAL", "OP_TRAJ_FD"] and "struct TrajArgs" in phys
    assert re.search(r"\bTrajArgs tj;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    kernels = _read("physics", "rsr_physics_kernels.hpp")
    assert '#include "rsr_trajectory.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    assert "op == OP_TRAJ_FD || op == OP_PHYS_TRANSITION ? fd_lds_bytes<C>() : sizeof(Smem<C>)" in lp and lp.count("hipLaunchKernelGGL(") == 1
    for op, k in (("OP_TRAJ_NOMINAL", "nominal_kernel"), ("OP_TRAJ_FD", "trajectory_fd_kernel")):
        assert f"if (op == {op}) return ap ? go({k}<C, WAVES, Applied>, ph.p, ph.tj, ph.ap) : go({k}<C, WAVES>, ph.p, ph.tj);" in lp, op
        assert lp.count(k) == 2
    for f in ("rsr_transition.hpp", "rsr_sweep.hpp", "rsr_sample.hpp"):
        text = _read("physics", f)
        assert "trajectory_fd" not in text and "rsr_trajectory" not in text and "nominal_kernel" not in text and "OP_TRAJ_" not in text, f
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "trajectory_fd" not in text and "nominal_kernel" not in text and "OP_TRAJ_" not in text and "TrajArgs" not in text, f
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4l."):]
    for word in ("nominal_kernel", "trajectory_fd_kernel", "two launches", "nq + 2 nv", "VGPRs", "trajectory_fd_rates"):
        assert word in sec, word


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.trajectory_fd)
    assert list(sig.parameters) == ["self", "ctrl", "nsteps", "eps", "centered", "env_ids", "nominal", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "ctrl")}
    assert d == dict(nsteps=None, eps=1e-3, centered=True, env_ids=None, nominal=True, out=None)
    assert "Physics.trajectory_fd(ctrl [M, T, nu])" in physics.__doc__
    doc = Physics.trajectory_fd.__doc__
    for word in ("[M, T, 2nv, 2nv]", "[M, T, 2nv, nu]", "[M, T, nsensordata, 2nv]", "[M, T, nsensordata, nu]", "[M, T+1, nq]", "[M, T+1, nv]",
                 "fd_A .. fd_D", "sample_rollouts", "must not overlap"):
        assert word in doc, word
    # the sibling is as it was
    assert list(inspect.signature(Physics.transition_fd).parameters) == ["self", "env_ids", "nsteps", "eps", "centered", "keep_states"]
    # every bad input is refused before the C call: the recording library sees none
    nu, nq, nv, nsd = 3, 5, 4, 2
    p = standin(handle=None, nsensordata=nsd, nq=nq, nv=nv)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, T, ncol, w = 4, 3, 2 * nv + nu, 2 * nv + nsd
    good = dict(ctrl=z(M, T, nu))
    cases = [(dict(ctrl=z(M, nu)), "expects ctrl"),                                                     # rank
             (dict(ctrl=z(M, 1, T, nu)), "expects ctrl"),
             (dict(ctrl=z(M, T, nu + 1)), "expects ctrl"),                                              # nu
             (dict(ctrl=z(M, 0, nu)), "expects ctrl"),                                                  # T
             (dict(ctrl=z(M - 1, T, nu)), "expects ctrl"),                                              # M
             (dict(good, env_ids=[0, 2]), "expects ctrl"),
             (dict(ctrl=z(M, T, nu).double()), "expects ctrl"),                                         # dtype
             (dict(ctrl=z(M, T, nu, device="meta")), "expects ctrl"),                                   # device
             (dict(ctrl=z(M, T, nu).numpy()), "expects ctrl"),                                          # not a tensor
             (dict(good, env_ids=[0, 1, 2, 4]), "env_ids must lie in"),                                 # env_ids
             (dict(good, env_ids=[0, 1, -1, 2]), "env_ids must lie in"),
             (dict(good, nsteps=0), "nsteps must lie in"),                                              # nsteps
             (dict(good, nsteps=2 ** 30), "nsteps must lie in"),
             (dict(ctrl=z(M, 4, nu), nsteps=2 ** 29), "below 2\\^31"),
             (dict(good, eps=0.0), "eps must be finite"),                                               # eps
             (dict(good, eps=-1e-3), "eps must be finite"),
             (dict(good, eps=float("inf")), "eps must be finite"),
             (dict(good, eps=float("nan")), "eps must be finite"),
             (dict(good, out={"columns": z(M, T, ncol, w + 1)}), "out\\['columns'\\]"),                  # out
             (dict(good, out={"columns": z(M, T, ncol, 2 * nv + 64)}), "out\\['columns'\\]"),            # (tight rows, not padded ones)
             (dict(good, out={"columns": z(M, T, ncol, w).double()}), "out\\['columns'\\]"),
             (dict(good, out={"columns": z(M, T, w, ncol).transpose(2, 3)}), "out\\['columns'\\]"),
             (dict(good, out={"columns": z(M, T, ncol, w, device="meta")}), "out\\['columns'\\]"),
             (dict(good, out={"columns": z(M, T, ncol, w).numpy()}), "out\\['columns'\\]"),
             (dict(good, out={"qpos": z(M, T, nq)}), "out\\['qpos'\\]"),                                 # (T + 1 rows)
             (dict(good, out={"qvel": z(M, T + 1, nq)}), "out\\['qvel'\\]"),
             (dict(good, out={"A": z(M, T, 2 * nv, 2 * nv)}), "out has \\['A'\\]"),
             (dict(good, nominal=False, out={"qpos": z(M, T + 1, nq)}), "out has \\['qpos'\\]")]
    refused(monkeypatch, p.trajectory_fd, cases)
    # the good calls get as far as the C call: the stand-in has no handle, and the library refuses it
    for kw in (good, dict(good, centered=False, nominal=False), dict(ctrl=z(3, T, nu), env_ids=[1, 3, 1]), dict(good, nsteps=1, eps=1e-6),
               dict(good, out={"columns": z(M, T, ncol, w), "qpos": z(M, T + 1, nq), "qvel": z(M, T + 1, nv)})):
        with pytest.raises(RuntimeError, match="rsr_physics_trajectory_fd: null handle"):
            p.trajectory_fd(**kw)
    # ... as the one library call in the env-list convention (repeats allowed), ctrl kept in the method's own slot, not copied
    rec = record(monkeypatch)
    c = z(3, T, nu)
    p.trajectory_fd(c, env_ids=[1, 3, 1])
    (sym, args), = rec.calls
    assert sym == "rsr_physics_trajectory_fd" and len(args) == 10 and args[2:4] == (3, c.data_ptr()) and ints(args[1], 3) == [1, 3, 1]
    assert p._held["trajectory_fd"][0] is c and p._held["trajectory_fd"][1].data_ptr() == args[1]
