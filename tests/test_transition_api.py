"""Finite-difference transition Jacobians of the physics layer (rsr_physics_transition_fd / rsr_physics_transition_view,
Physics.transition_fd), host side only: the ABI and the Python surface.  The kernel is covered by tests/test_transition_gpu.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_support import CSRC, HANDLE, STREAM, header, ints, record, standin


def test_header_declares_the_transition_api():
    h = header()
    for sig in ("int rsr_physics_transition_fd(rsr_physics* p, const int32_t* env_ids, int count, int nsteps, float eps, int flags, void* hip_stream);",
                "int rsr_physics_transition_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);"):
        assert sig in h, sig
    from rsr_mjx_amd import _lib
    assert re.search(r"#define RSR_FD_CENTERED %d\b" % _lib.FD_CENTERED, h) and re.search(r"#define RSR_FD_STATES %d\b" % _lib.FD_STATES, h)
    assert _lib.FD_CENTERED & _lib.FD_STATES == 0
    enum = re.search(r"enum rsr_transition_field \{(.*?)\};", h, re.S).group(1)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    assert names == ["RSR_T_" + f.upper() for f in _lib.TRANSITION_FIELDS] + ["RSR_T_COUNT"]
    assert "RSR_T_COLUMNS = 0" in enum and _lib.TRANSITION_FIELDS == ["columns", "states_x", "states_y"]
    # documented as differences at the given eps that write nothing else, and as deviating from MuJoCo's ctrl nudging
    doc = h[h.index("/* Transition Jacobians by finite differences"):h.index("#define RSR_FD_CENTERED")]
    for phrase in ("mjd_transitionFD", "mj_integratePos", "mj_differentiatePos", "no ctrl-range handling", "qacc_warmstart",
                   "not its\n * derivative", "Nothing but the handle's transition buffer"):
        assert phrase in doc, phrase


def test_library_exports_and_argument_checks():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    for sym in ("rsr_physics_transition_fd", "rsr_physics_transition_view"):
        assert sym in _lib.PHYS_SYMBOLS and getattr(L, sym).argtypes is not None
    assert L.rsr_physics_transition_fd.argtypes[4] is C.c_float
    # null handle, refused before any device work
    ids = (C.c_int32 * 2)(0, 1)
    for table, k in ((None, 0), (ids, 2)):
        assert L.rsr_physics_transition_fd(None, table, k, 1, 1e-3, _lib.FD_CENTERED, None) == -1
        assert b"null" in L.rsr_last_error()
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    for fid in (0, 2, 3, -1):
        assert L.rsr_physics_transition_view(None, fid, C.byref(ptr), shape, stride) == -1
    assert not ptr.value


def test_refusals_come_before_device_work():
    """nsteps < 1, eps not finite or <= 0, unknown flag bits, env_ids with count < 1: RSR_ERR_ARG with the checks ahead of every
    device call and of the buffers' allocation (by source order, as a handle needs a device); the buffers go with the handle."""
    src = open(os.path.join(CSRC, "physics", "rsr_physics.hip")).read()

    def body(name):
        b = src[src.index(name + "("):]
        return b[:b.index("\n}\n")]
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "zeroed_once", "fd_buffers", "launch(")
    first_dev = lambda b: min(b.index(k) for k in dev if k in b)
    call = body("int rsr_physics_transition_fd")
    for check in ("!p)", "nsteps < 1", "nsteps > INT32_MAX / 2", "std::isfinite(eps)", "eps > 0.0f", "~(RSR_FD_CENTERED | RSR_FD_STATES)", "env_count("):
        assert call.index(check) < first_dev(call), check
    count = body("static int env_count")                                     # the shared refusal of a list with count < 1
    assert 'if (env_ids && count < 1) return fail(RSR_ERR_ARG, std::string(who) + ": count < 1 with env_ids");' in count
    assert not any(k in count for k in dev)
    assert call.count("RSR_ERR_ARG") + count.count("RSR_ERR_ARG") >= 5 and "fd_buffers(" in call
    assert "OP_PHYS_TRANSITION" in call and "x.ph.fd = rsr::FdArgs{" in call and "OP_PHYS_ROLLOUT" not in call      # an op of its own
    assert "RollArgs" not in call and "x.ph.r" not in call and set(re.findall(r"\bx\.ph\.(\w+)", call)) == {"fd"}
    view = body("int rsr_physics_transition_view")
    assert view.index("default: return fail(RSR_ERR_ARG") < first_dev(view)
    for f in ("COLUMNS", "STATES_X", "STATES_Y"):
        assert f"RSR_T_{f}" in view, f
    bufs = body("static int fd_buffers")
    assert 'zeroed_once(p, &p->fd, ' in bufs and "return states ? zeroed_once(p, &p->fd_states, " in bufs     # the states buffer only on request
    assert src.count("&p->fd,") == 1 and src.count("&p->fd_states,") == 1 and "p->fd = " not in src and "p->fd_states = " not in src
    alloc = body("static int zeroed_once")                                   # once, zeroed, never moved; null after a failure
    alloc = alloc[alloc.index("{"):]
    assert alloc.index("if (*slot) return RSR_OK;") < first_dev(alloc)
    assert alloc.count("*slot = ") == 1 and alloc.index("hipMemset(buf, 0, bytes)") < alloc.index("*slot = buf;")
    assert src.count("static int zeroed_once(") == 1 and "_alloc" not in src
    destroy = body("void rsr_physics_destroy")
    assert "hipFree(p->fd)" in destroy and "hipFree(p->fd_states)" in destroy


def test_the_kernel_lives_in_the_physics_layer():
    """transition_kernel is a file of its own under csrc/physics that calls the step's stages instead of restating them: one
    forward<C> in the loop over the two runs' substeps (or two calls), no inline assembly, no read-modify-write memory
    operations.  Its launch is an op of its own, a member of the physics op enum with its arguments a field of the physics launch
    struct (tests/test_dynamics_api.py checks every physics op's), which every unit forwards without naming it; no source directly
    under csrc/ knows of the kernel or the op, and the parity envelopes were measured on these sources."""
    kern = open(os.path.join(CSRC, "physics", "rsr_transition.hpp")).read()
    assert "void transition_kernel(" in kern
    code = re.sub(r"//.*", "", kern)
    nfwd = code.count("forward<C>(")
    assert nfwd == 2 or (nfwd == 1 and re.search(r"for \(int \w+ = 0; \w+ < (2|total); \+\+\w+\)", code)), nfwd
    assert code.count("integrate<C>(") == nfwd and "sensor_stage<C>(" in code and "force_stage<C>(" in code
    assert "load_overrides<C>(" in code
    named = re.findall(r"\b(kinematics|com_crb_mass|load_mrow|smooth_forces|\w+_factor|\w+_solve|collision|make_constraint|solve)\b", code)
    assert not named, named
    assert "asm" not in kern and "atomic" not in kern
    assert "perturb_state(" in kern and "differentiate_pos(" in kern
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "transition_kernel" not in text and "FdLayout" not in text and "rsr_transition" not in text and "OP_PHYS_" not in text, f
    phys = open(os.path.join(CSRC, "physics", "rsr_physics.hpp")).read()
    assert "OP_PHYS_TRANSITION" in re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1)
    assert re.search(r"\bFdArgs fd;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    for unit in ("rsr_cube.hip", "rsr_tshape.hip", "rsr_go2.hip"):          # each unit reaches launch_physics, which knows the ops
        assert "launch_physics<" in open(os.path.join(CSRC, unit)).read(), unit
    kernels = open(os.path.join(CSRC, "physics", "rsr_physics_kernels.hpp")).read()
    lp = kernels[kernels.index("int launch_physics("):]
    assert lp.rstrip().endswith("default: return -1;\n  }\n}\n\n}  // namespace rsr")
    assert "switch (op)" in lp and "gofd" not in lp and lp.count("hipLaunchKernelGGL(") == 1      # one launch lambda
    assert "op == OP_PHYS_TRANSITION ? fd_lds_bytes<C>() : sizeof(Smem<C>)" in lp
    roll_case = lp[lp.index("case OP_PHYS_ROLLOUT:"):lp.index("case OP_PHYS_TRANSITION:")]
    assert "rollout_kernel<C, WAVES, Applied>" in roll_case and "rollout_kernel<C, WAVES>" in roll_case
    assert re.findall(r"\b\w+_kernel\b", roll_case) == ["rollout_kernel"] * 2 and "fd" not in roll_case and roll_case.count("\n") == 1
    fd_case = lp[lp.index("case OP_PHYS_TRANSITION:"):lp.index("case OP_PHYS_DYNAMICS:")]
    assert "transition_kernel<C, WAVES, Applied>" in fd_case and "transition_kernel<C, WAVES>" in fd_case and "ph.fd" in fd_case
    assert re.findall(r"\b\w+_kernel\b", fd_case) == ["transition_kernel"] * 2
    assert "transition_kernel" not in lp[lp.index("case OP_PHYS_DYNAMICS:"):] and lp.count("transition_kernel") == 2
    assert "struct FdArgs" in phys and "struct FdLayout" in phys
    roll = re.search(r"struct RollArgs \{(.*?)\};", phys, re.S).group(1)      # again exactly what rollout_kernel reads
    assert "fd" not in roll and "FdArgs" not in roll
    import bench
    import parity_envelopes as PE
    assert PE.ENV["_provenance"]["csrc_sha16"] == bench.csrc_sha16()


def test_physics_module_surface(monkeypatch):
    from rsr_mjx_amd import _lib, physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.transition_fd)
    assert list(sig.parameters) == ["self", "env_ids", "nsteps", "eps", "centered", "keep_states"]
    d = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert d == dict(env_ids=None, nsteps=None, eps=1e-3, centered=True, keep_states=False)
    for view in ("fd_A", "fd_B", "fd_C", "fd_D", "fd_x", "fd_y"):
        assert isinstance(getattr(Physics, view), property), view
    # one calling convention for every entry point that takes an env list: (handle, ids, count, ..., stream) with the ids checked,
    # int32 and in env_ids order, and kept alive in the method's own slot, which is written before the call is made (two entry
    # points' launches can be in flight at once); nsteps defaults to n_substeps
    p = standin()
    rec = record(monkeypatch)
    for method, fn, own in (("dynamics", "rsr_physics_dynamics", ()), ("constraint_forces", "rsr_physics_constraint", ()),
                            ("transition_fd", "rsr_physics_transition_fd", (p.n_substeps, 1e-3, _lib.FD_CENTERED)),
                            ("set_state", "rsr_physics_forward_envs", ())):
        rec.peek[fn] = lambda *a, method=method: p._held[method]
        getattr(p, method)(env_ids=[2, 0])
        sym, (h, ids, k, *rest) = rec.calls.pop()
        assert sym == fn and (h, k, tuple(rest)) == (HANDLE, 2, own + (STREAM,)) and ints(ids, 2) == [2, 0], method
        assert [x.data_ptr() for x in rec.peeked.pop() if x is not None] == [ids], method          # held when the library is entered
        for bad, msg in (([0, 4], "env_ids must lie in"), ([1, 1], "env_ids must not repeat")):
            with pytest.raises(ValueError, match=f"{method}: {msg}"):
                getattr(p, method)(env_ids=bad)
        assert rec.calls == []
    slots = [p._held[m][-1] for m in ("dynamics", "constraint_forces", "transition_fd", "set_state")]
    assert len({t.data_ptr() for t in slots}) == 4 and all(t.tolist() == [2, 0] for t in slots)      # no single shared slot
    assert "Physics.transition_fd()" in physics.__doc__ and "mjd_transitionFD" in physics.__doc__
