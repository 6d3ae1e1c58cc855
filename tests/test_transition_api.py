"""Finite-difference transition Jacobians of the physics layer (rsr_physics_transition_fd / rsr_physics_transition_view,
Physics.transition_fd), host side only: the ABI and the Python surface.  The kernel is covered by tests/test_transition_gpu.py."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rsr_mjx_amd", "csrc")


def _header():
    return open(os.path.join(ROOT, "include", "rsr_physics.h")).read()


def test_header_declares_the_transition_api():
    h = _header()
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
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", _header())) == set(_lib.PHYS_SYMBOLS)
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
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "fd_alloc", "launch(")
    first_dev = lambda b: min(b.index(k) for k in dev if k in b)
    call = body("int rsr_physics_transition_fd")
    for check in ("!p)", "nsteps < 1", "nsteps > INT32_MAX / 2", "std::isfinite(eps)", "eps > 0.0f", "~(RSR_FD_CENTERED | RSR_FD_STATES)", "count < 1"):
        assert call.index(check) < first_dev(call), check
    assert call.count("RSR_ERR_ARG") >= 5 and "fd_alloc(" in call
    assert "OP_PHYS_ROLLOUT" in call and "r.fd = rsr::FdArgs{" in call       # rides on the rollout op
    view = body("int rsr_physics_transition_view")
    assert view.index("default: return fail(RSR_ERR_ARG") < first_dev(view)
    for f in ("COLUMNS", "STATES_X", "STATES_Y"):
        assert f"RSR_T_{f}" in view, f
    alloc = body("static int fd_alloc")
    assert "if (p->fd && (!states || p->fd_states)) return RSR_OK;" in alloc and "hipMemset(buf, 0," in alloc
    assert "if (states && !p->fd_states)" in alloc                           # the states buffer only on request
    destroy = body("void rsr_physics_destroy")
    assert "hipFree(p->fd)" in destroy and "hipFree(p->fd_states)" in destroy


def test_the_kernel_lives_in_the_physics_layer():
    """transition_kernel is a file of its own under csrc/physics that calls the step's stages instead of restating them: one
    forward<C> in the loop over the two runs' substeps (or two calls), no inline assembly, no read-modify-write memory
    operations; no source directly under csrc/ knows of it, so the hashed sources are those the parity envelopes were measured on."""
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
            assert "transition_kernel" not in text and "FdArgs" not in text and "rsr_transition" not in text, f
    kernels = open(os.path.join(CSRC, "physics", "rsr_physics_kernels.hpp")).read()
    lp = kernels[kernels.index("int launch_physics("):]
    roll_case = lp[lp.index("case OP_PHYS_ROLLOUT:"):lp.index("case OP_PHYS_DYNAMICS:")]
    assert "if (x.r.fd.out)" in roll_case
    assert "transition_kernel<C, WAVES, Applied>" in roll_case and "transition_kernel<C, WAVES>" in roll_case
    assert "rollout_kernel<C, WAVES, Applied>" in roll_case and "rollout_kernel<C, WAVES>" in roll_case
    assert "transition_kernel" not in lp[lp.index("case OP_PHYS_DYNAMICS:"):]
    phys = open(os.path.join(CSRC, "physics", "rsr_physics.hpp")).read()
    assert "struct FdArgs" in phys and "struct FdLayout" in phys
    assert re.search(r"\bFdArgs fd;", re.search(r"struct RollArgs \{(.*?)\};", phys, re.S).group(1))
    import bench
    import parity_envelopes as PE
    # (the hashed sources are unchanged; the binaries of the units are not: DESIGN.md 4g)
    assert PE.ENV["_provenance"]["csrc_sha16"] == bench.csrc_sha16()


def test_physics_module_surface():
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.transition_fd)
    assert list(sig.parameters) == ["self", "env_ids", "nsteps", "eps", "centered", "keep_states"]
    d = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert d == dict(env_ids=None, nsteps=None, eps=1e-3, centered=True, keep_states=False)
    for view in ("fd_A", "fd_B", "fd_C", "fd_D", "fd_x", "fd_y"):
        assert isinstance(getattr(Physics, view), property), view
    src = inspect.getsource(Physics.transition_fd)
    assert "rsr_physics_transition_fd(" in src and 'self._ids(env_ids, "transition_fd")' in src and "self._fd_ids_in = ids32" in src
    assert "n_substeps" in src
    assert "Physics.transition_fd()" in physics.__doc__ and "mjd_transitionFD" in physics.__doc__
