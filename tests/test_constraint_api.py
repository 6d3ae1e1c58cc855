"""Constraint and contact forces of the physics layer (rsr_physics_constraint / rsr_physics_constraint_view,
Physics.constraint_forces / Physics.contact_forces), host side only: the ABI and the Python surface.  The kernel is covered by
tests/test_constraint_gpu.py."""
import ctypes as C
import inspect
import os
import re

from api_support import CSRC, HANDLE, STREAM, header, ints, record, standin


def test_header_declares_the_constraint_api():
    h = header()
    for sig in ("int rsr_physics_constraint(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream);",
                "int rsr_physics_constraint_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);"):
        assert sig in h, sig
    enum = re.sub(r"/\*.*?\*/", "", re.search(r"enum rsr_constraint_field \{(.*?)\n\};", h, re.S).group(1), flags=re.S)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    from rsr_mjx_amd import _lib
    assert names == ["RSR_C_" + f.upper() for f in _lib.CONSTRAINT_FIELDS] + ["RSR_C_COUNT"]
    assert "RSR_C_QFRC_CONSTRAINT = 0" in enum
    assert _lib.CONSTRAINT_FIELDS == ["qfrc_constraint", "qacc", "efc_counts", "efc_force", "ncon", "contact", "contact_wrench"]
    # documented as a forward pass at the state after the integration, writing nothing else
    doc = h[h.index("/* Constraint and contact forces"):h.index("enum rsr_constraint_field")]
    assert "after the last integration" in doc and "Nothing else is written" in doc and "qacc_warmstart" in doc
    # the other enums are unchanged
    assert len(_lib.PHYS_FIELDS) == 7 and len(_lib.APPLIED_FIELDS) == 2 and len(_lib.DYNAMICS_FIELDS) == 6


def test_library_exports_and_argument_checks():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    for sym in ("rsr_physics_constraint", "rsr_physics_constraint_view"):
        assert sym in _lib.PHYS_SYMBOLS and getattr(L, sym) is not None
        assert getattr(L, sym).argtypes is not None
    # null handle, refused before any device work
    ids = (C.c_int32 * 2)(0, 1)
    for table, k in ((None, 0), (ids, 2), (ids, 0)):
        assert L.rsr_physics_constraint(None, table, k, None) == -1
        assert b"null" in L.rsr_last_error()
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    for fid in (0, len(_lib.CONSTRAINT_FIELDS) - 1, len(_lib.CONSTRAINT_FIELDS), -1):
        assert L.rsr_physics_constraint_view(None, fid, C.byref(ptr), shape, stride) == -1
    assert not ptr.value


def test_argument_checks_come_before_device_work():
    """env_ids with count < 1 and unknown view ids: RSR_ERR_ARG on a real handle, with the check ahead of every device call and of
    the buffer's allocation (checked by source order, as the handle needs a device); the buffer goes with the handle."""
    src = open(os.path.join(CSRC, "physics", "rsr_physics.hip")).read()

    def body(name):
        b = src[src.index(name + "("):]
        return b[:b.index("\n}\n")]
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "zeroed_once", "con_buffer", "dyn_buffers", "launch(")
    first_dev = lambda b: min(b.index(k) for k in dev if k in b)
    call = body("int rsr_physics_constraint")
    assert call.index("!p)") < first_dev(call) and call.index("env_count(") < first_dev(call)
    count = body("static int env_count")                                     # the shared refusal of a list with count < 1
    assert 'if (env_ids && count < 1) return fail(RSR_ERR_ARG, std::string(who) + ": count < 1 with env_ids");' in count
    assert not any(k in count for k in dev)
    assert call.count("RSR_ERR_ARG") + count.count("RSR_ERR_ARG") == 2 and "con_buffer(" in call and "OP_PHYS_CONSTRAINT" in call
    assert "rsr::ConArgs{ph->con, ids}" in body("static rsr::Launch physics_args")      # the op runs on the handle's buffer
    launch = body("static int physics_launch")                               # no defaulted parameter: a prepared Launch
    assert " = " not in launch[:launch.index(")")] and "const rsr::Launch& x" in launch[:launch.index(")")]
    view = body("int rsr_physics_constraint_view")
    assert view.index("default: return fail(RSR_ERR_ARG") < first_dev(view)
    for f in ("QFRC_CONSTRAINT", "QACC", "EFC_COUNTS", "EFC_FORCE", "NCON", "CONTACT", "CONTACT_WRENCH"):
        assert f"case RSR_C_{f}:" in view, f
    alloc = body("static int zeroed_once")                                   # once, zeroed, never moved
    alloc = alloc[alloc.index("{"):]
    assert alloc.index("if (*slot) return RSR_OK;") < first_dev(alloc) and "hipMemset(buf, 0, bytes)" in alloc
    assert alloc.count("*slot = ") == 1 and "p->con = " not in src
    assert "con_buffer(" in view                                             # by the call or by its view, whichever is first
    assert "return zeroed_once(p, &p->con, " in body("static int con_buffer") and src.count("&p->con,") == 1      # one size, one place
    assert src.count("static int zeroed_once(") == 1 and "_alloc" not in src
    destroy = body("void rsr_physics_destroy")
    assert "hipFree(p->con)" in destroy


def test_the_kernel_lives_in_the_physics_layer():
    """constraint_kernel is a file of its own under csrc/physics, calls forward<C> once with a rows tail instead of restating its
    stages, and has an op of its own in launch_physics, plain or applied; no kernel source outside csrc/physics knows of it, and
    the parity envelopes were measured on these kernel sources."""
    kern = open(os.path.join(CSRC, "physics", "rsr_constraint.hpp")).read()
    assert "void constraint_kernel(" in kern
    assert kern.count("forward<C>(") == 1
    code = re.sub(r"//.*", "", kern)                                       # one statement of the forward pass: none of its stages here
    named = re.findall(r"\b(kinematics|com_crb_mass|load_mrow|smooth_forces|\w+_factor|\w+_solve|collision|make_constraint|solve)\b", code)
    assert not named, named
    order = [kern.index(k) for k in ("forward<C>(", "rows_cost<C, false>(", "jt_force<C>(", "make_frame(")]
    assert order == sorted(order)
    assert "asm" not in kern and "atomic" not in kern                      # plain stores only
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "constraint_kernel" not in text and "ConLayout" not in text and "rsr_constraint" not in text, f
    kernels = open(os.path.join(CSRC, "physics", "rsr_physics_kernels.hpp")).read()
    lp = kernels[kernels.index("int launch_physics("):]
    dyn_case = lp[lp.index("case OP_PHYS_DYNAMICS:"):lp.index("case OP_PHYS_CONSTRAINT:")]
    assert "dynamics_kernel<C, WAVES>" in dyn_case and "constraint_kernel" not in dyn_case
    con_case = re.search(r"case OP_PHYS_CONSTRAINT:(.*?)\n\s*(?:case |default:)", lp, re.S).group(1)      # (up to the next case label)
    assert "constraint_kernel<C, WAVES, Applied>" in con_case and "constraint_kernel<C, WAVES>" in con_case
    assert re.findall(r"\b\w+_kernel\b", con_case) == ["constraint_kernel"] * 2
    dyn = open(os.path.join(CSRC, "physics", "rsr_dynamics.hpp")).read()
    assert "constraint_kernel" not in dyn
    phys = open(os.path.join(CSRC, "physics", "rsr_physics.hpp")).read()
    assert "struct ConLayout" in phys and "struct ConArgs" in phys and "sizeof(DynArgs) == 32" in phys
    import bench
    import parity_envelopes as PE
    assert PE.ENV["_provenance"]["csrc_sha16"] == bench.csrc_sha16()


def test_physics_module_surface(monkeypatch):
    from rsr_mjx_amd.physics import Physics
    for m in ("constraint_forces", "contact_forces"):
        assert callable(getattr(Physics, m))
    assert list(inspect.signature(Physics.constraint_forces).parameters) == ["self", "env_ids"]
    assert list(inspect.signature(Physics.contact_forces).parameters) == ["self"]
    for view in ("qfrc_constraint", "efc_force", "efc_counts", "constraint_qacc"):
        assert isinstance(getattr(Physics, view), property), view
    src = inspect.getsource(Physics.contact_forces)
    for key in ("ncon=", "dist=", "pos=", "normal=", "geom1=", "geom2=", "normal_force=", "force=", "torque="):
        assert key in src, key
    # the env-list calling convention: (handle, ids, count, stream), null and 0 for every env
    p, rec = standin(), record(monkeypatch)
    p.constraint_forces()
    p.constraint_forces([2, 0])
    (s0, a0), (s1, (h, ids, k, stream)) = rec.calls
    assert s0 == s1 == "rsr_physics_constraint" and a0 == (HANDLE, None, 0, STREAM) and (h, k, stream) == (HANDLE, 2, STREAM) and ints(ids, 2) == [2, 0]
