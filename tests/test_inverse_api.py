"""Inverse dynamics of the physics layer (rsr_physics_inverse / rsr_physics_inverse_view, Physics.inverse), host side only: the ABI
and the Python surface.  The kernel is covered by tests/test_inverse_gpu.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_support import CSRC, ROOT, header, refused, standin


def test_header_declares_the_inverse_api():
    h = header()
    for sig in ("int rsr_physics_inverse(rsr_physics* p, const float* qacc, const int32_t* env_ids, int count, int flags, void* hip_stream);",
                "int rsr_physics_inverse_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);"):
        assert sig in h, sig
    enum = re.search(r"enum rsr_inverse_field \{(.*?)\n\};", h, re.S).group(1)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    from rsr_mjx_amd import _lib
    assert names == ["RSR_I_" + f.upper() for f in _lib.INVERSE_FIELDS] + ["RSR_I_COUNT"]
    assert "RSR_I_QFRC_INVERSE = 0" in enum
    assert _lib.INVERSE_FIELDS == ["qfrc_inverse", "qfrc_constraint", "qacc", "qfrc_actuator", "efc_counts", "efc_force"]
    assert int(re.search(r"#define RSR_INV_DISCRETE (\d+)", h).group(1)) == _lib.INV_DISCRETE == 1
    doc = h[h.index("/* Inverse dynamics"):h.index("#define RSR_INV_DISCRETE")]
    for word in ("after the last integration", "No Newton solve", "applied forces enter none", "mj_discreteAcc", "qacc_warmstart",
                 "noisy"):
        assert word in doc, word
    # the other enums are unchanged
    assert len(_lib.PHYS_FIELDS) == 7 and len(_lib.DYNAMICS_FIELDS) == 6 and len(_lib.CONSTRAINT_FIELDS) == 7
    assert len(_lib.TRANSITION_FIELDS) == 3


def test_library_exports_and_null_arguments():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    for sym in ("rsr_physics_inverse", "rsr_physics_inverse_view"):
        assert sym in _lib.PHYS_SYMBOLS and getattr(L, sym).argtypes is not None
    ids = (C.c_int32 * 2)(0, 1)
    qacc = (C.c_float * 8)()
    for table, k in ((None, 0), (ids, 2), (ids, 0)):
        assert L.rsr_physics_inverse(None, qacc, table, k, 0, None) == -1
        assert b"null handle" in L.rsr_last_error()
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    for fid in (0, len(_lib.INVERSE_FIELDS) - 1, len(_lib.INVERSE_FIELDS), -1):
        assert L.rsr_physics_inverse_view(None, fid, C.byref(ptr), shape, stride) == -1
    assert not ptr.value


def test_refusals_come_before_device_work():
    """A null handle, a null qacc, unknown flag bits, env_ids with count < 1 and an unknown field id: RSR_ERR_ARG with the checks
    ahead of every device call and of the buffer's allocation (by source order, as a handle needs a device); the buffer comes
    through the one allocation helper and goes with the handle."""
    src = open(os.path.join(CSRC, "physics", "rsr_physics.hip")).read()

    def body(name):
        b = src[src.index(name + "("):]
        return b[:b.index("\n}\n")]
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "zeroed_once", "inv_buffer", "launch(")
    first_dev = lambda b: min(b.index(k) for k in dev if k in b)
    call = body("int rsr_physics_inverse")
    for check in ("!p)", "!qacc)", "flags & ~RSR_INV_DISCRETE", "env_count("):
        assert call.index(check) < first_dev(call), check
    assert "count < 1" in body("static int env_count") and first_dev(call) < call.index("physics_launch(")
    # the dispatch: its own op with its own field, filled after the arguments physics_args shares; no other op's field is touched
    assert "rsr::OP_PHYS_INVERSE" in call and len(re.findall(r"\bOP_PHYS_\w+", call)) == 1
    assert call.index("physics_args(") < call.index("x.ph.inv = rsr::InvArgs{p->inv, env_ids, qacc, flags};") < call.index("physics_launch(")
    assert set(re.findall(r"\bx\.ph\.(\w+)", call)) == {"inv"}
    view = body("int rsr_physics_inverse_view")
    assert view.index("default: return fail(RSR_ERR_ARG") < first_dev(view) and "inv_buffer(" in view
    for f in ("QFRC_INVERSE", "QFRC_CONSTRAINT", "QACC", "QFRC_ACTUATOR", "EFC_COUNTS", "EFC_FORCE"):
        assert f"case RSR_I_{f}:" in view, f
    assert "zeroed_once(p, &p->inv, " in body("static int inv_buffer") and src.count("&p->inv,") == 1      # one size, one place
    assert "p->inv = " not in src and "hipFree(p->inv)" in body("void rsr_physics_destroy")


def test_the_kernel_restates_the_pass_without_the_solve():
    """inverse_kernel is a file of its own under csrc/physics, instantiated once per family by launch_physics.  It runs
    forward<C>'s stages up to the rows' final aref in forward<C>'s order, the discrete conversion where forward<C> factorises M,
    then constraint_kernel's tail; no Newton solve, no inline assembly, no read-modify-write memory operations, no applied
    forces."""
    kern = open(os.path.join(CSRC, "physics", "rsr_inverse.hpp")).read()
    code = re.sub(r"//.*", "", kern)
    body = code[code.index("void inverse_kernel("):]
    stages = ("kinematics<C>(", "com_crb_mass<C>(", "load_mrow<C>(", "smooth_forces<C>(", "discrete_acc<C>(", "collision<C>(",
              "make_constraint<C>(", "jdot<C>(", "row_dot<C>(", "rows_cost<C, false>(", "jt_force<C>(")
    order = [body.index(k) for k in stages]
    assert order == sorted(order)
    assert not re.findall(r"\b(solve|hessian_factor|integrate)<C>\(", code)
    assert "asm" not in kern and "atomic" not in kern and "Applied" not in code
    # where the kernel states stages of forward<C> itself, it keeps forward<C>'s order
    solver = open(os.path.join(CSRC, "rsr_solver.hpp")).read()
    fwd = solver[solver.index("__device__ __forceinline__ void forward("):solver.index("// integrate one substep")]
    shared = [k for k in stages[:8] if k in fwd and k in body]
    at = [fwd.index(k) for k in shared]
    assert at == sorted(at)
    kernels = open(os.path.join(CSRC, "physics", "rsr_physics_kernels.hpp")).read()
    lp = kernels[kernels.index("int launch_physics("):]
    assert lp.count("inverse_kernel<C, WAVES>") == 1
    # the op's own case, up to the next case label: its kernel with its arguments, and no other kernel
    case = re.search(r"case OP_PHYS_INVERSE:(.*?)\n\s*(?:case |default:)", lp, re.S).group(1)
    assert "go(inverse_kernel<C, WAVES>, ph.inv)" in case and re.findall(r"\b\w+_kernel\b", case) == ["inverse_kernel"]
    phys = open(os.path.join(CSRC, "physics", "rsr_physics.hpp")).read()
    assert "struct InvLayout" in phys and "struct InvArgs" in phys
    for top in (CSRC, os.path.join(ROOT, "include")):      # the protocol that carried the launch on the dynamics op is gone
        for d, _, files in os.walk(top):
            for f in files:
                if f.endswith((".hip", ".hpp", ".h")):
                    text = open(os.path.join(d, f)).read()
                    for gone in ("INVERSE_TAG", "SAMPLE_TAG", "inverse_launch_args", "inverse_args", "sample_launch_args", "sample_args"):
                        assert gone not in text, (f, gone)
    for f in os.listdir(CSRC):                             # nothing outside the physics layer knows
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "inverse_kernel" not in text and "rsr_inverse" not in text and "OP_PHYS_INVERSE" not in text and "InvArgs" not in text, f


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.inverse)
    assert list(sig.parameters) == ["self", "qacc", "env_ids", "discrete"]
    assert sig.parameters["env_ids"].default is None and sig.parameters["discrete"].default is False
    for view in ("qfrc_inverse", "inverse_qacc", "inverse_qfrc_constraint", "inverse_qfrc_actuator", "inverse_efc_force",
                 "inverse_efc_counts"):
        assert isinstance(getattr(Physics, view), property), view
    assert "Physics.inverse(qacc)" in physics.__doc__ and "mj_inverse" in physics.__doc__
    # a wrong shape, dtype, layout or device is refused before the C call: the recording library sees none
    p = standin(nv=6)
    good = torch.zeros((4, 6), dtype=torch.float32)
    bads = (torch.zeros((4, 5)), torch.zeros((3, 6)), torch.zeros(24), torch.zeros((4, 6), dtype=torch.float64),
            torch.zeros((6, 4)).t(), torch.zeros((4, 6), device="meta"), good.numpy(), None)
    msg = r"inverse expects qacc as a contiguous float32 tensor of shape \(4, 6\) on cpu"
    refused(monkeypatch, p.inverse, [(dict(qacc=bad, **kw), msg) for bad in bads for kw in ({}, dict(env_ids=[0], discrete=True))])
    # a good one gets as far as the C call: a stand-in without a handle, and the library refuses it
    with pytest.raises(RuntimeError, match="rsr_physics_inverse: null handle"):
        standin(handle=None, nv=6).inverse(good, env_ids=[1, 3])
