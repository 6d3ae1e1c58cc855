"""Inverse kinematics on site pose targets (rsr_physics_ik, Physics.ik), host side only: the ABI, the entry point's refusals ahead of
its first device call, the kernel's header and dispatch, and the Python surface with every bad input refused before the C call.
The kernel is covered by tests/test_ik_gpu.py, the numpy reference it is held against by tests/test_ik_ref.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_support import CSRC, ROOT, body as _body, header, ints, read as _read, record, refused, standin
SIG = ("int rsr_physics_ik(rsr_physics* p, const int32_t* env_ids, int count, const rsr_ik_task* task, const rsr_ik_in* in, "
       "const rsr_ik_opt* opt, const rsr_ik_out* out, void* hip_stream);")


def test_header_declares_the_call_and_the_structs():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat
    assert ("typedef struct rsr_ik_task { int32_t nsite; int32_t sites[RSR_MAX_JAC_SITES]; float pos_weight[RSR_MAX_JAC_SITES]; "
            "float rot_weight[RSR_MAX_JAC_SITES]; uint32_t dofs; } rsr_ik_task;") in flat
    assert "typedef struct rsr_ik_in { const float* target_pos; const float* target_quat; const float* qpos0; const float* damping; } rsr_ik_in;" in flat
    assert "typedef struct rsr_ik_opt { int32_t iters; float tol_pos; float tol_rot; float max_step; int32_t limits; } rsr_ik_opt;" in flat
    assert "typedef struct rsr_ik_out { float* qpos; float* err; int32_t* info; } rsr_ik_out;" in flat
    doc = h[h.index("/* Inverse kinematics on site pose targets"):h.index("typedef struct rsr_ik_task")]
    for word in ("[M, nsite, 3]", "[M, nsite, 4]", "(w, x, y, z", "[M, nq]", "damping [M]", "read on the device", "by value", "rsr_physics_set_jac_sites",
                 "more than once", "out of range leaves", "kinematics(q)", "rotation vector of R*_k R_k^T", "the short way round", "it == iters",
                 "(J^T J + lambda I)^-1 J^T b", "max_step / max|dq|", "mj_integratePos", "body-frame rotation vector", "jnt_range where jnt_limited",
                 "status 2", "iterations taken, status", "forward-kinematics query", "bit for bit", "untouched", "owns no buffer",
                 "before any device work", "all weights zero", "without target_quat"):
        assert word in doc, word
    assert "rsr_physics_ik      <-" in h[:h.index("typedef")]                       # the opening list
    assert "rsr_ik" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_structs_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_ik" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_ik
    assert fn.argtypes is not None and len(fn.argtypes) == 8
    K = _lib.MAX_JAC_SITES
    assert [n for n, _ in _lib.IkTask._fields_] == ["nsite", "sites", "pos_weight", "rot_weight", "dofs"] and C.sizeof(_lib.IkTask) == 4 + 12 * K + 4
    assert [n for n, _ in _lib.IkIn._fields_] == ["target_pos", "target_quat", "qpos0", "damping"] and C.sizeof(_lib.IkIn) == 4 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _lib.IkOpt._fields_] == ["iters", "tol_pos", "tol_rot", "max_step", "limits"] and C.sizeof(_lib.IkOpt) == 20
    assert [n for n, _ in _lib.IkOut._fields_] == ["qpos", "err", "info"] and C.sizeof(_lib.IkOut) == 3 * C.sizeof(C.c_void_p)
    # the kernel's argument struct: eight pointers, the three tables by value, seven scalars
    phys = _read("physics", "rsr_physics.hpp")
    args = re.search(r"struct IkArgs \{(.*?)\};", phys, re.S).group(1)
    assert "int sites[RSR_MAX_JAC_SITES];" in args and "float wp[RSR_MAX_JAC_SITES], wr[RSR_MAX_JAC_SITES];" in args and "unsigned dofs;" in args
    assert "static_assert(sizeof(IkArgs) == 64 + 12 * RSR_MAX_JAC_SITES + 32," in phys
    task, ins, opt, out = _lib.IkTask(), _lib.IkIn(), _lib.IkOpt(), _lib.IkOut()
    for t in (None, C.byref(task)):
        assert fn(None, None, 0, t, C.byref(ins), C.byref(opt), C.byref(out), None) == -1
        assert b"rsr_physics_ik: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every RSR_ERR_ARG check of the entry comes ahead of its first device call (by source order, as a handle needs a device); the
    call owns no buffer, and its one launch is an op of its own with the one argument struct."""
    src = _read("physics", "rsr_physics.hip")
    call = _body(src, "int rsr_physics_ik")
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "nominal_scratch(",
           "physics_args(", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_args(")
    checks = ("!p)", "!task || !in || !opt || !out)", "!in->target_pos || !in->damping)", "!out->qpos || !out->err || !out->info)", "env_count(",
              "task->nsite < 1 || task->nsite > RSR_MAX_JAC_SITES", "task->sites[k] >= d.nsite", "wp < 0.0f || wr < 0.0f", "if (!any)",
              "rot && !in->target_quat", "(task->dofs >> d.nv) != 0u", "opt->iters < 0", "opt->max_step < 0.0f", "opt->limits != 0 && opt->limits != 1")
    at = [call.index(c) for c in checks]
    assert at == sorted(at) and all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.rindex("RSR_ERR_ARG") < first_dev and call.count("RSR_ERR_ARG") == len(checks) - 1       # (env_count's is its own)
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipDeviceSynchronize", "zeroed_once", "p->jac_sites", "p->njac", "p->dyn", "counted("):
        assert k not in call, k
    assert re.findall(r"\bOP_\w+", call) == ["OP_IK"] and call.count("physics_launch(") == 1
    assert sorted(set(re.findall(r"\bx\.ph\.(\w+)", call))) == ["ik"]
    for part in (_body(src, "void rsr_physics_destroy"), src[src.index("struct rsr_physics {"):src.index("};")]):
        assert "ik_" not in part and "Ik" not in part


def test_the_kernel_is_a_header_of_its_own_and_shares_the_site_jacobian():
    kern = _read("physics", "rsr_ik.hpp")
    code = re.sub(r"//.*", "", kern)
    assert "void ik_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, IkArgs q)" in code
    assert "template <class C, int WAVES>" in code and "__launch_bounds__(64)" in code and '#include "rsr_dynamics.hpp"' in code
    body = code[code.index("void ik_kernel("):]
    for w in ("load_overrides<C>(", "kinematics<C>(", "com_crb_mass<C>(", "site_jac<C>(", "chol_factor<C, true>(", "chol_solve<C>(", "rowtree_factor<C, true>(", "rowchol_factor<C, true, true>(", "arrow_factor<C, true>(", "uniform_i(",
              "q.qpos0 ?", "e < 0 || e >= a.n", "status = 2"):
        assert w in body, w
    for w in ("smooth_forces<C>(", "collision<C>(", "forward<C>(", "integrate<C>(", "atomic", "double", "rec[", "q.ids[lane"):
        assert w not in body, w
    # nothing of the record or the handle is written: the only global stores go through the three output pointers
    stores = re.findall(r"\b(q\.\w+)\[[^\]]*\] = ", body)
    assert set(stores) == {"q.qpos", "q.err", "q.info"}, stores
    assert not re.search(r"\ba\.state\[[^\]]*\]\s*=[^=]", body) and "a.state +" in body
    # dynamics_kernel calls the same device function
    dyn = re.sub(r"//.*", "", _read("physics", "rsr_dynamics.hpp"))
    assert dyn.count("site_jac<C>(") == 1 and "SiteJac site_jac(" in dyn and "body_dofmask" not in dyn[dyn.index("void dynamics_kernel("):]
    # the dispatch: an op of the physics enum taken ahead of the switch, its struct a field of the launch's
    phys = _read("physics", "rsr_physics.hpp")
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert re.findall(r"\bOP_IK\w*", enum) == ["OP_IK"] and len(re.findall(r"\bOP_PHYS_\w+", enum)) == 9
    assert re.search(r"\bIkArgs ik;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    kernels = _read("physics", "rsr_physics_kernels.hpp")
    assert '#include "rsr_ik.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    assert "op == OP_IK ? ik_lds_bytes<C>() :" in lp and lp.count("hipLaunchKernelGGL(") == 1
    assert "if (op == OP_IK) return go(ik_kernel<C, WAVES>, ph.ik);" in lp and lp.count("ik_kernel") == 1
    assert lp.index("if (op == OP_IK)") < lp.index("switch (op)") and "case OP_IK" not in lp
    # nothing outside physics/ knows
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "ik_kernel" not in text and "IkArgs" not in text and "OP_IK" not in text, f
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4n."):]
    for word in ("ik_kernel", "site_jac", "chol_factor<C, true>", "com_crb_mass", "VGPRs", "scratch", "ik_rates", "set_state"):
        assert word in sec, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    sub = readme[readme.index("#### Inverse kinematics"):]
    for word in ("phys.ik(", "q_hold", "endpoint", "dofs=", "set_state("):
        assert word in sub, word
    assert "Physics.ik(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.ik)
    assert list(sig.parameters) == ["self", "sites", "target_pos", "target_quat", "pos_weight", "rot_weight", "dofs", "qpos0", "damping", "iters",
                                    "tol_pos", "tol_rot", "max_step", "limits", "env_ids", "out"]
    assert "Physics.ik(sites, target_pos, target_quat=None)" in physics.__doc__
    doc = Physics.ik.__doc__
    for word in ("[M, K, 3]", "[M, K, 4]", "[M, nq]", "err [M, 2]", "info [M, 2]", "status", "damping", "jnt_range", "set_state", "bit for bit",
                 "more than once", "forward-kinematics query"):
        assert word in doc, word
    # every bad input is refused before the C call: the recording library sees none
    nq, nv, nsite = 6, 5, 4
    p = standin(handle=None)
    p._dyn = before = {}                                     # (the site table of set_jac_sites and its views are not this call's)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, K = 4, 2
    good = dict(sites=["tip", 1], target_pos=z(M, K, 3))
    cases = [(dict(good, sites=[]), "1 to 8 sites"), (dict(good, sites=list(range(9)) * 1, target_pos=z(M, 9, 3)), "site ids must lie|1 to 8 sites"),
             (dict(good, sites=[0] * 9, target_pos=z(M, 9, 3)), "1 to 8 sites"), (dict(good, sites=["nose", 1]), "no site 'nose'"),
             (dict(good, sites=[0, nsite]), "site ids must lie"), (dict(good, sites=[-1, 0]), "site ids must lie"),
             (dict(good, target_pos=z(M, K, 4)), "expects target_pos"), (dict(good, target_pos=z(M + 1, K, 3)), "expects target_pos"),
             (dict(good, target_pos=z(M, K, 3).double()), "expects target_pos"), (dict(good, target_pos=z(M, K, 3).numpy()), "expects target_pos"),
             (dict(good, target_pos=z(M, K, 4)[..., :3]), "expects target_pos"), (dict(good, target_pos=z(M, K, 3, device="meta")), "expects target_pos"),
             (dict(good, target_quat=z(M, K, 3)), "expects target_quat"), (dict(good, target_quat=z(M, K, 4).double()), "expects target_quat"),
             (dict(good, qpos0=z(M, nq + 1)), "expects qpos0"), (dict(good, qpos0=z(M, nq).numpy()), "expects qpos0"),
             (dict(good, pos_weight=[1.0, 2.0, 3.0]), "expects pos_weight"), (dict(good, pos_weight=-1.0), "expects pos_weight"),
             (dict(good, pos_weight=float("nan")), "expects pos_weight"), (dict(good, pos_weight="heavy"), "expects pos_weight"),
             (dict(good, rot_weight=[0.0, -0.1]), "expects rot_weight"), (dict(good, rot_weight=0.5), "needs target_quat"),
             (dict(good, pos_weight=0.0), "every weight is zero"), (dict(good, pos_weight=0.0, rot_weight=0.0, target_quat=z(M, K, 4)), "every weight is zero"),
             (dict(good, dofs=[0, nv]), "expects dofs"), (dict(good, dofs=[-1]), "expects dofs"), (dict(good, dofs=[0.5]), "expects dofs"),
             (dict(good, dofs=np.ones(nv + 1, bool)), "expects dofs"), (dict(good, damping=0.0), "expects damping"),
             (dict(good, damping=float("inf")), "expects damping"), (dict(good, damping="soft"), "expects damping"),
             (dict(good, damping=z(M + 1)), "expects damping"), (dict(good, damping=z(M).double()), "expects damping"),
             (dict(good, iters=-1), "iters must be >= 0"), (dict(good, tol_pos=-1e-3), "tol_pos must be"), (dict(good, tol_rot=float("nan")), "tol_rot must be"),
             (dict(good, max_step=-0.1), "max_step must be"), (dict(good, env_ids=[0, 4], target_pos=z(2, K, 3)), "env_ids must lie"),
             (dict(good, out={"qpos": z(M, nq + 1)}), "out\\['qpos'\\]"), (dict(good, out={"err": z(M, 2).double()}), "out\\['err'\\]"),
             (dict(good, out={"info": z(M, 2)}), "out\\['info'\\]"), (dict(good, out={"status": z(M)}), "out has \\['status'\\]")]
    refused(monkeypatch, p.ik, cases)
    # the good calls get as far as the C call: the stand-in has no handle, and the library refuses it
    for kw in (good, dict(good, target_quat=z(M, K, 4), rot_weight=[0.2, 0.0], dofs=np.array([True, False, True, True, False])),
               dict(good, sites="tip", target_pos=z(M, 1, 3), damping=torch.full((M,), 1e-2), iters=0, limits=False),
               dict(good, env_ids=[3, 3, 0], target_pos=z(3, K, 3), qpos0=z(3, nq), dofs=[4, 0], max_step=0.0,
                    out={"qpos": z(3, nq), "err": z(3, 2), "info": z(3, 2, dtype=torch.int32)})):
        with pytest.raises(RuntimeError, match="rsr_physics_ik: null handle"):
            p.ik(**kw)
    # ... as the one library call in the env-list convention (repeats allowed), on the caller's very tensors: they are kept in the
    # method's own slot, none of them copied; set_jac_sites' table is not touched
    rec = record(monkeypatch)
    kw = dict(target_pos=z(3, K, 3), target_quat=z(3, K, 4), qpos0=z(3, nq), damping=torch.full((3,), 1e-2))
    p.ik(["tip", 1], env_ids=[3, 3, 0], **kw)
    (sym, args), = rec.calls
    assert sym == "rsr_physics_ik" and len(args) == 8 and args[2] == 3 and ints(args[1], 3) == [3, 3, 0] and p._dyn is before
    assert [getattr(args[4], n) for n, _ in args[4]._fields_] == [kw[n].data_ptr() for n in ("target_pos", "target_quat", "qpos0", "damping")]
    assert all(any(t is x for x in p._held["ik"]) for t in kw.values()) and p._held["ik"][-1].data_ptr() == args[1]
