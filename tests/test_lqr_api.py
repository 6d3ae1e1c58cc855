"""The LQR backward pass (rsr_physics_lqr_backward, Physics.lqr_backward), host side only: the ABI, the entry point's refusals ahead
of its first device call, the kernel's header and dispatch, and the Python surface with every bad input refused before the C call.
The kernel is covered by tests/test_lqr_gpu.py, the numpy reference it is held against by tests/test_lqr_ref.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_support import CSRC, ROOT, body as _body, header, read as _read, record, refused, standin
SIG = ("int rsr_physics_lqr_backward(rsr_physics* p, int M, int T, const float* columns, int row_stride, const rsr_lqr_cost* cost, "
       "const float* mu, int flags, const rsr_lqr_out* out, void* hip_stream);")


def test_header_declares_the_call_and_the_structs():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat                                             # (the declaration may break its lines)
    assert ("typedef struct rsr_lqr_cost { const float* lx; const float* lu; const float* lxx; const float* luu; const float* lux; } "
            "rsr_lqr_cost;") in flat
    assert "typedef struct rsr_lqr_out { float* gain; float* k; float* dv; float* status; float* vx; float* vxx; } rsr_lqr_out;" in flat
    assert re.search(r"#define RSR_LQR_REG_STATE\s+1\b", h)
    doc = h[h.index("/* LQR backward pass"):h.index("typedef struct rsr_lqr_cost")]
    for word in ("[M, T, ncol, row_stride]", "row_stride >= nx", "2 nv + nsensordata", "never read", "[M, T+1, nx]", "[M, T+1, nx, nx]",
                 "[M, T, nu]", "[M, T, nu, nu]", "[M, T, nu, nx]", "may be NULL", "mu: [M]", "Tassa", "unregularised Q", "RSR_LQR_REG_STATE",
                 "mu B^T B", "mu B^T A", "Cholesky", "(Vxx + Vxx^T) / 2", "alpha dv[0] + alpha^2 dv[1]", "rsr_feedback", "status[s] = t",
                 "status[s] = -1", "left alone", "keep what was written", "bit for bit", "no env_ids", "neither the model nor the record",
                 "untouched", "owns no buffer", "before any device work", "row_stride < 2 nv", "unknown flag bits", "2^31"):
        assert word in doc, word
    assert "rsr_physics_lqr_backward <-" in h[:h.index("typedef")]                       # the opening list
    assert "rsr_lqr" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_lqr_backward" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_lqr_backward
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    cost, out = _lib.LqrCost(), _lib.LqrOut()
    assert [n for n, _ in _lib.LqrCost._fields_] == ["lx", "lu", "lxx", "luu", "lux"] and C.sizeof(cost) == 5 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _lib.LqrOut._fields_] == ["gain", "k", "dv", "status", "vx", "vxx"] and C.sizeof(out) == 6 * C.sizeof(C.c_void_p)
    assert not any(getattr(cost, n) for n, _ in _lib.LqrCost._fields_) and not any(getattr(out, n) for n, _ in _lib.LqrOut._fields_)
    assert _lib.LQR_REG_STATE == 1
    buf = (C.c_float * 8)()
    for c in (None, C.byref(cost)):
        for o in (None, C.byref(out)):
            assert fn(None, 1, 1, buf, 8, c, buf, 0, o, None) == -1
            assert b"rsr_physics_lqr_backward: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every RSR_ERR_ARG check of the entry comes ahead of its first device call (by source order, as a handle needs a device); the
    call owns no buffer, and its one launch is an op of its own with the one argument struct."""
    src = _read("physics", "rsr_physics.hip")
    call = _body(src, "int rsr_physics_lqr_backward")
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "nominal_scratch(",
           "physics_args(", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_args(")
    checks = ("!p)", "!columns || !cost || !mu || !out)", "!cost->lx || !cost->lu || !cost->lxx || !cost->luu)",
              "!out->gain || !out->k || !out->dv || !out->status)", "M < 1 || T < 1", "row_stride < 2 * d.nv", "flags & ~RSR_LQR_REG_STATE",
              "(int64_t)M * ((int64_t)T + 1) > INT32_MAX")
    at = [call.index(c) for c in checks]
    assert at == sorted(at) and all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.count("RSR_ERR_ARG") == len(checks) and call.rindex("RSR_ERR_ARG") < first_dev
    assert "cost->lux" in call and "!cost->lux" not in call and "!out->vx" not in call           # (the optional members)
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipDeviceSynchronize", "zeroed_once", "p->nominal", "env_count(", "counted("):
        assert k not in call, k
    assert re.findall(r"\bOP_\w+", call) == ["OP_LQR_BACKWARD"] and call.count("physics_launch(") == 1
    assert sorted(set(re.findall(r"\bx\.ph\.(\w+)", call))) == ["lq"]
    assert "lqr" not in _body(src, "void rsr_physics_destroy") and "lqr" not in src[src.index("struct rsr_physics {"):src.index("};")]


def test_the_kernel_is_a_header_of_its_own():
    kern = _read("physics", "rsr_lqr.hpp")
    code = re.sub(r"//.*", "", kern)
    assert "void lqr_kernel(" in code and "template <class C, int WAVES>" in code and "__launch_bounds__(64)" in code
    body = code[code.index("void lqr_kernel("):]
    # C gives NV and NU and nothing else; the model, the layout and the record are not read
    assert set(re.findall(r"\bC::(\w+)", code)) == {"NV", "NU"}
    assert "void lqr_kernel(const DModel* __restrict__, Layout, StepArgs, LqrArgs q)" in code
    for w in ("a.state", "Smem<", "forward<C>", "integrate<C>", "asm", "atomic", "mfma", "double", "frcp(", "frsq("):
        assert w not in body, w
    assert "1.0f / sqrtf(d)" in body and "!(d > 0.0f) || !(d < __builtin_inff())" in body
    assert "q.status[slot] = (float)t;" in body and "q.status[slot] = -1.0f;" in body
    assert "extern __shared__" in body and "lqr_lds_bytes" in code
    # the dispatch: an op of the physics enum, its struct a field of the launch's, its LDS image chosen next to the others'
    phys = _read("physics", "rsr_physics.hpp")
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert re.findall(r"\bOP_LQR\w*", enum) == ["OP_LQR_BACKWARD"] and "struct LqrArgs" in phys
    assert re.search(r"\bLqrArgs lq;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    kernels = _read("physics", "rsr_physics_kernels.hpp")
    assert '#include "rsr_lqr.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    assert "op == OP_LQR_BACKWARD ? lqr_lds_bytes<C>() :" in lp and lp.count("hipLaunchKernelGGL(") == 1
    assert "if (op == OP_LQR_BACKWARD) return go(lqr_kernel<C, WAVES>, ph.lq);" in lp and lp.count("lqr_kernel") == 1
    # nothing outside physics/ knows
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "lqr_" not in text and "LqrArgs" not in text and "OP_LQR" not in text, f
    for f in os.listdir(os.path.join(CSRC, "physics")):
        if f not in ("rsr_lqr.hpp", "rsr_physics.hpp", "rsr_physics_kernels.hpp", "rsr_physics.hip") and f.endswith((".hip", ".hpp")):
            text = _read("physics", f)
            assert "lqr_" not in text and "LqrArgs" not in text and "OP_LQR" not in text, f
    # every family's LDS image stays under the 64 KB a workgroup may take
    for nv, nu in ((20, 5), (18, 12), (14, 5)):
        nx, nc = 2 * nv, 2 * nv + nu
        ib = nx // 4
        ld, kblk = nx + (0 if ib & 1 else 4), 64 // ib
        rows = kblk * -(-nc // kblk)
        floats = nx * ld + 3 * rows * ld + 2 * nu * ld + 2 * ((nu * nu + 3) & ~3) + nx + ((nc + 3) & ~3) + 32
        assert (ld // 4) % 2 == 1 and ib * kblk <= 64 and ib * (ib + 1) // 2 <= 64 and rows >= nc and 4 * floats < 48 * 1024, (nv, nu)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4m."):]
    for word in ("lqr_kernel", "LD", "ds_read_b128", "Tassa", "VGPRs", "scratch", "lqr_rates", "torch loop"):
        assert word in sec, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert readme.index("Transition Jacobians along a trajectory") < readme.index("LQR backward pass")
    sub = readme[readme.index("LQR backward pass"):]
    for word in ("trajectory_fd(", "lqr_backward(", "feedback_rollouts("):
        assert word in sub, word


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.lqr_backward)
    assert list(sig.parameters) == ["self", "columns", "lx", "lu", "lxx", "luu", "lux", "mu", "state_reg", "values", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(lux=None, mu=0.0, state_reg=False, values=False, out=None)
    assert "Physics.lqr_backward(columns, lx, lu, lxx, luu)" in physics.__doc__
    doc = Physics.lqr_backward.__doc__
    for word in ("[M, T, ncol, w]", "[M, T+1, nx]", "[M, T+1, nx, nx]", "[M, T, nu, nu]", "[M, T, nu, nx]", "trajectory_fd", "feedback_rollouts",
                 "dV [M, 2]", "status [M]", "state_reg", "Tassa", "bit for bit"):
        assert word in doc, word
    # the neighbours are as they were
    assert list(inspect.signature(Physics.trajectory_fd).parameters) == ["self", "ctrl", "nsteps", "eps", "centered", "env_ids", "nominal", "out"]
    # every bad input is refused before the C call: the recording library sees none
    nu, nq, nv = 3, 5, 4
    p = standin(handle=None, nq=nq, nv=nv)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, T, nx = 6, 3, 2 * nv                                      # (M is the buffers', not num_envs)
    ncol, w = nx + nu, nx + 2
    good = dict(columns=z(M, T, ncol, w), lx=z(M, T + 1, nx), lu=z(M, T, nu), lxx=z(M, T + 1, nx, nx), luu=z(M, T, nu, nu))
    cases = [(dict(good, columns=z(M, T, ncol)), "expects columns"),                                    # rank
             (dict(good, columns=z(M, T, ncol + 1, w)), "expects columns"),                             # ncol
             (dict(good, columns=z(M, T, ncol, nx - 1)), "expects columns"),                            # w < nx
             (dict(good, columns=z(M, 0, ncol, w)), "expects columns"),                                 # T
             (dict(good, columns=z(0, T, ncol, w)), "expects columns"),                                 # M
             (dict(good, columns=z(M, T, ncol, w).double()), "expects columns"),                        # dtype
             (dict(good, columns=z(M, T, ncol, w, device="meta")), "expects columns"),                  # device
             (dict(good, columns=z(M, T, ncol, w).numpy()), "expects columns"),                         # not a tensor
             (dict(good, columns=z(M, T, ncol, w + 1)[..., :w]), "expects columns"),                    # contiguity
             (dict(good, lx=z(M, T, nx)), "expects lx"),                                                # (T + 1 rows)
             (dict(good, lx=z(M - 1, T + 1, nx)), "expects lx"),                                        # disagreeing M
             (dict(good, lx=z(M, T + 1, nx).double()), "expects lx"),
             (dict(good, lu=z(M, T + 1, nu)), "expects lu"),                                            # disagreeing T
             (dict(good, lu=z(M, T, nu, device="meta")), "expects lu"),
             (dict(good, lxx=z(M, T, nx, nx)), "expects lxx"),
             (dict(good, lxx=z(M, T + 1, nx, nx + 1)[..., :nx]), "expects lxx"),
             (dict(good, lxx=None), "expects lxx"),
             (dict(good, luu=z(M, T, nu, nx)), "expects luu"),
             (dict(good, luu=z(M, T, nu, nu).numpy()), "expects luu"),
             (dict(good, lux=z(M, T, nx, nu)), "expects lux"),
             (dict(good, lux=z(M, T, nx, nu).transpose(2, 3)), "expects lux"),
             (dict(good, mu=z(M + 1)), "expects mu"),
             (dict(good, mu=z(M).double()), "expects mu"),
             (dict(good, mu=z(M, 1)), "expects mu"),
             (dict(good, mu="big"), "expects mu"),
             (dict(good, out={"gain": z(M, T, nx, nu)}), "out\\['gain'\\]"),
             (dict(good, out={"k": z(M, T, nu).double()}), "out\\['k'\\]"),
             (dict(good, out={"dV": z(M, 3)}), "out\\['dV'\\]"),
             (dict(good, out={"status": z(M, 1)}), "out\\['status'\\]"),
             (dict(good, out={"status": z(M).numpy()}), "out\\['status'\\]"),
             (dict(good, values=True, out={"Vxx": z(M, T, nx, nx)}), "out\\['Vxx'\\]"),
             (dict(good, values=True, out={"Vx": z(M, T + 1, nx + 1)[..., :nx]}), "out\\['Vx'\\]"),
             (dict(good, out={"Vx": z(M, T + 1, nx)}), "out has \\['Vx'\\]"),                            # (values=False)
             (dict(good, out={"K": z(M, T, nu, nx)}), "out has \\['K'\\]")]
    refused(monkeypatch, p.lqr_backward, cases)
    # the good calls get as far as the C call: the stand-in has no handle, and the library refuses it
    for kw in (good, dict(good, lux=z(M, T, nu, nx), mu=0.5, state_reg=True), dict(good, mu=z(M), values=True),
               dict(good, columns=z(M, T, ncol, nx)), dict(good, mu=1),
               dict(good, values=True, out={"gain": z(M, T, nu, nx), "k": z(M, T, nu), "dV": z(M, 2), "status": z(M), "Vx": z(M, T + 1, nx),
                                            "Vxx": z(M, T + 1, nx, nx)})):
        with pytest.raises(RuntimeError, match="rsr_physics_lqr_backward: null handle"):
            p.lqr_backward(**kw)
    # ... as the one library call, on the caller's very tensors: they are kept in the method's own slot, none of them copied
    rec = record(monkeypatch)
    kw = dict(good, lux=z(M, T, nu, nx), mu=z(M))
    p.lqr_backward(**kw)
    (sym, args), = rec.calls
    assert sym == "rsr_physics_lqr_backward" and len(args) == 10 and (args[3], args[6]) == (kw["columns"].data_ptr(), kw["mu"].data_ptr())
    assert [n for n, _ in args[5]._fields_ if getattr(args[5], n) == kw[n].data_ptr()] == ["lx", "lu", "lxx", "luu", "lux"]
    assert all(any(t is x for x in p._held["lqr_backward"]) for t in kw.values())
