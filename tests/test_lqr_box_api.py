"""The control-limited backward pass (rsr_physics_lqr_box, Physics.lqr_backward_box, Physics.ctrl_bounds), host side only: the ABI,
the entry point's refusals ahead of its first device call, the kernel's dispatch and LDS image, and the Python surface with every
bad input refused before the C call.  The kernel is covered by tests/test_lqr_box_gpu.py, the numpy reference it is held against
by tests/test_lqr_box_ref.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_support import ROOT, body as _body, header, read as _read, record, refused, standin
SIG = ("int rsr_physics_lqr_box(rsr_physics* p, int M, int T, const float* columns, int row_stride, const rsr_lqr_cost* cost, "
       "const rsr_lqr_box* box, const float* mu, int max_iter, int flags, const rsr_lqr_out* out, void* hip_stream);")


def test_header_declares_the_call_and_the_struct():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat
    assert "typedef struct rsr_lqr_box { const float* lo; const float* hi; float* clamped; float* qp; } rsr_lqr_box;" in flat
    doc = h[h.index("/* Control-limited LQR backward pass"):h.index("typedef struct rsr_lqr_box")]
    for word in ("Tassa, Mansard and Todorov 2014", "RSR_FB_CLAMP", "[M, T, nu]", "[M, T, 2]", "ctrlrange - u_nom", "-inf / +inf", "may be NULL",
                 "-1 where", "+1 at hi", "0 converged", "1 every control clamped", "2 max_iter reached", "3 the line search found no descent",
                 "max_iter in [1, 64]", "x = min(max(0, l), h)", "grad_j = g_j + sum_i H_ji x_i", "c_prev", "all c: code 1", "code 0, stop",
                 "it == max_iter: code 2", "replaced by the identity", "r_j = 0 where c_j", "y = -Hm^-1 r", "fl(x_j + d_j)", "a = 0.6^n",
                 "0.1 grad^T (x - z)", "code 3", "rows of the last c are 0", "Every loop is bounded", "KKT", "bit for bit", "qp is (1, 0)",
                 "status[s] = t", "status[s] = -1", "left alone", "owns no buffer", "before any device work", "NULL box", "outside [1, 64]"):
        assert word in doc, word
    assert "rsr_physics_lqr_box <-" in h[:h.index("typedef")]                            # the opening list
    assert h.index("int rsr_physics_lqr_backward(") < h.index("/* Control-limited LQR backward pass") < h.index("/* Kalman filter")


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert "rsr_physics_lqr_box" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_lqr_box
    assert fn.argtypes is not None and len(fn.argtypes) == 12
    box = _lib.LqrBox()
    assert [n for n, _ in _lib.LqrBox._fields_] == ["lo", "hi", "clamped", "qp"] and C.sizeof(box) == 4 * C.sizeof(C.c_void_p)
    assert not any(getattr(box, n) for n, _ in _lib.LqrBox._fields_)
    cost, out = _lib.LqrCost(), _lib.LqrOut()
    buf = (C.c_float * 8)()
    for b in (None, C.byref(box)):
        assert fn(None, 1, 1, buf, 8, C.byref(cost), b, buf, 32, 0, C.byref(out), None) == -1
        assert b"rsr_physics_lqr_box: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every RSR_ERR_ARG check of the entry comes ahead of its first device call (by source order, as a handle needs a device); the
    call owns no buffer, and its one launch is an op of its own with the one argument struct."""
    src = _read("physics", "rsr_physics.hip")
    call = _body(src, "int rsr_physics_lqr_box")
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "nominal_scratch(",
           "physics_args(", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_args(")
    checks = ("!p)", "!columns || !cost || !box || !mu || !out)", "!cost->lx || !cost->lu || !cost->lxx || !cost->luu)", "!box->lo || !box->hi)",
              "!out->gain || !out->k || !out->dv || !out->status)", "M < 1 || T < 1", "row_stride < 2 * d.nv", "max_iter < 1 || max_iter > 64",
              "flags & ~RSR_LQR_REG_STATE", "(int64_t)M * ((int64_t)T + 1) > INT32_MAX")
    at = [call.index(c) for c in checks]
    assert at == sorted(at) and all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.count("RSR_ERR_ARG") == len(checks) and call.rindex("RSR_ERR_ARG") < first_dev
    assert "box->clamped" in call and "!box->clamped" not in call and "!box->qp" not in call and "!cost->lux" not in call     # (optional)
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipDeviceSynchronize", "zeroed_once", "p->nominal", "env_count(", "counted("):
        assert k not in call, k
    assert re.findall(r"\bOP_\w+", call) == ["OP_BOX_BACKWARD"] and call.count("physics_launch(") == 1
    assert sorted(set(re.findall(r"\bx\.ph\.(\w+)", call))) == ["bx"]
    assert "box" not in _body(src, "void rsr_physics_destroy") and "box" not in src[src.index("struct rsr_physics {"):src.index("};")]


def test_the_kernel_shares_the_plain_pass_body():
    kern = _read("physics", "rsr_lqr.hpp")
    code = re.sub(r"//.*", "", kern)
    assert "void box_backward_kernel(const DModel* __restrict__, Layout, StepArgs, BoxArgs b)" in code
    assert "lqr_body<C, true>(b.lq, b);" in code and "lqr_body<C, false>(q, BoxArgs{});" in code
    assert code.count("1.0f / sqrtf(d)") == 1 and code.count("row_dot<NX>(F + (NX + j) * LD, W + (NX + j2) * LD, 0.0f)") == 1     # one body
    body = code[code.index("void lqr_body(const LqrArgs& q, const BoxArgs& bx) {"):]
    for w in ("a.state", "Smem<", "forward<C>", "integrate<C>", "asm", "atomic", "mfma", "double"):
        assert w not in body, w
    assert "n < 20" in body and "it == bx.max_iter" in body and "0.6f" in body and "0.1f * gd" in body and "__ballot(" in body
    phys = _read("physics", "rsr_physics.hpp")
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert re.findall(r"\bOP_BOX\w*", enum) == ["OP_BOX_BACKWARD"] and "struct BoxArgs" in phys
    assert re.search(r"\bBoxArgs bx;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    lp = _read("physics", "rsr_physics_kernels.hpp")
    lp = lp[lp.index("int launch_physics("):]
    assert "op == OP_BOX_BACKWARD ? box_lds_bytes<C>() :" in lp and lp.count("hipLaunchKernelGGL(") == 1
    assert "if (op == OP_BOX_BACKWARD) return go(box_backward_kernel<C, WAVES>, ph.bx);" in lp and lp.count("box_backward_kernel") == 1
    assert lp.index("if (op == OP_BOX_BACKWARD)") < lp.index("switch (op)")
    # every family's LDS image stays under the 64 KB a workgroup may take: the plain image, Quu~ once more and five vectors of 16
    for nv, nu in ((20, 5), (18, 12), (14, 5)):
        nx, nc = 2 * nv, 2 * nv + nu
        ib = nx // 4
        ld, kblk = nx + (0 if ib & 1 else 4), 64 // ib
        rows = kblk * -(-nc // kblk)
        plain = nx * ld + 3 * rows * ld + 2 * nu * ld + 2 * ((nu * nu + 3) & ~3) + nx + ((nc + 3) & ~3) + 32
        floats = plain + ((nu * nu + 3) & ~3) + 5 * 16
        assert 4 * floats < 64 * 1024, (nv, nu, 4 * floats)
    assert "X = H + ((NU * NU + 3) & ~3), GR = X + 16, R = GR + 16, Z = R + 16, HZ = Z + 16;" in code and "FLOATS = HZ + 16;" in code
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4s."):]
    for word in ("box_backward_kernel", "Tassa, Mansard and Todorov", "bit for bit", "KKT", "VGPRs", "scratch", "LDS", "waves per SIMD", "lqr_box_rates",
                 "lqr_rates_parent_vs_box"):
        assert word in sec, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert readme.index("LQR backward pass") < readme.index("Control-limited backward pass")
    sub = readme[readme.index("Control-limited backward pass"):]
    for word in ("trajectory_fd(", "ctrl_bounds(", "lqr_backward_box(", "feedback_rollouts(", "clamp=True"):
        assert word in sub, word
    assert "rsr_physics_lqr_box" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.lqr_backward_box)
    assert list(sig.parameters) == ["self", "columns", "lx", "lu", "lxx", "luu", "lo", "hi", "lux", "mu", "state_reg", "values", "max_iter", "report", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(lux=None, mu=0.0, state_reg=False, values=False, max_iter=32, report=False, out=None)
    assert list(inspect.signature(Physics.ctrl_bounds).parameters) == ["self", "u_nom"]
    assert "Physics.lqr_backward_box(columns, lx, lu, lxx, luu, lo, hi)" in physics.__doc__ and "Physics.ctrl_bounds(u_nom)" in physics.__doc__
    doc = Physics.lqr_backward_box.__doc__
    for word in ("Tassa, Mansard and Todorov 2014", "[M, T, nu]", "[M, T, 2]", "ctrl_bounds", "clamp=True", "max_iter", "report", "bit for bit",
                 "0 converged", "-inf / +inf"):
        assert word in doc, word
    nu, nq, nv = 3, 5, 4
    p = standin(handle=None, nq=nq, nv=nv)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, T, nx = 6, 3, 2 * nv
    ncol, w = nx + nu, nx + 2
    good = dict(columns=z(M, T, ncol, w), lx=z(M, T + 1, nx), lu=z(M, T, nu), lxx=z(M, T + 1, nx, nx), luu=z(M, T, nu, nu), lo=z(M, T, nu), hi=z(M, T, nu))
    cases = [(dict(good, columns=z(M, T, ncol)), "expects columns"),
             (dict(good, columns=z(M, T, ncol, nx - 1)), "expects columns"),
             (dict(good, columns=z(M, T, ncol, w).double()), "expects columns"),
             (dict(good, lx=z(M, T, nx)), "expects lx"),
             (dict(good, luu=z(M, T, nu, nx)), "expects luu"),
             (dict(good, lux=z(M, T, nx, nu)), "expects lux"),
             (dict(good, mu=z(M + 1)), "expects mu"),
             (dict(good, lo=z(M, T, nu + 1)), "expects lo"),                                           # shape
             (dict(good, lo=z(M, T + 1, nu)), "expects lo"),                                           # disagreeing T
             (dict(good, lo=None), "expects lo"),
             (dict(good, lo=z(M, T, nu).double()), "expects lo"),                                      # dtype
             (dict(good, hi=z(M, T, nu, device="meta")), "expects hi"),                                # device
             (dict(good, hi=z(M, T, nu).numpy()), "expects hi"),                                       # not a tensor
             (dict(good, hi=z(M, T, nu + 1)[..., :nu]), "expects hi"),                                 # contiguity
             (dict(good, max_iter=0), "max_iter"),
             (dict(good, max_iter=65), "max_iter"),
             (dict(good, max_iter=2.0), "max_iter"),
             (dict(good, max_iter=True), "max_iter"),
             (dict(good, out={"clamped": z(M, T, nu)}), "out has \\['clamped'\\]"),                     # (report=False)
             (dict(good, report=True, out={"clamped": z(M, T, nu + 1)}), "out\\['clamped'\\]"),
             (dict(good, report=True, out={"qp": z(M, T, 2).double()}), "out\\['qp'\\]"),
             (dict(good, out={"Vx": z(M, T + 1, nx)}), "out has \\['Vx'\\]"),
             (dict(good, out={"gain": z(M, T, nx, nu)}), "out\\['gain'\\]")]
    refused(monkeypatch, p.lqr_backward_box, cases)
    for kw in (good, dict(good, lux=z(M, T, nu, nx), mu=0.5, state_reg=True, max_iter=1), dict(good, mu=z(M), values=True, report=True, max_iter=64),
               dict(good, report=True, out={"clamped": z(M, T, nu), "qp": z(M, T, 2), "k": z(M, T, nu)})):
        with pytest.raises(RuntimeError, match="rsr_physics_lqr_box: null handle"):
            p.lqr_backward_box(**kw)
    # the one library call, on the caller's very tensors, held in the method's own slot
    rec = record(monkeypatch)
    kw = dict(good, lux=z(M, T, nu, nx), mu=z(M), report=True, max_iter=7, state_reg=True)
    res = p.lqr_backward_box(**kw)
    (sym, args), = rec.calls
    assert sym == "rsr_physics_lqr_box" and len(args) == 12 and (args[1], args[2], args[3], args[4]) == (M, T, kw["columns"].data_ptr(), w)
    assert (args[7], args[8], args[9]) == (kw["mu"].data_ptr(), 7, 1)
    assert [getattr(args[5], n) for n in ("lx", "lu", "lxx", "luu", "lux")] == [kw[n].data_ptr() for n in ("lx", "lu", "lxx", "luu", "lux")]
    assert [getattr(args[6], n) for n in ("lo", "hi", "clamped", "qp")] == [kw["lo"].data_ptr(), kw["hi"].data_ptr(), res["clamped"].data_ptr(), res["qp"].data_ptr()]
    assert [getattr(args[10], n) for n in ("gain", "k", "dv", "status", "vx", "vxx")] == [res["gain"].data_ptr(), res["k"].data_ptr(), res["dV"].data_ptr(),
                                                                                         res["status"].data_ptr(), None, None]
    assert list(res) == ["gain", "k", "dV", "status", "clamped", "qp"] and tuple(res["qp"].shape) == (M, T, 2)
    tensors = [v for v in kw.values() if torch.is_tensor(v)]
    assert all(any(t is x for x in p._held["lqr_backward_box"]) for t in tensors) and "lqr_backward" not in p._held
    rec.calls.clear()
    res = p.lqr_backward_box(**good)
    (sym, args), = rec.calls
    assert (getattr(args[6], "clamped"), getattr(args[6], "qp")) == (None, None) and list(res) == ["gain", "k", "dV", "status"]


def test_ctrl_bounds(monkeypatch):
    import torch
    nu = 3
    p = standin(nu=nu)
    p.env.sys.arrays.update(actuator_ctrlrange=np.array([[-1.0, 2.0], [0.0, 0.0], [-0.5, 0.5]]), actuator_ctrllimited=np.array([1, 0, 1], np.int32))
    rec = record(monkeypatch)
    u = torch.tensor([[[0.25, 3.0, 0.5], [-1.0, -7.0, 0.0]]])
    lo, hi = p.ctrl_bounds(u)
    assert rec.calls == []
    inf = float("inf")
    assert lo.dtype == hi.dtype == torch.float32 and lo.is_contiguous() and hi.is_contiguous() and tuple(lo.shape) == tuple(hi.shape) == (1, 2, nu)
    assert lo.tolist() == [[[-1.25, -inf, -1.0], [0.0, -inf, -0.5]]] and hi.tolist() == [[[1.75, inf, 0.0], [3.0, inf, 0.5]]]
    for bad in (u.double(), u[0], u.numpy(), torch.zeros(1, 2, nu + 1)):
        with pytest.raises(ValueError, match="ctrl_bounds expects u_nom"):
            p.ctrl_bounds(bad)
