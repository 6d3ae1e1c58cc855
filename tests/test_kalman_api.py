"""The Kalman filter and smoother (rsr_physics_kalman, Physics.kalman_smooth) and Physics.integrate_state, host side only: the ABI,
the entry point's refusals ahead of its first device call, the kernel's header and dispatch, and the Python surface with every bad
input refused before the C call.  The kernel is covered by tests/test_kalman_gpu.py, the numpy reference it is held against by
tests/test_kalman_ref.py."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import ik_ref
from api_support import CSRC, ROOT, body as _body, header, read as _read, record, refused, standin

SIG = ("int rsr_physics_kalman(rsr_physics* p, int M, int T, const float* columns, int row_stride, int ny, const rsr_kalman_in* in, "
       "int flags, const rsr_kalman_out* out, void* hip_stream);")


def test_header_declares_the_call_and_the_structs():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat
    assert ("typedef struct rsr_kalman_in { const float* dy; const float* r; const float* q; const float* x0; const float* P0; } "
            "rsr_kalman_in;") in flat
    assert ("typedef struct rsr_kalman_out { float* xf; float* pf; float* xs; float* ps; float* nll; float* status; } "
            "rsr_kalman_out;") in flat
    doc = re.sub(r"\n \*\s+", " ", h[h.index("/* Kalman filter and smoother"):h.index("typedef struct rsr_kalman_in")])
    for word in ("[M, T, ncol, row_stride]", "A_t[i][j]", "C_t[r][j]", "never read", "RSR_MAX_SENSORDATA", "nx + ny <= row_stride",
                 "dx_{t+1} = A_t dx_t + w_t", "dy_t = C_t dx_t + v_t", "[M, T, ny]", "[M, T, nx]", "[M, nx, nx]", "+inf", "may be NULL",
                 "one sensor entry at a time", "logf(s)", "Rauch-Tung-Striebel", "Cholesky", "the same bits", "[M, T+1, nx]",
                 "[M, T+1, nx, nx]", "status [M, 2]", "left alone", "keep what was written", "nll[s] = 0", "bit for bit", "no env_ids",
                 "neither the model nor the record", "untouched", "owns no buffer", "before any device work", "xs or ps without pf",
                 "ps without xs", "row_stride < 2 nv + ny", "flags must be 0", "2^31"):
        assert word in doc, word
    assert "rsr_physics_kalman  <-" in h[:h.index("typedef")]                            # the opening list
    assert "rsr_kalman" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_kalman" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_kalman
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    ins, out = _lib.KalmanIn(), _lib.KalmanOut()
    assert [n for n, _ in _lib.KalmanIn._fields_] == ["dy", "r", "q", "x0", "P0"] and C.sizeof(ins) == 5 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _lib.KalmanOut._fields_] == ["xf", "pf", "xs", "ps", "nll", "status"] and C.sizeof(out) == 6 * C.sizeof(C.c_void_p)
    assert not any(getattr(ins, n) for n, _ in _lib.KalmanIn._fields_) and not any(getattr(out, n) for n, _ in _lib.KalmanOut._fields_)
    buf = (C.c_float * 8)()
    for i in (None, C.byref(ins)):
        for o in (None, C.byref(out)):
            assert fn(None, 1, 1, buf, 8, 1, i, 0, o, None) == -1
            assert b"rsr_physics_kalman: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every RSR_ERR_ARG check of the entry comes ahead of its first device call (by source order, as a handle needs a device); the
    call owns no buffer, and its one launch is an op of its own with the one argument struct."""
    src = _read("physics", "rsr_physics.hip")
    call = _body(src, "int rsr_physics_kalman")
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "nominal_scratch(",
           "physics_args(", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_args(")
    checks = ("!p)", "!columns || !in || !out)", "!in->dy || !in->r || !in->q || !in->P0)", "!out->xf || !out->status)",
              "(out->xs || out->ps) && !out->pf", "out->ps && !out->xs", "M < 1 || T < 1", "ny < 1 || ny > RSR_MAX_SENSORDATA",
              "row_stride < 2 * d.nv + ny", "flags != 0", "(int64_t)M * ((int64_t)T + 1) > INT32_MAX")
    at = [call.index(c) for c in checks]
    assert at == sorted(at) and all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.count("RSR_ERR_ARG") == len(checks) and call.rindex("RSR_ERR_ARG") < first_dev
    assert "in->x0" in call and "!in->x0" not in call and "!out->nll" not in call                 # (the optional members)
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipDeviceSynchronize", "zeroed_once", "p->nominal", "env_count(", "counted("):
        assert k not in call, k
    assert re.findall(r"\bOP_\w+", call) == ["OP_KALMAN"] and call.count("physics_launch(") == 1
    assert sorted(set(re.findall(r"\bx\.ph\.(\w+)", call))) == ["kf"]
    assert "kalman" not in _body(src, "void rsr_physics_destroy") and "kalman" not in src[src.index("struct rsr_physics {"):src.index("};")]


def test_the_kernel_is_a_header_of_its_own():
    kern = _read("physics", "rsr_kalman.hpp")
    code = re.sub(r"//.*", "", kern)
    assert "void kalman_kernel(" in code and "template <class C, int WAVES>" in code and "__launch_bounds__(64)" in code
    assert "struct KalmanDims" in code and '#include "rsr_lqr.hpp"' in code
    body = code[code.index("void kalman_kernel("):]
    # C gives NV and NU and nothing else; the model, the layout and the record are not read
    assert set(re.findall(r"\bC::(\w+)", code)) == {"NV", "NU"}
    assert "void kalman_kernel(const DModel* __restrict__, Layout, StepArgs, KalmanArgs q)" in code
    for w in ("a.state", "Smem<", "forward<C>", "integrate<C>", "atomic", "mfma", "double", "frcp(", "frsq("):
        assert w not in body, w
    # the shared pieces are the Riccati pass's, not copies
    for w in ("lds4(", "fma4(", "row_dot<NX>("):
        assert w in code, w
    for w in ("float4 lds4(", "void fma4(", "float row_dot(", "float dot4("):
        assert w not in code, w
    assert "LqrDims<C>::LD" in code
    assert "1.0f / sqrtf(d)" in body and "!(d > 0.0f) || !(d < __builtin_inff())" in body
    assert "rj == __builtin_inff()" in body and "rj > 0.0f && s > 0.0f && s < __builtin_inff()" in body
    assert "q.status[2 * slot] = (float)t;" in body and "q.status[2 * slot + 1] = (float)t;" in body and "q.status[2 * slot] = -1.0f;" in body
    assert "extern __shared__" in body and "kalman_lds_bytes" in code
    # the image stays under the 64 KB a plain launch may ask for, by the compiler's own arithmetic; the launcher raises no limit
    assert "static_assert(sizeof(float) * FLOATS <= 64 * 1024" in code
    # the smoother's loads of xf and pf stand behind the drained stores
    fence = body.index('__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup")')
    wait = body.index('asm volatile("s_waitcnt vmcnt(0)" ::: "memory")')
    acq = body.index('__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup")')
    first_load = min(body.index("get_mat(P, q.pf"), body.index("= q.xf["))
    last_store = body.index("put_mat(q.pf + (slot * (T + 1) + T)")
    assert last_store < fence < wait < acq < first_load
    assert body.count("__restrict__") == 1                       # (the unused model pointer's: no buffer of q is declared unaliased)
    # the dispatch: an op of the physics enum, its struct a field of the launch's, its LDS image chosen next to the others'
    phys = _read("physics", "rsr_physics.hpp")
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert re.findall(r"\bOP_KALMAN\w*", enum) == ["OP_KALMAN"] and "struct KalmanArgs" in phys
    assert len(re.findall(r"\bOP_PHYS_\w+", enum)) == 9
    assert re.search(r"\bKalmanArgs kf;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    kernels = _read("physics", "rsr_physics_kernels.hpp")
    assert '#include "rsr_kalman.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    assert "op == OP_KALMAN ? kalman_lds_bytes<C>(x.ph.kf.xs != nullptr) :" in lp and lp.count("hipLaunchKernelGGL(") == 1
    assert "if (op == OP_KALMAN) return go(kalman_kernel<C, WAVES>, ph.kf);" in lp and lp.count("kalman_kernel") == 1
    assert lp.index("if (op == OP_KALMAN)") < lp.index("switch (op)") and "case OP_KALMAN" not in lp
    assert "hipFuncSetAttribute" not in kernels and "MaxDynamicSharedMemorySize" not in kernels
    # nothing outside physics/ knows
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "kalman" not in text.lower() and "OP_KALMAN" not in text, f
    for f in os.listdir(os.path.join(CSRC, "physics")):
        if f not in ("rsr_kalman.hpp", "rsr_physics.hpp", "rsr_physics_kernels.hpp", "rsr_physics.hip") and f.endswith((".hip", ".hpp")):
            assert "kalman" not in _read("physics", f).lower(), f
    # every family's LDS image, as KalmanDims counts it
    for nv in (20, 18, 14):
        nx = 2 * nv
        ib = nx // 4
        ld = nx + (0 if ib & 1 else 4)
        grp = 64 // ib
        floats, filter_floats = 8 * 64 + 8 * nx * ld, 8 * 64 + 4 * nx * ld + 64 * ld
        assert (ld // 4) % 2 == 1 and grp * ib <= 64 and grp * -(-ib // grp) >= ib and filter_floats <= floats and 4 * floats <= 64 * 1024, nv
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4r."):]
    for word in ("kalman_kernel", "LD", "ds_read_b128", "VGPRs", "scratch", "kalman_rates", "torch loop", "vmcnt(0)"):
        assert word in sec, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert readme.index("LQR backward pass") < readme.index("Kalman filter and smoother")
    sub = readme[readme.index("#### Kalman filter and smoother"):]
    sub = sub[:sub.index("\n#### ", 10)]
    for word in ("set_state(", "trajectory_fd(", "sample_rollouts(", "kalman_smooth(", "integrate_state(", "Gauss", "K = 1"):
        assert word in sub, word
    assert "kalman_smooth" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.kalman_smooth)
    assert list(sig.parameters) == ["self", "columns", "dy", "r", "q", "P0", "x0", "smooth", "covariances", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(x0=None, smooth=True, covariances=False, out=None)
    assert list(inspect.signature(Physics.integrate_state).parameters) == ["self", "qpos", "qvel", "dx"]
    assert "Physics.kalman_smooth(columns, dy, r, q, P0)" in physics.__doc__ and "Physics.integrate_state" in physics.__doc__
    doc = Physics.kalman_smooth.__doc__
    for word in ("[M, T, ncol, w]", "[M, T, ny]", "[M, ny]", "[M, T, nx]", "[M, nx]", "[M, nx, nx]", "[M, T+1, nx]", "[M, T+1, nx, nx]",
                 "trajectory_fd", "sample_rollouts", "+inf", "status [M, 2]", "nll [M]", "Rauch-Tung-Striebel", "bit for bit",
                 "integrate_state"):
        assert word in doc, word
    # the neighbours are as they were
    assert list(inspect.signature(Physics.lqr_backward).parameters) == ["self", "columns", "lx", "lu", "lxx", "luu", "lux", "mu", "state_reg",
                                                                        "values", "out"]
    # every bad input is refused before the C call: the recording library sees none
    nu, nq, nv = 3, 5, 4
    p = standin(handle=None, nq=nq, nv=nv)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, T, nx, ny = 6, 3, 2 * nv, 5                               # (M is the buffers', not num_envs)
    ncol, w = nx + nu, nx + ny
    good = dict(columns=z(M, T, ncol, w), dy=z(M, T, ny), r=z(M, T, ny), q=z(M, T, nx), P0=z(M, nx, nx))
    cases = [(dict(good, columns=z(M, T, ncol)), "expects columns"),                                    # rank
             (dict(good, columns=z(M, T, ncol + 1, w)), "expects columns"),                             # ncol
             (dict(good, columns=z(M, T, ncol, nx)), "expects columns"),                                # ny = 0
             (dict(good, columns=z(M, T, ncol, nx + 65), dy=z(M, T, 65), r=z(M, T, 65)), "expects columns"),   # ny > 64
             (dict(good, columns=z(M, 0, ncol, w)), "expects columns"),                                 # T
             (dict(good, columns=z(0, T, ncol, w)), "expects columns"),                                 # M
             (dict(good, columns=z(M, T, ncol, w).double()), "expects columns"),                        # dtype
             (dict(good, columns=z(M, T, ncol, w, device="meta")), "expects columns"),                  # device
             (dict(good, columns=z(M, T, ncol, w).numpy()), "expects columns"),                         # not a tensor
             (dict(good, columns=z(M, T, ncol, w + 1)[..., :w]), "expects columns"),                    # contiguity
             (dict(good, dy=z(M, T + 1, ny)), "expects dy"),
             (dict(good, dy=z(M, T, ny + 1)), "expects dy"),
             (dict(good, dy=z(M, ny)), "expects dy"),                                                   # (only r and q broadcast)
             (dict(good, dy=z(M, T, ny).double()), "expects dy"),
             (dict(good, dy=None), "expects dy"),
             (dict(good, r=z(M, T, nx)), "expects r"),
             (dict(good, r=z(M - 1, ny)), "expects r"),
             (dict(good, r=z(ny)), "expects r"),
             (dict(good, r=1.0), "expects r"),
             (dict(good, r=z(M, T, ny, device="meta")), "expects r"),
             (dict(good, q=z(M, T, ny)), "expects q"),
             (dict(good, q=z(M, nx + 1)[:, :nx]), "expects q"),
             (dict(good, q=z(M, T, nx).numpy()), "expects q"),
             (dict(good, P0=z(M, nx)), "expects P0"),
             (dict(good, P0=z(M, nx, nx).transpose(1, 2)), "expects P0"),                               # contiguity
             (dict(good, P0=z(M, nx, nx + 1)[..., :nx]), "expects P0"),
             (dict(good, P0=None), "expects P0"),
             (dict(good, x0=z(M, nx + 1)), "expects x0"),
             (dict(good, x0=z(M, nx).double()), "expects x0"),
             (dict(good, x0=z(nx)), "expects x0"),
             (dict(good, smooth=False, covariances=True), "covariances=True needs smooth=True"),
             (dict(good, out={"xf": z(M, T, nx)}), "out\\['xf'\\]"),
             (dict(good, out={"Pf": z(M, T + 1, nx, nx).double()}), "out\\['Pf'\\]"),
             (dict(good, out={"xs": z(M, T + 1, nx + 1)[..., :nx]}), "out\\['xs'\\]"),
             (dict(good, out={"nll": z(M, 1)}), "out\\['nll'\\]"),
             (dict(good, out={"status": z(M)}), "out\\['status'\\]"),
             (dict(good, out={"status": z(M, 2).numpy()}), "out\\['status'\\]"),
             (dict(good, covariances=True, out={"Ps": z(M, T, nx, nx)}), "out\\['Ps'\\]"),
             (dict(good, out={"Ps": z(M, T + 1, nx, nx)}), "out has \\['Ps'\\]"),                        # (covariances=False)
             (dict(good, smooth=False, out={"xs": z(M, T + 1, nx)}), "out has \\['xs'\\]"),              # (smooth=False)
             (dict(good, out={"P": z(M, T + 1, nx, nx)}), "out has \\['P'\\]")]
    refused(monkeypatch, p.kalman_smooth, cases)
    # the good calls get as far as the C call: the stand-in has no handle, and the library refuses it
    for kw in (good, dict(good, x0=z(M, nx), covariances=True), dict(good, r=z(M, ny), q=z(M, nx)), dict(good, smooth=False),
               dict(good, columns=z(M, T, ncol, nx + 1), dy=z(M, T, 1), r=z(M, T, 1)),
               dict(good, columns=z(M, T, ncol, nx + 64), dy=z(M, T, 64), r=z(M, 64)),
               dict(good, covariances=True, out={"xf": z(M, T + 1, nx), "Pf": z(M, T + 1, nx, nx), "xs": z(M, T + 1, nx),
                                                 "Ps": z(M, T + 1, nx, nx), "nll": z(M), "status": z(M, 2)})):
        with pytest.raises(RuntimeError, match="rsr_physics_kalman: null handle"):
            p.kalman_smooth(**kw)
    # ... as the one library call, on the caller's very tensors: they are kept in the method's own slot, none of them copied
    rec = record(monkeypatch)
    kw = dict(good, x0=z(M, nx))
    res = p.kalman_smooth(**kw)
    (sym, args), = rec.calls
    assert sym == "rsr_physics_kalman" and len(args) == 10 and args[1:3] == (M, T) and args[3] == kw["columns"].data_ptr()
    assert args[4:6] == (w, ny) and args[7] == 0
    assert [n for n, _ in args[6]._fields_ if getattr(args[6], n) == kw[n].data_ptr()] == ["dy", "r", "q", "x0", "P0"]
    assert list(res) == ["xf", "Pf", "xs", "nll", "status"]
    assert (args[8].xf, args[8].pf, args[8].xs, args[8].ps, args[8].nll, args[8].status) == \
        (res["xf"].data_ptr(), res["Pf"].data_ptr(), res["xs"].data_ptr(), None, res["nll"].data_ptr(), res["status"].data_ptr())
    assert [tuple(t.shape) for t in res.values()] == [(M, T + 1, nx), (M, T + 1, nx, nx), (M, T + 1, nx), (M,), (M, 2)]
    assert all(any(t is x for x in p._held["kalman_smooth"]) for t in kw.values())
    # smooth=False: no xs pointer, so no smoother; covariances: ps
    rec.calls.clear()
    res = p.kalman_smooth(**dict(good, smooth=False))
    assert list(res) == ["xf", "Pf", "nll", "status"] and rec.calls[0][1][8].xs is None and rec.calls[0][1][8].ps is None
    rec.calls.clear()
    res = p.kalman_smooth(**dict(good, covariances=True))
    assert list(res) == ["xf", "Pf", "xs", "Ps", "nll", "status"] and rec.calls[0][1][8].ps == res["Ps"].data_ptr()
    # r and q per slot are expanded on the host to rows per step, and the expanded tensors are held too
    rec.calls.clear()
    r2, q2 = torch.arange(M * ny, dtype=torch.float32).reshape(M, ny), torch.arange(M * nx, dtype=torch.float32).reshape(M, nx)
    p.kalman_smooth(**dict(good, r=r2, q=q2))
    ins = rec.calls[0][1][6]
    held = {t.data_ptr(): t for t in p._held["kalman_smooth"] if torch.is_tensor(t)}
    assert ins.r != r2.data_ptr() and tuple(held[ins.r].shape) == (M, T, ny) and held[ins.r].is_contiguous()
    assert torch.equal(held[ins.r], r2[:, None].expand(M, T, ny)) and torch.equal(held[ins.q], q2[:, None].expand(M, T, nx))


def _model(kind):
    from model_variants import envdef_of
    return envdef_of(kind, None).sys.arrays


@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_integrate_state_is_mj_integrate_pos(kind):
    """On CPU tensors against tests/ik_ref.integrate_pos: the cube scene (hinges, slides and free bodies) and the Go2 (a free
    base), any leading dims, the free joints' quaternions of unit length."""
    import torch
    from rsr_mjx_amd.physics import Physics
    A = _model(kind)
    nq, nv = int(A["jnt_qposadr"][-1]) + (7 if int(A["jnt_type"][-1]) == 0 else 1), int(A["jnt_dofadr"][-1]) + (6 if int(A["jnt_type"][-1]) == 0 else 1)
    assert any(int(t) == 0 for t in A["jnt_type"])
    p = Physics.__new__(Physics)
    p.dims = types.SimpleNamespace(nq=nq, nv=nv)
    p.env = types.SimpleNamespace(sys=types.SimpleNamespace(arrays=A))
    rng = np.random.default_rng(4)
    n = 12
    q = rng.normal(size=(n, nq))
    for j in range(len(A["jnt_type"])):
        if int(A["jnt_type"][j]) == 0:
            qa = int(A["jnt_qposadr"][j])
            q[:, qa + 3:qa + 7] /= np.linalg.norm(q[:, qa + 3:qa + 7], axis=1, keepdims=True)
    v, dx = rng.normal(size=(n, nv)), 0.3 * rng.normal(size=(n, 2 * nv))
    want = q.copy()
    ik_ref.integrate_pos(A, want, dx[:, :nv].copy(), np.ones(nv, bool))
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    q1, v1 = p.integrate_state(t(q), t(v), t(dx))
    assert np.abs(q1.numpy() - want).max() < 1e-12 and np.abs(v1.numpy() - (v + dx[:, nv:])).max() == 0
    assert not np.shares_memory(q1.numpy(), q)
    # fp32, and leading dims [3, 4]
    f = lambda a: torch.as_tensor(a, dtype=torch.float32).reshape(3, 4, -1)
    q2, v2 = p.integrate_state(f(q), f(v), f(dx))
    assert tuple(q2.shape) == (3, 4, nq) and tuple(v2.shape) == (3, 4, nv) and q2.dtype == torch.float32
    assert np.abs(q2.reshape(n, nq).numpy() - want).max() < 2e-6
    for j in range(len(A["jnt_type"])):
        if int(A["jnt_type"][j]) == 0:
            qa = int(A["jnt_qposadr"][j])
            assert np.abs(q2[..., qa + 3:qa + 7].norm(dim=-1).numpy() - 1).max() < 3e-7
    # a zero deviation of a unit-quaternion state is the state
    q3, v3 = p.integrate_state(t(q), t(v), torch.zeros(n, 2 * nv, dtype=torch.float64))
    assert np.abs(q3.numpy() - q).max() < 1e-15 and torch.equal(v3, t(v))
    for bad, msg in (((t(q)[:, :-1], t(v), t(dx)), "expects qpos"), ((t(q), t(v), t(dx)[:, :-1]), "expects dx"),
                     ((t(q), t(v)[:3], t(dx)), "same leading dims"), ((q, t(v), t(dx)), "expects qpos")):
        with pytest.raises(ValueError, match=msg):
            p.integrate_state(*bad)
