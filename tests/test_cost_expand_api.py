"""The cost expansion (rsr_physics_cost_expand, Physics.cost_expand, Physics.differentiate_state), host side only: the ABI, the entry
point's refusals ahead of its first device call, the kernel's header and dispatch, and the Python surface with every bad input
refused before the C call.  The kernel is covered by tests/test_cost_expand_gpu.py, the numpy reference it is held against by
tests/test_cost_expand_ref.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_support import CSRC, HANDLE as H, ROOT, STREAM as S, body as _body, fields, header, read as _read, record, refused, standin

SIG = ("int rsr_physics_cost_expand(rsr_physics* p, int M, int T, const float* columns, int row_stride, int ny, const rsr_cost* cost, "
       "const rsr_cost_nominal* nominal, const rsr_cost_expansion* out, void* hip_stream);")
OUTS = ("lx", "lu", "lxx", "luu", "lux")


def test_header_declares_the_call_and_the_structs():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat
    assert "typedef struct rsr_cost_nominal { const float* dx; const float* ctrl; const float* sensordata; } rsr_cost_nominal;" in flat
    assert "typedef struct rsr_cost_expansion { float* lx; float* lu; float* lxx; float* luu; float* lux; } rsr_cost_expansion;" in flat
    doc = re.sub(r"\n \*\s+", " ", h[h.index("/* Cost expansion"):h.index("typedef struct rsr_cost_nominal")])
    for word in ("rsr_physics_cost_rollouts", "rsr_physics_trajectory_fd", "rsr_physics_lqr_backward", "rsr_lqr_cost", "[M, T, ncol, row_stride]",
                 "C_t[j][a] = columns[s, t, a, nx + j]", "D_t[j][p] = columns[s, t, nx + p, nx + j]", "never read", "[M, T, nx]", "[M, T+1, nx]",
                 "[M, T+1, nx, nx]", "[M, T, nu, nx]", "qpos_ref and qvel_ref are not read", "index t+1", "Row 0", "row T", "terminal cost",
                 "every element of all five is written", "Gauss-Newton", "exact Hessian", "right-multiplied perturbation", "identity",
                 "first order in the rotation error", "mj_differentiatePos", "second derivatives are dropped", "positive semi-definite",
                 "no contraction", "j = 0 .. ny-1 ascending", "depends on its own inputs alone, bit for bit", "whatever M is",
                 # guarantee 1
                 "the single fp32 product w . dx[t] bit for bit", "one subtraction and one product", "exactly diagonal", "exactly +0",
                 # guarantee 2
                 "symmetric bit for bit", "(c_a c_b) commutes",
                 # side effects and refusals
                 "Only the five buffers of out are written", "untouched", "owns no buffer", "no env_ids", "neither the model nor the record",
                 "before any device work", "a null handle, cost, nominal or out", "a NULL member of out", "M < 1 or T < 1",
                 "ny outside [0, RSR_MAX_SENSORDATA]", "no weight given at all", "w_qpos or w_qvel without nominal->dx",
                 "w_ctrl without nominal->ctrl", "w_sensor with ny == 0", "without nominal->sensordata or without columns",
                 "row_stride < nx + ny when columns is read", "2^31"):
        assert word in doc, word
    assert "rsr_physics_cost_expand <-" in h[:h.index("typedef")]                        # the opening list
    assert h.index("int rsr_physics_lqr_box(") < h.index("/* Cost expansion") < h.index("/* Kalman filter")
    assert "rsr_cost" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_cost_expand" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_cost_expand
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    ptr = C.sizeof(C.c_void_p)
    assert [n for n, _ in _lib.CostNominal._fields_] == ["dx", "ctrl", "sensordata"] and C.sizeof(_lib.CostNominal) == 3 * ptr
    assert [n for n, _ in _lib.CostExpansion._fields_] == list(OUTS) and C.sizeof(_lib.CostExpansion) == 5 * ptr
    assert [n for n, _ in _lib.CostExpansion._fields_] == [n for n, _ in _lib.LqrCost._fields_]       # passed straight on
    cs, nom, out = _lib.Cost(), _lib.CostNominal(), _lib.CostExpansion()
    assert not any(fields(nom).values()) and not any(fields(out).values())
    buf = (C.c_float * 8)()
    for c in (None, C.byref(cs)):
        for n in (None, C.byref(nom)):
            for o in (None, C.byref(out)):
                assert fn(None, 1, 1, buf, 8, 1, c, n, o, None) == -1
                assert b"rsr_physics_cost_expand: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every RSR_ERR_ARG check of the entry comes ahead of its first device call (by source order, as a handle needs a device); the
    call owns no buffer, and its one launch is an op of its own with the one argument struct."""
    src = _read("physics", "rsr_physics.hip")
    call = _body(src, "int rsr_physics_cost_expand")
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "nominal_scratch(",
           "physics_args(", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_args(")
    checks = ("!p)", "!cost || !nominal || !out)", "!out->lx || !out->lu || !out->lxx || !out->luu || !out->lux)", "M < 1 || T < 1",
              "ny < 0 || ny > RSR_MAX_SENSORDATA", "!(cost->w_qpos || cost->w_qvel || cost->w_ctrl || cost->w_sensor)",
              "(cost->w_qpos || cost->w_qvel) && !nominal->dx", "cost->w_ctrl && !nominal->ctrl", "cost->w_sensor && ny == 0",
              "cost->w_sensor && (!nominal->sensordata || !columns)", "cost->w_sensor && row_stride < 2 * d.nv + ny",
              "(int64_t)M * ((int64_t)T + 1) > INT32_MAX")
    at = [call.index(c) for c in checks]
    assert at == sorted(at) and all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.count("RSR_ERR_ARG") == len(checks) and call.rindex("RSR_ERR_ARG") < first_dev
    assert "cost->ctrl_ref" in call and "!cost->ctrl_ref" not in call and "!cost->sensor_ref" not in call      # (optional)
    assert "qpos_ref" not in call and "qvel_ref" not in call                                                    # (not read)
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipDeviceSynchronize", "zeroed_once", "p->nominal", "env_count(", "counted("):
        assert k not in call, k
    assert re.findall(r"\bOP_\w+", call) == ["OP_EXPAND"] and call.count("physics_launch(") == 1
    assert sorted(set(re.findall(r"\bx\.ph\.(\w+)", call))) == ["ex"]
    assert "physics_args(p, nullptr, nullptr, M * (T + 1), 1, hip_stream)" in call                             # the grid
    assert "expan" not in _body(src, "void rsr_physics_destroy") and "expan" not in src[src.index("struct rsr_physics {"):src.index("};")]


def test_the_kernel_is_a_header_of_its_own():
    kern = _read("physics", "rsr_expand.hpp")
    code = re.sub(r"//.*", "", kern)
    assert "void expand_kernel(const DModel* __restrict__, Layout, StepArgs, ExpandArgs q)" in code
    assert "template <class C, int WAVES>" in code and "__launch_bounds__(64)" in code and "struct ExpandDims" in code
    body = code[code.index("void expand_kernel("):]
    # C gives NV and NU and nothing else; the model, the layout and the record are not read
    assert set(re.findall(r"\bC::(\w+)", code)) == {"NV", "NU"}
    for w in ("a.state", "Smem<", "forward<C>", "integrate<C>", "asm", "atomic", "mfma", "double", "fmaf", "frcp("):
        assert w not in body, w
    assert "#pragma clang fp contract(off)" in body and "extern __shared__" in body and "expand_lds_bytes" in code
    assert body.count("__restrict__") == 1                       # (the unused model pointer's: no buffer of q is declared unaliased)
    # only the five outputs are stored to
    assert set(re.findall(r"\bq\.(\w+)\[[^\]]*\] = ", body)) == set(OUTS)
    # the dispatch: an op of the physics enum, its struct a field of the launch's, its LDS image chosen next to the others'
    phys = _read("physics", "rsr_physics.hpp")
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert re.findall(r"\bOP_EXPAND\w*", enum) == ["OP_EXPAND"] and "struct ExpandArgs" in phys
    assert re.search(r"\bExpandArgs ex;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    kernels = _read("physics", "rsr_physics_kernels.hpp")
    assert '#include "rsr_expand.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    assert "op == OP_EXPAND ? expand_lds_bytes<C>() :" in lp and lp.count("hipLaunchKernelGGL(") == 1
    assert "if (op == OP_EXPAND) return go(expand_kernel<C, WAVES>, ph.ex);" in lp and lp.count("expand_kernel") == 1
    assert lp.index("if (op == OP_EXPAND)") < lp.index("switch (op)") and "case OP_EXPAND" not in lp
    assert "hipFuncSetAttribute" not in kernels and "MaxDynamicSharedMemorySize" not in kernels
    # nothing outside physics/ knows
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "expand_kernel" not in text and "ExpandArgs" not in text and "OP_EXPAND" not in text and "rsr_expand" not in text, f
    for f in os.listdir(os.path.join(CSRC, "physics")):
        if f not in ("rsr_expand.hpp", "rsr_physics.hpp", "rsr_physics_kernels.hpp", "rsr_physics.hip") and f.endswith((".hip", ".hpp")):
            text = _read("physics", f)
            assert "expand_kernel" not in text and "ExpandArgs" not in text and "OP_EXPAND" not in text, f
    # every family's LDS image, as ExpandDims counts it: two vectors of 64 and 64 rows of LD floats, LD / 4 odd
    for nv, nu in ((20, 5), (18, 12), (14, 5)):
        nc = 2 * nv + nu
        ld = ((nc + 7) & ~7) + 4
        assert nc <= 64 and ld % 4 == 0 and (ld // 4) % 2 == 1 and 4 * (2 * 64 + 64 * ld) <= 16 * 1024, (nv, nu)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.index("### 4s.") < design.index("### 4t.")
    sec = re.sub(r"\s+", " ", design[design.index("### 4t."):])
    for word in ("expand_kernel", "Gauss-Newton", "first order in the rotation error", "bit for bit", "across lanes", "bank", "VGPRs", "SGPR", "scratch",
                 "LDS", "cost_expand_rates", "einsum", "cost_expand_tolerances.json"):
        assert word in sec, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert readme.index("#### Cost rollouts") < readme.index("#### Cost expansion")
    sub = readme[readme.index("#### Cost expansion"):]
    sub = re.sub(r"\s+", " ", sub[:sub.index("\n#### ", 10)])
    for word in ("cost_rollouts(", "trajectory_fd(", "cost_expand(", "lqr_backward(", "residual=True", "differentiate_state(", "first order in the rotation error"):
        assert word in sub, word
    assert "tangent(" not in readme                                                  # the examples no longer leave the cost model to the reader
    assert "Physics.cost_expand(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import _lib, physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.cost_expand)
    assert list(sig.parameters) == ["self", "cost", "dx", "ctrl", "sensordata", "columns", "out"]
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("self", "cost")} == dict(dx=None, ctrl=None, sensordata=None, columns=None, out=None)
    assert list(inspect.signature(Physics.differentiate_state).parameters) == ["self", "qpos", "qvel", "qpos_ref", "qvel_ref"]
    assert "Physics.cost_expand(cost, dx, ctrl, sensordata, columns)" in physics.__doc__ and "Physics.differentiate_state" in physics.__doc__
    doc = re.sub(r"\s+", " ", Physics.cost_expand.__doc__)
    for word in ("[M, T, nx]", "[M, T+1, nx]", "[M, T+1, nx, nx]", "[M, T, nu, nx]", "cost_rollouts", "residual=True", "trajectory_fd", "lqr_backward",
                 "Gauss-Newton", "first order in the rotation error", "accepted and ignored", "bit for bit", "differentiate_state"):
        assert word in doc, word
    # the neighbours are as they were
    assert list(inspect.signature(Physics.lqr_backward).parameters) == ["self", "columns", "lx", "lu", "lxx", "luu", "lux", "mu", "state_reg",
                                                                        "values", "out"]
    nu, nq, nv, ny = 3, 5, 4, 7
    p = standin(handle=None, nq=nq, nv=nv)                     # (no sensor table: the call does not ask the handle for one)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, T, nx = 6, 3, 2 * nv
    ncol, w = nx + nu, nx + ny + 2
    full = dict(qpos_ref=z(M, T, nq), qvel_ref=z(M, T, nv), ctrl_ref=z(M, T, nu), sensor_ref=z(M, T, ny),
                w_qpos=z(M, T, nv), w_qvel=z(M, T, nv), w_ctrl=z(M, T, nu), w_sensor=z(M, T, ny))
    good = dict(cost=full, dx=z(M, T, nx), ctrl=z(M, T, nu), sensordata=z(M, T, ny), columns=z(M, T, ncol, w))
    wv = dict(w_qvel=full["w_qvel"])
    cases = [(dict(good, cost=None), "cost must be a dict"),
             (dict(good, cost=dict(full, w_time=z(M, T, 1))), r"cost has \['w_time'\]"),
             (dict(good, cost={k: v for k, v in full.items() if not k.startswith("w_")}), "cost gives no weight"),
             (dict(good, cost=dict(w_qpos=None, ctrl_ref=full["ctrl_ref"])), "cost gives no weight"),
             (dict(good, cost=dict(full, w_qpos=z(M, T, nq))), r"cost\['w_qpos'\]"),
             (dict(good, cost=dict(full, w_qvel=z(M, T + 1, nv))), r"cost\['w_qvel'\]"),
             (dict(good, cost=dict(full, w_ctrl=z(M - 1, T, nu))), r"cost\['w_ctrl'\]"),
             (dict(good, cost=dict(full, w_sensor=z(M, T, 0))), r"cost\['w_sensor'\]"),
             (dict(good, cost=dict(full, w_sensor=z(M, T, 65))), r"cost\['w_sensor'\]"),
             (dict(good, cost=dict(full, sensor_ref=z(M, T, ny + 1))), r"cost\['sensor_ref'\]"),
             (dict(good, cost=dict(full, ctrl_ref=z(M, T, nu).double())), r"cost\['ctrl_ref'\]"),
             (dict(good, cost=dict(full, w_qpos=z(M, T, nv, device="meta"))), r"cost\['w_qpos'\]"),
             (dict(good, cost=dict(full, w_qpos=z(M, T, nv).numpy())), r"cost\['w_qpos'\]"),
             (dict(good, cost=dict(w_qvel=z(0, T, nv))), r"cost\['w_qvel'\]"),                         # M
             (dict(good, cost=dict(w_qvel=z(M, 0, nv))), r"cost\['w_qvel'\]"),                         # T
             (dict(good, cost=dict(w_qvel=z(1, 1, nv).expand(2 ** 30, 1, nv))), "below 2\\^31"),
             (dict(good, dx=None), "expects dx"),
             (dict(good, dx=z(M, T, nv)), "expects dx"),
             (dict(good, dx=z(M, T, nx + 1)[..., :nx]), "expects dx"),                                 # contiguity
             (dict(good, ctrl=None), "expects ctrl"),
             (dict(good, ctrl=z(M, T + 1, nu)), "expects ctrl"),
             (dict(good, sensordata=None), "expects sensordata"),
             (dict(good, sensordata=z(M, T, ny).double()), "expects sensordata"),
             (dict(good, columns=None), "expects columns"),
             (dict(good, columns=z(M, T, ncol, nx + ny - 1)), "expects columns"),                      # row_stride
             (dict(good, columns=z(M, T, ncol + 1, w)), "expects columns"),
             (dict(good, columns=z(M, T, ncol, w + 1)[..., :w]), "expects columns"),
             (dict(good, out={"Vx": z(M, T + 1, nx)}), r"out has \['Vx'\]"),
             (dict(good, out={"lx": z(M, T, nx)}), r"out\['lx'\]"),
             (dict(good, out={"lux": z(M, T, nx, nu)}), r"out\['lux'\]"),
             (dict(good, out={"luu": z(M, T, nu, nu).double()}), r"out\['luu'\]")]
    refused(monkeypatch, p.cost_expand, cases)
    # the good calls get as far as the C call: the stand-in has no handle, and the library refuses it
    for kw in (good, dict(cost=wv, dx=good["dx"]), dict(cost=dict(w_ctrl=full["w_ctrl"]), ctrl=good["ctrl"]),
               dict(cost=dict(wv, sensor_ref=z(M, T, 99)), dx=good["dx"], columns="not read"),          # what no term needs is not looked at
               dict(good, cost=dict(full, w_sensor=z(M, T, 64), sensor_ref=None), sensordata=z(M, T, 64), columns=z(M, T, ncol, nx + 64))):
        with pytest.raises(RuntimeError, match="rsr_physics_cost_expand: null handle"):
            p.cost_expand(**kw)
    # the one library call, on the caller's very tensors, held in the method's own slot
    p, rec = standin(nq=nq, nv=nv), record(monkeypatch)
    res = p.cost_expand(**good)
    (sym, (h, m, t, col, stride, n, cs, nom, out, s)), = rec.calls
    assert (sym, h, m, t, col, stride, n, s) == ("rsr_physics_cost_expand", H, M, T, good["columns"].data_ptr(), w, ny, S)
    ptrs = lambda struct, **want: fields(struct) == {k: (want[k].data_ptr() if k in want else None) for k, _ in struct._fields_}
    assert ptrs(cs, **{k: v for k, v in full.items() if k not in ("qpos_ref", "qvel_ref")})              # (the state references: not passed)
    assert ptrs(nom, dx=good["dx"], ctrl=good["ctrl"], sensordata=good["sensordata"]) and ptrs(out, **res)
    assert list(res) == list(OUTS) and [tuple(v.shape) for v in res.values()] == [(M, T + 1, nx), (M, T, nu), (M, T + 1, nx, nx), (M, T, nu, nu), (M, T, nu, nx)]
    held = [good[k] for k in ("dx", "ctrl", "sensordata", "columns")] + [v for k, v in full.items() if k not in ("qpos_ref", "qvel_ref")]
    assert all(any(x is y for y in p._held["cost_expand"]) for x in held)
    # its result passes straight on
    rec.calls.clear()
    p.lqr_backward(good["columns"], **res)
    assert rec.calls[0][0] == "rsr_physics_lqr_backward" and ptrs(rec.calls[0][1][5], **res)
    # the sensor term off: no columns, ny = 0, and the caller's outputs
    rec.calls.clear()
    mine = {"lxx": z(M, T + 1, nx, nx)}
    res = p.cost_expand(wv, dx=good["dx"], columns=good["columns"], out=mine)
    (_, (h, m, t, col, stride, n, cs, nom, out, s)), = rec.calls
    assert (col, stride, n) == (None, 0, 0) and ptrs(cs, w_qvel=full["w_qvel"]) and ptrs(nom, dx=good["dx"]) and res["lxx"] is mine["lxx"]
