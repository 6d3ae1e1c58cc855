"""Cost rollouts of the physics layer (rsr_physics_cost_rollouts, Physics.cost_rollouts), host side only: the ABI, the entry point's
refusals ahead of its one launch, the op's place in the dispatch, the stage's header, and the Python surface with every bad input
refused before the C call.  The kernel is covered by tests/test_cost_rollouts_gpu.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_support import CSRC, HANDLE as H, ROOT, STREAM as S, body as _body, fields, header, ints, read as _read, record, refused, standin

SIG = ("int rsr_physics_cost_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, "
       "const rsr_feedback* fb /* NULL: open loop */, const rsr_param_samples* params, "
       "const rsr_cost* cost, int K, int T, int nsteps, int flags /* RSR_FB_* */, "
       "const rsr_rollout_out* traj /* NULL or all-NULL: nothing recorded */, "
       "const rsr_cost_out* out, void* hip_stream);")
REFS, WEIGHTS = ("qpos_ref", "qvel_ref", "ctrl_ref", "sensor_ref"), ("w_qpos", "w_qvel", "w_ctrl", "w_sensor")
OUTS = ("cost", "step_cost", "terms", "dx", "ctrl")


def test_header_declares_the_call_and_the_structs():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat                                             # (the declaration may break its lines)
    cost = flat[flat.index("typedef struct rsr_cost {"):flat.index("} rsr_cost;")]
    assert re.findall(r"\*\s*(\w+)[,;]", re.sub(r"/\*.*?\*/", "", cost)) == list(REFS + WEIGHTS) and cost.count("const float") == 5
    out = flat[flat.index("typedef struct rsr_cost_out {"):flat.index("} rsr_cost_out;")]
    assert re.findall(r"float \*(\w+);", out) == list(OUTS) and "const" not in out
    doc = h[h.index("/* Cost rollouts"):h.index("typedef struct rsr_cost {")]
    for word in ("rsr_physics_feedback_rollouts", "rsr_physics_param_rollouts", "bit for bit", "mj_differentiatePos", "exactly 0",
                 "after feedback and clamp", "sensordata row t", "wave_sum", "no contraction", "from +0", "qpos, qvel, ctrl, sensor",
                 "depend on that sample's inputs alone", "heavier row T-1", "weights >= 0", "no status word", "untouched",
                 "owns no buffer", "left alone, in every output", "before any device work", "RSR_FB_PER_SAMPLE or RSR_FB_CLAMP with fb NULL",
                 "all four weights NULL", "without qpos_ref", "no sensor table set", "RSR_ERR_UNSUPPORTED"):
        assert word in doc, word
    assert "rsr_physics_cost_rollouts <-" in h[:h.index("typedef")]                      # the opening list
    assert "rsr_cost" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_struct_sizes_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_cost_rollouts" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_cost_rollouts
    assert fn.argtypes is not None and len(fn.argtypes) == 14
    ptr = C.sizeof(C.c_void_p)
    assert [n for n, _ in _lib.Cost._fields_] == list(REFS + WEIGHTS) and C.sizeof(_lib.Cost) == 8 * ptr
    assert [n for n, _ in _lib.CostOut._fields_] == list(OUTS) and C.sizeof(_lib.CostOut) == 5 * ptr
    assert (_lib.COST_REFS, _lib.COST_WEIGHTS) == (REFS, WEIGHTS)
    # the device-side argument block carries the same thirteen pointers
    phys = _read("physics", "rsr_physics.hpp")
    assert "static_assert(sizeof(CostArgs) == 13 * sizeof(void*)" in phys
    cs, co = _lib.Cost(), _lib.CostOut()
    assert not any(fields(cs).values()) and not any(fields(co).values())
    ids = (C.c_int32 * 2)(0, 1)
    ctrl = (C.c_float * 8)()
    o, ps, fb = _lib.RolloutOut(), _lib.ParamSamples(), _lib.Feedback()
    for table, k in ((None, 0), (ids, 2)):
        for params in (None, C.byref(ps)):
            for f in (None, C.byref(fb)):
                for traj in (None, C.byref(o)):
                    assert fn(None, table, k, ctrl, f, params, C.byref(cs), 1, 1, 1, 0, traj, C.byref(co), None) == -1
                    assert b"rsr_physics_cost_rollouts: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every refusal comes ahead of the one device call (by source order, as a handle needs a device), and the call allocates
    nothing: the handle owns no buffer for it.  The entry's own checks, the refusals of all (slot, sample) rollouts (sample_grid,
    read in its place), the leaves', then the one launch of the op."""
    src = _read("physics", "rsr_physics.hip")
    entry = _body(src, "int rsr_physics_cost_rollouts")
    first = "if (const int rc = sample_grid(p, env_ids, count, K, T, nsteps, tr, who, &grid)) return rc;"
    assert entry.count(first) == 1 and "sweep_rollouts(" not in entry
    call = entry.replace(first, _body(src, "static int sample_grid"))
    dev = ("hipSetDevice", "hipMalloc", "hipMemset", "hipMemcpy", "hipDeviceSynchronize", "zeroed_once", "nominal_scratch(", "physics_args(", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_args(")
    checks = ("!p)", "!ctrl)", "fb && (!fb->gain || !fb->qpos_ref || !fb->qvel_ref)", "!fb && (flags & (RSR_FB_PER_SAMPLE | RSR_FB_CLAMP))",
              "!cost || !out || !out->cost", "!(cost->w_qpos || cost->w_qvel || cost->w_ctrl || cost->w_sensor)", "cost->w_qpos && !cost->qpos_ref",
              "out->dx && !cost->qpos_ref", "K < 1", "T < 1", "nsteps < 1", "flags & ~(RSR_FB_CTRL_PER_SAMPLE | RSR_FB_PER_SAMPLE | RSR_FB_CLAMP)",
              "(cost->w_sensor || cost->sensor_ref) && p->nsd == 0", "env_count(", "out->sensordata && p->nsd == 0", "grid > INT32_MAX",
              "(int64_t)T * nsteps > INT32_MAX", "f >= RSR_DR_BODY_IPOS")
    at = [call.index(c) for c in checks]
    assert at == sorted(at) and all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.count("RSR_ERR_ARG") == 13 and call.count("RSR_ERR_UNSUPPORTED") == 1 and call.rindex("fail(") < first_dev
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "hipDeviceSynchronize", "zeroed_once", "_buffer", "new ", "std::vector", "p->out", "p->sd"):
        assert k not in call, k
    # a null traj is a zeroed local, and the tail fills the three argument structs and sends the one op
    assert "const rsr_rollout_out none{};" in entry and "const rsr_rollout_out* tr = traj ? traj : &none;" in entry
    assert "rsr::SweepArgs sw{};" in entry and "sw.ctrl_out" not in re.sub(r"//.*", "", entry)
    assert "if (fb) { sw.fb_gain = fb->gain; sw.fb_qpos = fb->qpos_ref; sw.fb_qvel = fb->qvel_ref; }" in entry
    assert entry.index("physics_args(") < entry.index("x.ph.r = rsr::RollArgs{ctrl, T, tr->qpos") < entry.index("x.ph.sw = sw;") \
        < entry.index("x.ph.cs = rsr::CostArgs{cost->qpos_ref") < entry.index("physics_launch(")
    assert "out->cost, out->step_cost, out->terms, out->dx, out->ctrl};" in entry
    assert re.findall(r"\bOP_\w+", entry) == ["OP_COST_ROLLOUTS"] and entry.count("physics_launch(") == 1
    assert entry.rstrip().endswith("return counted(p, physics_launch(p, rsr::OP_COST_ROLLOUTS, x, who));")
    for part in (_body(src, "void rsr_physics_destroy"), src[src.index("struct rsr_physics {"):src.index("};")]):
        assert "cost" not in part.lower()
    assert set(re.findall(r"\b(\w*launch\w*)\(", src)) == {"launch", "launch_args", "physics_launch"}


def test_the_op_is_an_ordinary_op_and_the_kernel_a_header_of_its_own():
    phys = _read("physics", "rsr_physics.hpp")
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert re.findall(r"\bOP_COST\w*", enum) == ["OP_COST_ROLLOUTS"] and len(re.findall(r"\bOP_PHYS_\w+", enum)) == 9
    assert "struct CostArgs" in phys and re.search(r"\bCostArgs cs;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    kernels = _read("physics", "rsr_physics_kernels.hpp")
    assert '#include "rsr_cost.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    assert "const size_t lds = op == OP_COST_ROLLOUTS ? cost_lds_bytes<C>() : op == OP_IK ? ik_lds_bytes<C>() :" in lp
    assert "op == OP_PHYS_TRANSITION ? fd_lds_bytes<C>() : sizeof(Smem<C>)" in lp and lp.count("hipLaunchKernelGGL(") == 1
    assert ("if (op == OP_COST_ROLLOUTS) return ap ? go(sampled_kernel<C, WAVES, CostOp, Applied>, ph.p, ph.r, CostOp::Args{ph.sw, ph.cs}, ph.ap) : "
            "go(sampled_kernel<C, WAVES, CostOp>, ph.p, ph.r, CostOp::Args{ph.sw, ph.cs});") in lp
    assert lp.index("if (op == OP_COST_ROLLOUTS)") < lp.index("switch (op)") and "case OP_COST" not in lp
    assert lp.count("sampled_kernel<C, WAVES, CostOp") == 2 and lp.count("sampled_kernel<C, WAVES, SweepOp") == 2 and lp.count("sampled_kernel") == 6
    # the two argument structs travel as one, in the order and with the bytes they had as two kernel arguments
    assert "struct CostOp { struct Args { SweepArgs sw; CostArgs c; }; };" in re.sub(r"\s+", " ", _read("physics", "rsr_sample.hpp"))
    # nothing directly under csrc/ knows; the hashed sources are the parent's
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "sampled_kernel" not in text and "CostOp" not in text and "CostArgs" not in text and "OP_COST" not in text and "rsr_cost" not in text, f
    import bench
    import parity_envelopes as PE
    assert PE.ENV["_provenance"]["csrc_sha16"] == bench.csrc_sha16()
    # the stage and the accumulators' place are a header of their own; the kernel's text: tests/test_sampled_kernel_api.py
    assert "void cost_stage(" in _read("physics", "rsr_cost.hpp") and "cost_stage<C>(" in _read("physics", "rsr_sample.hpp")
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4q."):]
    for word in ("sampled_kernel", "CostOp", "cost_stage", "SweepOp", "wave_sum", "cost_lds_bytes", "VGPRs", "SGPR", "scratch", "cost_rollout_rates"):
        assert word in sec, word
    assert design.index("### 4p.") < design.index("### 4q.")
    assert "cost_rollouts(" in open(os.path.join(ROOT, "README.md")).read()
    assert "Physics.cost_rollouts(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import _lib, physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.cost_rollouts)
    assert list(sig.parameters) == ["self", "ctrl", "cost", "feedback", "params", "nsteps", "fields", "env_ids", "clamp", "out", "K",
                                    "step_cost", "terms", "residual"]
    d = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "ctrl", "cost")}
    assert d == dict(feedback=None, params=None, nsteps=None, fields=(), env_ids=None, clamp=False, out=None, K=None, step_cost=False,
                     terms=False, residual=False)
    assert "Physics.cost_rollouts(ctrl, cost)" in physics.__doc__
    # the siblings are as they were
    assert list(inspect.signature(Physics.feedback_rollouts).parameters) == ["self", "ctrl", "gain", "qpos_ref", "qvel_ref", "params", "nsteps",
                                                                             "fields", "env_ids", "clamp", "out", "K"]
    nu, nq, nv, nsd = 3, 5, 4, 7
    p = standin(handle=None, nq=nq, nv=nv, nsensordata=nsd)
    bare = standin(handle=None, nq=nq, nv=nv)              # no sensors set
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, K, T = 4, 2, 3
    c3, c4 = z(M, T, nu), z(M, K, T, nu)
    full = dict(qpos_ref=z(M, T, nq), qvel_ref=z(M, T, nv), ctrl_ref=z(M, T, nu), sensor_ref=z(M, T, nsd),
                w_qpos=z(M, T, nv), w_qvel=z(M, T, nv), w_ctrl=z(M, T, nu), w_sensor=z(M, T, nsd))
    wv = dict(w_qvel=full["w_qvel"])
    fb3 = dict(gain=z(M, T, nu, 2 * nv), qpos_ref=z(M, T, nq), qvel_ref=z(M, T, nv))
    fb4 = dict(gain=z(M, K, T, nu, 2 * nv), qpos_ref=z(M, K, T, nq), qvel_ref=z(M, K, T, nv))
    sh = dict(ctrl=c4, cost=full)
    cases = [(dict(sh, ctrl=z(M, nu)), "expects ctrl"),                                                  # ctrl as feedback_rollouts
             (dict(sh, ctrl=z(M, K, T, nu + 1)), "expects ctrl"),
             (dict(sh, ctrl=c4.double()), "expects ctrl"),
             (dict(sh, ctrl=c4[:3]), "expects ctrl"),
             (dict(sh, ctrl=c3), "K is not given"),
             (dict(sh, ctrl=c3, K=0), "K must be >= 1"),
             (dict(sh, K=5), "K = 5"),
             (dict(sh, cost=None), "cost must be a dict"),                                               # cost
             (dict(sh, cost=dict(full, w_time=z(M, T, 1))), r"cost has \['w_time'\]"),
             (dict(sh, cost={k: v for k, v in full.items() if k in REFS}), "cost gives no weight"),
             (dict(sh, cost=dict(w_qpos=None, qpos_ref=full["qpos_ref"])), "cost gives no weight"),
             (dict(sh, cost=dict(w_qpos=full["w_qpos"])), r"cost\['qpos_ref'\] is needed by w_qpos"),
             (dict(sh, cost=wv, residual=True), r"cost\['qpos_ref'\] is needed by residual=True"),
             (dict(sh, cost=dict(full, w_qpos=z(M, T, nq))), r"cost\['w_qpos'\]"),
             (dict(sh, cost=dict(full, w_qvel=z(M, K, T, nv))), r"cost\['w_qvel'\]"),
             (dict(sh, cost=dict(full, w_ctrl=z(M, T + 1, nu))), r"cost\['w_ctrl'\]"),
             (dict(sh, cost=dict(full, w_sensor=z(M, T, nsd + 1))), r"cost\['w_sensor'\]"),
             (dict(sh, cost=dict(full, qpos_ref=z(M, T, nv))), r"cost\['qpos_ref'\]"),
             (dict(sh, cost=dict(full, qvel_ref=z(M, T, nv).double())), r"cost\['qvel_ref'\]"),
             (dict(sh, cost=dict(full, ctrl_ref=z(M, T, nu, device="meta"))), r"cost\['ctrl_ref'\]"),
             (dict(sh, cost=dict(full, sensor_ref=z(M, T, nsd).numpy())), r"cost\['sensor_ref'\]"),
             (dict(sh, cost=dict(full, w_qvel=z(M - 1, T, nv))), r"cost\['w_qvel'\]"),
             (dict(sh, feedback=(1, 2, 3)), "feedback must be None or a dict"),                          # feedback
             (dict(sh, feedback={k: v for k, v in fb3.items() if k != "qvel_ref"}), "feedback must be None or a dict"),
             (dict(sh, feedback=dict(fb3, qpos_ref=None)), "feedback must be None or a dict"),
             (dict(sh, feedback=dict(fb3, gain=z(M, T, nu, nv))), r"expects feedback\['gain'\]"),
             (dict(sh, feedback=dict(fb3, qpos_ref=fb4["qpos_ref"])), r"expects feedback\['qpos_ref'\]"),
             (dict(sh, feedback=dict(fb4, qvel_ref=fb3["qvel_ref"])), r"expects feedback\['qvel_ref'\]"),
             (dict(sh, feedback=dict(fb3, gain=z(M, T + 1, nu, 2 * nv))), "T = 4, 3, 3"),
             (dict(sh, feedback=dict(fb4, qpos_ref=z(M, K + 1, T, nq))), "K = 2, 3, 2"),
             (dict(sh, feedback={k: v[:, :1].expand(-1, 3, *v.shape[2:]) for k, v in fb4.items()}), "feedback has K = 3"),
             (dict(sh, clamp=True), "clamp=True needs feedback"),
             (dict(sh, params=dict(mass=z(M, K, 3))), "not a model leaf"),                               # params as param_rollouts
             (dict(sh, params=dict(body_mass=z(M, K + 1, 3))), "K = 3"),
             (dict(sh, params=dict(qpos0=z(M, K, nq))), "Go2 models only"),
             (dict(sh, fields=("qpos", "qacc")), "unknown"),                                             # fields, nsteps, env_ids, out
             (dict(sh, nsteps=0), "nsteps must be >= 1"),
             (dict(sh, env_ids=[0, 2]), "expects ctrl"),
             (dict(sh, env_ids=[0, 4]), "env_ids must lie in"),
             (dict(sh, out={"cost": z(M, K, 1)}), r"out\['cost'\]"),
             (dict(sh, step_cost=True, out={"step_cost": z(M, K, T).double()}), r"out\['step_cost'\]"),
             (dict(sh, terms=True, out={"terms": z(M, K, 3)}), r"out\['terms'\]"),
             (dict(sh, residual=True, out={"dx": z(M, K, T, nv)}), r"out\['dx'\]"),
             (dict(sh, fields=("ctrl",), out={"ctrl": z(M, T, nu)}), r"out\['ctrl'\]")]
    refused(monkeypatch, p.cost_rollouts, cases)
    no_table = [(dict(sh, cost=dict(wv, w_sensor=z(M, T, 0))), "no sensors are set"),
                (dict(sh, cost=dict(wv, sensor_ref=z(M, T, 0))), "no sensors are set"),
                (dict(sh, cost=wv, fields=("sensordata",)), "no sensors are set")]
    refused(monkeypatch, bare.cost_rollouts, no_table)
    # the good calls get as far as the C call: the stand-in has no handle, and the library refuses it
    for kw in (sh, dict(sh, cost=wv), dict(ctrl=c3, cost=wv, K=2), dict(ctrl=c3, cost=full, feedback=fb4), dict(sh, feedback=fb3, clamp=True),
               dict(sh, params=dict(body_mass=z(M, K, 3)), step_cost=True, terms=True, residual=True, fields=("qpos", "ctrl", "sensordata"))):
        with pytest.raises(RuntimeError, match="rsr_physics_cost_rollouts: null handle"):
            p.cost_rollouts(**kw)
    with pytest.raises(RuntimeError, match="rsr_physics_cost_rollouts: null handle"):
        bare.cost_rollouts(c4, wv)


def test_the_structs_the_call_carries(monkeypatch):
    """The one library call: the pointers of the three structs, the flags, K and T, and the inputs held by identity."""
    import torch
    from rsr_mjx_amd import _lib
    nu, nq, nv, nsd = 3, 6, 5, 4
    p, rec = standin(nsensordata=nsd), record(monkeypatch)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    ptrs = lambda struct, **want: fields(struct) == {n: (want[n].data_ptr() if n in want else None) for n, _ in struct._fields_}
    M, K, T = 4, 2, 3
    c4 = z(M, K, T, nu)
    full = dict(qpos_ref=z(M, T, nq), qvel_ref=z(M, T, nv), ctrl_ref=z(M, T, nu), sensor_ref=z(M, T, nsd),
                w_qpos=z(M, T, nv), w_qvel=z(M, T, nv), w_ctrl=z(M, T, nu), w_sensor=z(M, T, nsd))
    res = p.cost_rollouts(c4, full)
    (sym, (h, ids, k, cp, fb, ps, cs, Kc, Tc, nsteps, flags, traj, co, s)), = rec.calls
    assert (sym, h, ids, k, cp, fb, Kc, Tc, nsteps, flags, s) == ("rsr_physics_cost_rollouts", H, None, 0, c4.data_ptr(), None, K, T, 2,
                                                                  _lib.FB_CTRL_PER_SAMPLE, S)
    assert ptrs(cs, **full) and not any(ps.leaf) and ptrs(traj) and ptrs(co, cost=res["cost"])
    assert list(res) == ["cost"] and tuple(res["cost"].shape) == (M, K) and res["cost"].dtype == torch.float32
    assert all(any(t is x for x in p._held["cost_rollouts"]) for t in (c4, *full.values()))
    rec.calls.clear()
    # everything at once, on listed envs, with the caller's tensors
    c3, mass = z(2, T, nu), z(2, K, 3)
    fbk = dict(gain=z(2, K, T, nu, 2 * nv), qpos_ref=z(2, K, T, nq), qvel_ref=z(2, K, T, nv))
    cost = dict(w_ctrl=z(2, T, nu), w_qpos=z(2, T, nv), qpos_ref=z(2, T, nq), qvel_ref=None)
    mine = {"cost": z(2, K), "dx": z(2, K, T, 2 * nv), "ctrl": z(2, K, T, nu), "qvel": z(2, K, T, nv)}
    res = p.cost_rollouts(c3, cost, feedback=fbk, params=dict(body_mass=mass), nsteps=4, fields=("qvel", "ctrl", "ncon"), env_ids=[3, 0], clamp=True,
                          out=mine, step_cost=True, terms=True, residual=True)
    (sym, (h, ids, k, cp, fb, ps, cs, Kc, Tc, nsteps, flags, traj, co, s)), = rec.calls
    assert (k, cp, Kc, Tc, nsteps, flags) == (2, c3.data_ptr(), K, T, 4, _lib.FB_PER_SAMPLE | _lib.FB_CLAMP) and ints(ids, 2) == [3, 0]
    assert ptrs(fb, **fbk) and ps.leaf[_lib.DR_FIELDS.index("body_mass")] == mass.data_ptr()
    assert ptrs(cs, w_ctrl=cost["w_ctrl"], w_qpos=cost["w_qpos"], qpos_ref=cost["qpos_ref"])
    assert ptrs(traj, qvel=mine["qvel"], ncon=res["ncon"])
    assert ptrs(co, cost=mine["cost"], step_cost=res["step_cost"], terms=res["terms"], dx=mine["dx"], ctrl=mine["ctrl"])
    assert list(res) == ["cost", "step_cost", "terms", "dx", "qvel", "ctrl", "ncon"]
    assert all(res[f] is mine[f] for f in mine)
    assert [tuple(res[f].shape) for f in ("step_cost", "terms", "dx", "ncon")] == [(2, K, T), (2, K, 4), (2, K, T, 2 * nv), (2, K, T, 1)]
    assert all(any(t is x for x in p._held["cost_rollouts"]) for t in (c3, mass, *fbk.values(), cost["w_ctrl"], cost["w_qpos"], cost["qpos_ref"]))
    rec.calls.clear()
    # shared gain rows and a shared ctrl: no flag, K from the caller; an empty list: no call
    fb3 = dict(gain=z(M, T, nu, 2 * nv), qpos_ref=z(M, T, nq), qvel_ref=z(M, T, nv))
    p.cost_rollouts(z(M, T, nu), dict(w_qvel=full["w_qvel"]), feedback=fb3, K=3)
    (_, a), = rec.calls
    assert (a[7], a[8], a[10]) == (3, T, 0)
    rec.calls.clear()
    res = p.cost_rollouts(z(0, K, T, nu), dict(w_qvel=z(0, T, nv)), env_ids=[])
    assert rec.calls == [] and tuple(res["cost"].shape) == (0, K)
