"""Closed-loop rollouts of the physics layer (rsr_physics_feedback_rollouts, Physics.feedback_rollouts), host side only: the ABI,
the entry point's refusals ahead of its one launch, the stage's header, and the Python surface with every bad input refused before
the C call.  The kernel is covered by tests/test_feedback_gpu.py."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_support import CSRC, ROOT, body as _body, header, read as _read, record, refused, standin

SIG = ("int rsr_physics_feedback_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, "
       "const rsr_feedback* fb, const rsr_param_samples* params, int K, int T, int nsteps, "
       "int flags, const rsr_rollout_out* out, float* ctrl_out, void* hip_stream);")


def test_header_declares_the_call_the_struct_and_the_flags():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat                                             # (the declaration may break its lines)
    assert "typedef struct rsr_feedback { const float* gain; const float* qpos_ref; const float* qvel_ref; } rsr_feedback;" in flat
    for name, bit in (("RSR_FB_CTRL_PER_SAMPLE", 1), ("RSR_FB_PER_SAMPLE", 2), ("RSR_FB_CLAMP", 4)):
        assert re.search(rf"#define {name}\s+{bit}\b", h), name
    doc = h[h.index("/* Closed-loop rollouts"):h.index("typedef struct rsr_feedback")]
    for word in ("mj_differentiatePos", "[M, T, nu, 2 nv]", "[M, T, nq]", "[M, T, nv]", "[M, K, T, nu]", "one fp32 fma per term",
                 "actuator_ctrllimited", "ctrl_out", "untouched", "owns no buffer", "before any device work", "unknown flag bits",
                 "RSR_ERR_UNSUPPORTED", "rsr_physics_param_rollouts", "rsr_physics_transition_fd"):
        assert word in doc, word
    assert "rsr_physics_feedback_rollouts <-" in h[:h.index("typedef")]                  # the opening list
    assert "rsr_feedback" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_feedback_rollouts" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_feedback_rollouts
    assert fn.argtypes is not None and len(fn.argtypes) == 13
    assert (_lib.FB_CTRL_PER_SAMPLE, _lib.FB_PER_SAMPLE, _lib.FB_CLAMP) == (1, 2, 4)
    fb = _lib.Feedback()
    assert [n for n, _ in _lib.Feedback._fields_] == ["gain", "qpos_ref", "qvel_ref"] and C.sizeof(fb) == 3 * C.sizeof(C.c_void_p)
    assert not (fb.gain or fb.qpos_ref or fb.qvel_ref)
    ids = (C.c_int32 * 2)(0, 1)
    ctrl = (C.c_float * 8)()
    o, ps = _lib.RolloutOut(), _lib.ParamSamples()
    for table, k in ((None, 0), (ids, 2)):
        for params in (None, C.byref(ps)):
            for applied in (None, ctrl):
                assert fn(None, table, k, ctrl, C.byref(fb), params, 1, 1, 1, 0, C.byref(o), applied, None) == -1
                assert b"rsr_physics_feedback_rollouts: null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every refusal comes ahead of the one device call (by source order, as a handle needs a device), and the call allocates
    nothing: the handle owns no buffer for it.  Its own checks, then the tail it shares with the parameter rollout's entry."""
    src = _read("physics", "rsr_physics.hip")
    entry, tail = _body(src, "int rsr_physics_feedback_rollouts"), _body(src, "static int sweep_rollouts")
    first = "if (const int rc = sample_grid(p, env_ids, count, sw.K, T, nsteps, out, who, &grid)) return rc;"
    assert first in tail
    tail = tail.replace(first, _body(src, "static int sample_grid"))                       # the shared refusals, read in their place
    assert entry.rstrip().endswith('return sweep_rollouts(p, env_ids, count, ctrl, params, sw, T, nsteps, out, hip_stream, "rsr_physics_feedback_rollouts");')
    assert "OP_PHYS_" not in entry
    call = entry + tail
    dev = ("hipSetDevice", "hipMalloc", "hipMemset", "hipMemcpy", "zeroed_once", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_launch(") + len("physics_")
    checks = ("!p)", "!ctrl)", "!fb || !fb->gain || !fb->qpos_ref || !fb->qvel_ref)", "!out)",
              "!ctrl_out && !(out->qpos || out->qvel || out->time || out->actuator_force || out->ncon || out->sensordata)",
              "K < 1", "T < 1", "nsteps < 1", "flags & ~(RSR_FB_CTRL_PER_SAMPLE | RSR_FB_PER_SAMPLE | RSR_FB_CLAMP)", "env_count(",
              "out->sensordata && p->nsd == 0", "grid > INT32_MAX", "(int64_t)T * nsteps > INT32_MAX", "RSR_ERR_UNSUPPORTED",
              "f >= RSR_DR_BODY_IPOS")
    at = [call.index(c) for c in checks]
    assert all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert call.count("RSR_ERR_ARG") == 9 and call.count("RSR_ERR_UNSUPPORTED") == 1 and call.count("physics_launch(") == 1
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "_buffer", "new ", "std::vector"):
        assert k not in call, k
    assert "_alloc" not in src and src.count("static int zeroed_once(") == 1
    for k in ("sw.fb_gain = fb->gain", "sw.fb_qpos = fb->qpos_ref", "sw.fb_qvel = fb->qvel_ref", "sw.ctrl_out = ctrl_out",
              "sw.fb_per_sample = (flags & RSR_FB_PER_SAMPLE) != 0", "sw.fb_clamp = (flags & RSR_FB_CLAMP) != 0",
              "sw.ctrl_per_sample = (flags & RSR_FB_CTRL_PER_SAMPLE) != 0"):
        assert k in entry and entry.index(k) < entry.index("sweep_rollouts("), k          # the entry's own, ahead of the shared tail
    # the open-loop call zero-initialises the arguments and sets no feedback member
    assert "rsr::SweepArgs sw{};" in call
    assert "rsr::SweepArgs sw{};" in _body(src, "int rsr_physics_param_rollouts") and "fb_" not in _body(src, "int rsr_physics_param_rollouts")


def test_the_stage_is_a_header_of_its_own_called_twice():
    fb = _read("physics", "rsr_feedback.hpp")
    code = re.sub(r"//.*", "", fb)
    assert "void feedback_ctrl(" in code and "differentiate_pos<C>(" in code
    for k in ("asm", "atomic", "hipMalloc", "_kernel("):
        assert k not in fb, k
    assert not re.search(r"\brec\[[^\]]*\]\s*=[^=]", code)
    # a fence first, the shuffles outside every lane condition, one fma per term in index order, the clamp by the model's arrays
    body = code[code.index("void feedback_ctrl("):]
    assert body.index("WSYNC();") < body.index("differentiate_pos<C>(") < body.index("__shfl(dq, i)") < body.index("__shfl(dv, i)")
    assert body.count("__builtin_fmaf(") == 2 and body.index("__shfl(dv, i)") < body.index("if (lane < C::NU)")
    assert "m.actuator_ctrllimited[j]" in body and "m.actuator_ctrlrange[2 * j]" in body and "m.actuator_ctrlrange[2 * j + 1]" in body
    assert "sw.fb_clamp" in body and "if (sw.ctrl_out) sw.ctrl_out[out_row * C::NU + lane] = u;" in body
    hdr = _read("physics", "rsr_physics.hpp")
    for k in ("const float* fb_gain;", "const float* fb_qpos;", "const float* fb_qvel;", "float* ctrl_out;", "int fb_per_sample;", "int fb_clamp;"):
        assert k in hdr, k
    # the two calls, each under `if (sw.fb_gain)` inside the kernel's SWEEP switch: tests/test_sampled_kernel_api.py
    assert '#include "rsr_feedback.hpp"' in _read("physics", "rsr_sweep.hpp")
    kern = re.sub(r"//.*", "", _read("physics", "rsr_sample.hpp"))
    assert len(re.findall(r"^\s*if \(sw\.fb_gain\) feedback_ctrl<C>\(m, hot, s, sw, ", kern, re.M)) == 2 == kern.count("feedback_ctrl")
    # the family units and the other ops' headers do not know
    for f in ("rsr_physics_kernels.hpp", "rsr_transition.hpp", "rsr_inverse.hpp"):
        assert "feedback" not in _read("physics", f).lower(), f
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            assert "feedback" not in open(os.path.join(CSRC, f)).read().lower(), f
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4k."):]
    for word in ("feedback_ctrl", "sampled_kernel", "differentiate_pos", "VGPRs", "feedback_rollout_rates"):
        assert word in sec, word


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.feedback_rollouts)
    assert list(sig.parameters) == ["self", "ctrl", "gain", "qpos_ref", "qvel_ref", "params", "nsteps", "fields", "env_ids", "clamp", "out", "K"]
    d = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "ctrl", "gain", "qpos_ref", "qvel_ref")}
    assert d == dict(params=None, nsteps=None, fields=("qpos", "qvel", "time"), env_ids=None, clamp=False, out=None, K=None)
    assert "Physics.feedback_rollouts(ctrl, gain, qpos_ref, qvel_ref)" in physics.__doc__
    assert "4 * M * K * T * w bytes" in Physics.feedback_rollouts.__doc__ and '"ctrl"' in Physics.feedback_rollouts.__doc__
    # the siblings are as they were
    assert list(inspect.signature(Physics.param_rollouts).parameters) == ["self", "ctrl", "params", "nsteps", "fields", "env_ids", "out"]
    assert list(inspect.signature(Physics.sample_rollouts).parameters) == ["self", "ctrl", "nsteps", "fields", "env_ids", "out"]
    # every bad input is refused before the C call: the recording library sees none
    nu, nq, nv = 3, 5, 4
    p = standin(handle=None, nq=nq, nv=nv)                  # (kind 0: an Airbot model; no sensors set)
    z = lambda *s, **kw: torch.zeros(s, **kw)
    M, K, T = 4, 2, 3
    c3, c4 = z(M, T, nu), z(M, K, T, nu)
    g4, q3, v3 = z(M, T, nu, 2 * nv), z(M, T, nq), z(M, T, nv)
    g5, q4, v4 = z(M, K, T, nu, 2 * nv), z(M, K, T, nq), z(M, K, T, nv)
    sh = dict(ctrl=c4, gain=g4, qpos_ref=q3, qvel_ref=v3)                                               # a good call: K from ctrl
    ps = dict(ctrl=c3, gain=g5, qpos_ref=q4, qvel_ref=v4)                                               # a good one: K from the rows
    mass = z(M, K, 3)
    cases = [(dict(sh, ctrl=z(M, nu)), "expects ctrl"),                                                  # ranks
             (dict(sh, ctrl=z(M, K, T, nu, 1)), "expects ctrl"),
             (dict(sh, gain=z(M, nu, 2 * nv)), "expects gain"),
             (dict(sh, gain=z(M, K, K, T, nu, 2 * nv)), "expects gain"),
             (dict(sh, qpos_ref=z(M, nq)), "expects qpos_ref"),
             (dict(sh, qvel_ref=z(M, nv)), "expects qvel_ref"),
             (dict(sh, qpos_ref=q4), "expects qpos_ref"),                                                # refs not of the gain's rank
             (dict(sh, qvel_ref=v4), "expects qvel_ref"),
             (dict(ps, qpos_ref=q3), "expects qpos_ref"),
             (dict(ps, qvel_ref=v3), "expects qvel_ref"),
             (dict(sh, ctrl=z(M, K, T, nu + 1)), "expects ctrl"),                                        # nu, nv, nq
             (dict(sh, gain=z(M, T, nu + 1, 2 * nv)), "expects gain"),
             (dict(sh, gain=z(M, T, nu, 2 * nv + 1)), "expects gain"),
             (dict(sh, gain=z(M, T, nu, nv)), "expects gain"),
             (dict(sh, qpos_ref=z(M, T, nv)), "expects qpos_ref"),
             (dict(sh, qvel_ref=z(M, T, nq)), "expects qvel_ref"),
             (dict(sh, gain=z(M, T + 1, nu, 2 * nv)), "T = 4"),                                          # T
             (dict(sh, qpos_ref=z(M, T - 1, nq)), "T = 3, 2, 3"),
             (dict(sh, qvel_ref=z(M, T + 2, nv)), "T = 3, 3, 5"),
             (dict(ps, ctrl=z(M, K + 1, T, nu)), "K = 2"),                                               # K
             (dict(ps, qpos_ref=z(M, K + 1, T, nq)), "K = 3"),
             (dict(ps, qvel_ref=z(M, K + 2, T, nv)), "K = 4"),
             (dict(ps, K=5), "K = 5"),
             (dict(sh, params=dict(body_mass=z(M, K + 1, 3))), "K = 3"),
             (dict(sh, ctrl=c3), "K is not given"),                                                      # nothing says K
             (dict(sh, ctrl=c3, K=0), "K must be >= 1"),
             (dict(sh, ctrl=c3[:3]), "expects ctrl"),                                                    # M
             (dict(sh, gain=g4[:3]), "expects gain"),
             (dict(sh, qpos_ref=q3[:3]), "expects qpos_ref"),
             (dict(sh, qvel_ref=v3[:3]), "expects qvel_ref"),
             (dict(sh, env_ids=[0, 2]), "expects ctrl"),
             (dict(sh, env_ids=[0, 4]), "env_ids must lie in"),
             (dict(sh, ctrl=c4.double()), "expects ctrl"),                                               # dtype
             (dict(sh, gain=g4.double()), "expects gain"),
             (dict(sh, qpos_ref=q3.double()), "expects qpos_ref"),
             (dict(sh, qvel_ref=v3.half()), "expects qvel_ref"),
             (dict(sh, ctrl=z(M, K, T, nu, device="meta")), "expects ctrl"),                            # device
             (dict(sh, gain=z(M, T, nu, 2 * nv, device="meta")), "expects gain"),
             (dict(sh, qpos_ref=z(M, T, nq, device="meta")), "expects qpos_ref"),
             (dict(sh, qvel_ref=z(M, T, nv, device="meta")), "expects qvel_ref"),
             (dict(sh, gain=g4.numpy()), "expects gain"),                                                # not a tensor
             (dict(sh, params=dict(mass=mass)), "not a model leaf"),                                     # params as param_rollouts
             (dict(sh, params=dict(body_mass=z(M, K, 4))), r"params\['body_mass'\]"),
             (dict(sh, params=dict(qpos0=z(M, K, nq))), "Go2 models only"),
             (dict(sh, fields=("qpos", "qacc")), "unknown"),                                             # fields
             (dict(sh, fields=()), "no fields"),
             (dict(sh, fields=("sensordata",)), "no sensors are set"),
             (dict(sh, nsteps=0), "nsteps must be >= 1"),
             (dict(sh, out={"qpos": z(M, K, T, nv)}), "out\\['qpos'\\]"),
             (dict(sh, fields=("ctrl",), out={"ctrl": z(M, T, nu)}), "out\\['ctrl'\\]"),
             (dict(sh, out={"qpos": z(M, K, T, nq).numpy()}), "out\\['qpos'\\]")]                       # (once an AttributeError)
    refused(monkeypatch, p.feedback_rollouts, cases)
    # the good calls get as far as the C call: the stand-in has no handle, and the library refuses it
    for kw in (sh, ps, dict(sh, ctrl=c3, K=2), dict(sh, fields=("ctrl",)), dict(sh, params=dict(body_mass=mass), clamp=True)):
        with pytest.raises(RuntimeError, match="rsr_physics_feedback_rollouts: null handle"):
            p.feedback_rollouts(**kw)
    # ... as the one library call, with the inputs kept in the method's own slot, not copied
    rec = record(monkeypatch)
    p.feedback_rollouts(**dict(sh, params=dict(body_mass=mass)))
    (sym, args), = rec.calls
    assert sym == "rsr_physics_feedback_rollouts" and len(args) == 13 and args[3] == c4.data_ptr()
    assert all(any(t is x for x in p._held["feedback_rollouts"]) for t in (c4, g4, q3, v3, mass))
