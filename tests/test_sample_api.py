"""Sampled rollouts of the physics layer (rsr_physics_sample_rollouts, Physics.sample_rollouts), host side only: the ABI, the
dispatch and the Python surface.  The kernel's text is covered by tests/test_sampled_kernel_api.py, the kernel by tests/test_sample_gpu.py."""
import ctypes as C
import inspect
import os
import re

from api_support import CSRC, HANDLE, ROOT, STREAM, body as _body, header, ints, record, refused, standin

SIG = ("int rsr_physics_sample_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, "
       "int K, int T, int nsteps, const rsr_rollout_out* out, void* hip_stream);")


def test_header_declares_the_sample_api():
    h = header()
    assert SIG in re.sub(r"\s+", " ", h)                          # (the declaration may break its line)
    doc = h[h.index("/* Sampled rollouts"):h.index("int rsr_physics_sample_rollouts(")]
    for word in ("[M, K, T, nu]", "[M, K, T, width]", "bit for bit", "qacc_warmstart", "position in env_ids", "untouched",
                 "no PRNG key advances", "left alone", "before any device work", "2^31"):
        assert word in doc, word
    assert h.count("typedef struct rsr_rollout_out") == 1          # the existing struct, not a second one
    from rsr_mjx_amd import _lib, physics
    assert len(_lib.PHYS_FIELDS) == 7 and len(_lib.DYNAMICS_FIELDS) == 6 and len(_lib.CONSTRAINT_FIELDS) == 7
    assert len(_lib.TRANSITION_FIELDS) == 3 and tuple(n for n, _ in _lib.RolloutOut._fields_) == physics.ROLLOUT_FIELDS


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_sample_rollouts" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_sample_rollouts
    assert fn.argtypes is not None and len(fn.argtypes) == 9
    ids = (C.c_int32 * 2)(0, 1)
    ctrl = (C.c_float * 8)()
    o = _lib.RolloutOut()
    for table, k in ((None, 0), (ids, 2), (ids, 0)):
        assert fn(None, table, k, ctrl, 1, 1, 1, C.byref(o), None) == -1
        assert b"null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every refusal of rsr_physics_sample_rollouts is RSR_ERR_ARG ahead of every device call (by source order, as a handle needs
    a device), and the call allocates nothing: the handle owns no buffer for it.  The refusals it shares with the two sweep
    entries are a helper's (sample_grid), read here in the place of its call."""
    src = open(os.path.join(CSRC, "physics", "rsr_physics.hip")).read()
    call = _body(src, "int rsr_physics_sample_rollouts")
    shared = "if (const int rc = sample_grid(p, env_ids, count, K, T, nsteps, out, who, &grid)) return rc;"
    assert call.count(shared) == 1
    call = call.replace(shared, _body(src, "static int sample_grid"))
    dev = ("hipSetDevice", "hipMalloc", "hipMemset", "hipMemcpy", "zeroed_once", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert "launch(" in call and first_dev == call.index("physics_launch(") + len("physics_")
    checks = ("!p)", "!ctrl)", "!out ||", "out->qpos || out->qvel || out->time || out->actuator_force || out->ncon || out->sensordata)",
              "K < 1", "T < 1", "nsteps < 1", "env_count(", "out->sensordata && p->nsd == 0", "grid > INT32_MAX",
              "(int64_t)T * nsteps > INT32_MAX")
    at = [call.index(c) for c in checks]
    assert all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]
    assert "(int64_t)n * K" in call and call.count("RSR_ERR_ARG") == 6
    assert "count < 1" in _body(src, "static int env_count")
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "_buffer", "new ", "std::vector"):
        assert k not in call, k
    assert "_alloc" not in src and src.count("static int zeroed_once(") == 1
    # the dispatch: its own op with its own fields, filled after the arguments physics_args shares; no other op's field is touched
    assert "rsr::OP_PHYS_SAMPLE" in call and len(re.findall(r"\bOP_PHYS_\w+", call)) == 1
    assert call.index("physics_args(") < call.index("x.ph.r = rsr::RollArgs{ctrl, T, ") < call.index("x.ph.K = K;") < call.index("physics_launch(")
    assert sorted(set(re.findall(r"\bx\.ph\.(\w+)", call))) == ["K", "r"]


def test_nothing_outside_the_physics_layer_knows():
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "sampled_kernel" not in text and "SampleOp" not in text and "rsr_sample" not in text and "OP_PHYS_SAMPLE" not in text, f
    kernels = open(os.path.join(CSRC, "physics", "rsr_physics_kernels.hpp")).read()
    assert '#include "rsr_sample.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    # the op's own case, up to the next case label: the one (slot, sample) kernel as this op's, plain and applied, with p, r and
    # K, and no other kernel or op
    case = re.search(r"case OP_PHYS_SAMPLE:(.*?)\n\s*(?:case |default:)", lp, re.S).group(1)
    assert case.count("sampled_kernel<C, WAVES, SampleOp, Applied>, ph.p, ph.r, ph.K, ph.ap)") == 1 and case.count("sampled_kernel<C, WAVES, SampleOp>, ph.p, ph.r, ph.K)") == 1
    assert re.findall(r"\b\w+_kernel\b", case) == ["sampled_kernel"] * 2 and lp.count("SampleOp") == 2 and re.findall(r"\b\w+Op\b", case) == ["SampleOp"] * 2
    assert lp.count("sampled_kernel") == 6                              # three ops, plain and applied
    assert lp.count("hipLaunchKernelGGL(") == 1 and "op == OP_PHYS_TRANSITION ? fd_lds_bytes<C>() : sizeof(Smem<C>)" in lp
    assert lp.rstrip().endswith("default: return -1;\n  }\n}\n\n}  // namespace rsr")      # nothing follows the switch
    phys = open(os.path.join(CSRC, "physics", "rsr_physics.hpp")).read()
    assert re.search(r"\bint K;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    # the protocol that carried this launch and the inverse's on other ops is gone from every source
    for top in (CSRC, os.path.join(ROOT, "include")):
        for d, _, files in os.walk(top):
            for f in files:
                if f.endswith((".hip", ".hpp", ".h")):
                    text = open(os.path.join(d, f)).read()
                    for gone in ("INVERSE_TAG", "SAMPLE_TAG", "inverse_launch_args", "inverse_args", "sample_launch_args", "sample_args"):
                        assert gone not in text, (f, gone)
    import bench
    import parity_envelopes as PE
    assert PE.ENV["_provenance"]["csrc_sha16"] == bench.csrc_sha16()


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.sample_rollouts)
    assert list(sig.parameters) == ["self", "ctrl", "nsteps", "fields", "env_ids", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "ctrl")}
    assert d == dict(nsteps=None, fields=("qpos", "qvel", "time"), env_ids=None, out=None)
    assert sig.parameters["ctrl"].default is inspect.Parameter.empty
    assert "Physics.sample_rollouts(ctrl [M, K, T, nu])" in physics.__doc__ and "vmap(lax.scan(mjx.step))" in physics.__doc__
    assert "4 * M * K * T * w bytes" in Physics.sample_rollouts.__doc__
    # every bad input is refused before the C call: the recording library sees none
    p = standin(nq=5, nv=4)
    good = torch.zeros((4, 2, 3, 3), dtype=torch.float32)
    cases = [(dict(ctrl=torch.zeros((4, 3, 3))), "expects ctrl"),                         # 3-D
             (dict(ctrl=torch.zeros((4, 2, 3, 2))), "expects ctrl"),                      # wrong nu
             (dict(ctrl=good.double()), "expects ctrl"),                                  # float64
             (dict(ctrl=torch.zeros((4, 2, 3, 3), device="meta")), "expects ctrl"),       # wrong device
             (dict(ctrl=good.numpy()), "expects ctrl"),
             (dict(ctrl=good, env_ids=[0, 2]), "expects ctrl"),                           # M != len(env_ids)
             (dict(ctrl=good[:3]), "expects ctrl"),                                       # M != num_envs
             (dict(ctrl=good[:2], env_ids=[0, 4]), "env_ids must lie in"),
             (dict(ctrl=good, fields=("qpos", "qacc")), "unknown"),
             (dict(ctrl=good, fields=("sensordata",)), "no sensors are set"),
             (dict(ctrl=good, nsteps=0), "nsteps must be >= 1"),
             (dict(ctrl=good, out={"qpos": torch.zeros((4, 2, 3, 4))}), "out\\['qpos'\\]"),
             (dict(ctrl=good, out={"qpos": torch.zeros((4, 2, 3, 5)).numpy()}), "out\\['qpos'\\]")]      # (once an AttributeError)
    refused(monkeypatch, p.sample_rollouts, cases)
    # a good call goes through the env-list convention, ctrl after the count, and its inputs stay in its own slot, not copied
    rec = record(monkeypatch)
    part = good[:2]
    p.sample_rollouts(part, env_ids=[3, 1])
    (sym, (h, ids, k, ctrl, K, T, nsteps, out, stream)), = rec.calls
    assert (sym, h, k, ctrl, K, T, nsteps, stream) == ("rsr_physics_sample_rollouts", HANDLE, 2, part.data_ptr(), 2, 3, p.n_substeps, STREAM)
    assert ints(ids, 2) == [3, 1] and p._held["sample_rollouts"][0] is part and p._held["sample_rollouts"][1].data_ptr() == ids
    p.dynamics([0])                                                                    # another entry point's launch drops neither
    assert p._held["sample_rollouts"][0] is part and p._held["sample_rollouts"][1].data_ptr() == ids
