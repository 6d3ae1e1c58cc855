"""Parameter rollouts of the physics layer (rsr_physics_param_rollouts, Physics.param_rollouts, tuning.RolloutLoss), host side
only: the ABI, the launch as an op of the physics layer, the Python surface and the tuning helper's reduction.
The kernel's text is covered by tests/test_sampled_kernel_api.py, the kernel by tests/test_param_rollouts_gpu.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_support import CSRC, ROOT, body as _body, header, read as _read, record, refused, standin

SIG = ("int rsr_physics_param_rollouts(rsr_physics* p, const int32_t* env_ids, int count, const float* ctrl, "
       "const rsr_param_samples* params, int K, int T, int nsteps, int flags, const rsr_rollout_out* out, void* hip_stream);")


def test_header_declares_the_call_and_the_struct():
    h = header()
    flat = re.sub(r"\s+", " ", h)
    assert SIG in flat                                             # (the declaration may break its lines)
    assert "typedef struct rsr_param_samples { const float* leaf[RSR_DR_COUNT]; } rsr_param_samples;" in flat
    assert re.search(r"#define RSR_PR_CTRL_PER_SAMPLE 1\b", h)
    doc = h[h.index("/* Parameter rollouts"):h.index("typedef struct rsr_param_samples")]
    for word in ("[M, K, width]", "[M, T, nu]", "[M, K, T, nu]", "[M, K, T, width]", "bit for bit", "qacc_warmstart",
                 "position in env_ids", "untouched", "own leaf tensors", "no PRNG key advances", "left alone", "before any device work",
                 "2^31", "RSR_ERR_UNSUPPORTED", "unknown flag bits", "rsr_physics_sample_rollouts", "owns no buffer"):
        assert word in doc, word
    assert h.count("typedef struct rsr_rollout_out") == 1          # the existing struct, not a second one
    assert "rsr_param" not in open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()


def test_library_exports_and_null_handle():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    assert "rsr_physics_param_rollouts" in _lib.PHYS_SYMBOLS
    fn = L.rsr_physics_param_rollouts
    assert fn.argtypes is not None and len(fn.argtypes) == 11
    assert _lib.PR_CTRL_PER_SAMPLE == 1
    ps = _lib.ParamSamples()
    assert C.sizeof(ps) == len(_lib.DR_FIELDS) * C.sizeof(C.c_void_p) and len(ps.leaf) == 9 and not any(ps.leaf)
    ids = (C.c_int32 * 2)(0, 1)
    ctrl = (C.c_float * 8)()
    o = _lib.RolloutOut()
    for table, k in ((None, 0), (ids, 2), (ids, 0)):
        for params in (None, C.byref(ps)):
            assert fn(None, table, k, ctrl, params, 1, 1, 1, 0, C.byref(o), None) == -1
            assert b"null handle" in L.rsr_last_error()


def test_refusals_come_before_device_work():
    """Every refusal comes ahead of every device call (by source order, as a handle needs a device), and the call allocates
    nothing: the handle owns no buffer for it.  The entry's own checks, then the tail the two sweep entries share, which opens
    with the refusals of all three (slot, sample) rollouts (sample_grid)."""
    src = _read("physics", "rsr_physics.hip")
    entry, tail = _body(src, "int rsr_physics_param_rollouts"), _body(src, "static int sweep_rollouts")
    first = "if (const int rc = sample_grid(p, env_ids, count, sw.K, T, nsteps, out, who, &grid)) return rc;"
    assert re.findall(r"^  (?:if|for|return)\b.*", tail, re.M)[0].strip() == first          # the tail's first statement
    tail = tail.replace(first, _body(src, "static int sample_grid"))                       # ... read in its place
    assert entry.rstrip().endswith('return sweep_rollouts(p, env_ids, count, ctrl, params, sw, T, nsteps, out, hip_stream, "rsr_physics_param_rollouts");')
    assert entry.count("sweep_rollouts(") == 1 and "OP_PHYS_" not in entry
    call = entry + tail
    dev = ("hipSetDevice", "hipMalloc", "hipMemset", "hipMemcpy", "zeroed_once", "launch(")
    first_dev = min(call.index(k) for k in dev if k in call)
    assert first_dev == call.index("physics_launch(") + len("physics_")
    checks = ("!p)", "!ctrl)", "!out ||", "out->qpos || out->qvel || out->time || out->actuator_force || out->ncon || out->sensordata)",
              "K < 1", "T < 1", "nsteps < 1", "flags & ~RSR_PR_CTRL_PER_SAMPLE", "env_count(", "out->sensordata && p->nsd == 0",
              "grid > INT32_MAX", "(int64_t)T * nsteps > INT32_MAX", "RSR_ERR_UNSUPPORTED", "f >= RSR_DR_BODY_IPOS")
    at = [call.index(c) for c in checks]
    assert at[:-1] == sorted(at[:-1]) and all(i < first_dev for i in at), [c for c, i in zip(checks, at) if i >= first_dev]      # (today's order)
    assert "(int64_t)n * K" in call and call.count("RSR_ERR_ARG") == 7 and call.count("RSR_ERR_UNSUPPORTED") == 1
    for k in ("hipMalloc", "hipMemset", "hipMemcpy", "hipFree", "zeroed_once", "_buffer", "new ", "std::vector"):
        assert k not in call, k
    assert "_alloc" not in src and src.count("static int zeroed_once(") == 1
    # the tail names the one op, and every message is the entry's: built from `who`
    assert re.findall(r"\bOP_PHYS_\w+", tail) == ["OP_PHYS_SWEEP"] and "rsr_physics_" not in tail
    assert tail.count("std::string(who) + ") == 3 and tail.count("fail(") == 3
    assert tail.index("physics_args(") < tail.index("x.ph.r = rsr::RollArgs{ctrl, T, ") < tail.index("x.ph.sw = sw;") < tail.index("physics_launch(")
    assert "counted(p, physics_launch(p, rsr::OP_PHYS_SWEEP, x, who))" in tail


def test_the_launch_is_an_ordinary_op():
    from rsr_mjx_amd import build
    assert len(build.UNITS) == 5 and len(dict(build.UNITS)) == 5
    physics = os.listdir(os.path.join(CSRC, "physics"))
    assert not [f for f in physics if f.startswith("rsr_sweep_")] and "rsr_sweep.hpp" in physics
    # the host sends the op like every other: no entry of its own per family, no second family switch
    host = _read("physics", "rsr_physics.hip")
    assert set(re.findall(r"\b(\w*launch\w*)\(", host)) == {"launch", "launch_args", "physics_launch"}
    assert "spec->family" not in host.replace("spec->family != rsr::FAMILY_GO2", "")
    assert "switch (ph->b->model" not in host and "FAMILY_CUBE" not in host and "FAMILY_TSHAPE" not in host
    # the arguments beside the other ops'
    phys = _read("physics", "rsr_physics.hpp")
    assert "struct SweepArgs" in phys and "const float* leaf[RSR_DR_COUNT];" in phys
    assert re.search(r"\bSweepArgs sw;", re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1))
    # the op's own case, up to the next label: the one (slot, sample) kernel as this op's, plain and applied, with p, r and sw,
    # and no other kernel or op
    kernels = _read("physics", "rsr_physics_kernels.hpp")
    assert '#include "rsr_sweep.hpp"' in kernels
    lp = kernels[kernels.index("int launch_physics("):]
    case = re.search(r"case OP_PHYS_SWEEP:(.*?)\n\s*(?:case |default:)", lp, re.S).group(1)
    assert case.count("sampled_kernel<C, WAVES, SweepOp, Applied>, ph.p, ph.r, ph.sw, ph.ap)") == 1 and case.count("sampled_kernel<C, WAVES, SweepOp>, ph.p, ph.r, ph.sw)") == 1
    assert re.findall(r"\b\w+_kernel\b", case) == ["sampled_kernel"] * 2 and lp.count("SweepOp") == 2 and re.findall(r"\b\w+Op\b", case) == ["SweepOp"] * 2
    assert lp.count("sampled_kernel") == 6                              # three ops, plain and applied
    assert lp.index("case OP_PHYS_SAMPLE:") < lp.index("case OP_PHYS_SWEEP:") < lp.index("default:")
    assert lp.count("hipLaunchKernelGGL(") == 1 and "op == OP_PHYS_TRANSITION ? fd_lds_bytes<C>() : sizeof(Smem<C>)" in lp
    for hdr in ("rsr_sweep.hpp", "rsr_feedback.hpp"):
        assert '#include "../rsr_launch.hpp"' in _read("physics", hdr), hdr
    # nothing directly under csrc/ knows; the hashed sources are the parent's
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            assert "sampled_kernel" not in text and "SweepOp" not in text and "rsr_sweep" not in text and "SweepArgs" not in text, f
    import bench
    import parity_envelopes as PE
    assert PE.ENV["_provenance"]["csrc_sha16"] == bench.csrc_sha16()
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    assert len(re.findall(r"\bOP_PHYS_\w+", enum)) == 9 and "OP_PHYS_SWEEP" in enum
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4j."):design.index("### 4k.")]
    assert "**Dispatch: an ordinary op.**" in sec and "OP_PHYS_SWEEP" in sec and "PhysLaunch::sw" in sec


def test_physics_module_surface(monkeypatch):
    import torch
    from rsr_mjx_amd import physics
    from rsr_mjx_amd.physics import Physics
    sig = inspect.signature(Physics.param_rollouts)
    assert list(sig.parameters) == ["self", "ctrl", "params", "nsteps", "fields", "env_ids", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "ctrl", "params")}
    assert d == dict(nsteps=None, fields=("qpos", "qvel", "time"), env_ids=None, out=None)
    assert "Physics.param_rollouts(ctrl [M, T, nu], {leaf: [M, K, ...]})" in physics.__doc__
    assert "4 * M * K * T * w bytes" in Physics.param_rollouts.__doc__
    # sample_rollouts is as it was
    assert list(inspect.signature(Physics.sample_rollouts).parameters) == ["self", "ctrl", "nsteps", "fields", "env_ids", "out"]
    # every bad input is refused before the C call: the recording library sees none
    p = standin(nq=5, nv=4)                                 # (kind 0: an Airbot model; no sensors set)
    shared, each = torch.zeros((4, 3, 3)), torch.zeros((4, 2, 3, 3))
    mass, fric, damp = torch.zeros((4, 2, 3)), torch.zeros((4, 2, 6, 3)), torch.zeros((4, 2, 4))
    ok = dict(body_mass=mass)
    cases = [(dict(ctrl=torch.zeros((4, 3)), params=ok), "expects ctrl"),                               # 2-D
             (dict(ctrl=torch.zeros((4, 3, 2)), params=ok), "expects ctrl"),                            # wrong nu
             (dict(ctrl=shared.double(), params=ok), "expects ctrl"),                                   # float64
             (dict(ctrl=torch.zeros((4, 3, 3), device="meta"), params=ok), "expects ctrl"),             # wrong device
             (dict(ctrl=shared.numpy(), params=ok), "expects ctrl"),
             (dict(ctrl=shared, params=ok, env_ids=[0, 2]), "expects ctrl"),                            # M != len(env_ids)
             (dict(ctrl=shared[:3], params=ok), "expects ctrl"),                                        # M != num_envs
             (dict(ctrl=shared[:2], params=dict(body_mass=mass[:2]), env_ids=[0, 4]), "env_ids must lie in"),
             (dict(ctrl=shared, params={}), "K is not given"),                                          # nothing says K
             (dict(ctrl=shared, params=None), "K is not given"),
             (dict(ctrl=shared, params=dict(mass=mass)), "not a model leaf"),                           # name
             (dict(ctrl=shared, params=dict(body_mass=torch.zeros((4, 2, 4)))), r"params\['body_mass'\]"),      # shape
             (dict(ctrl=shared, params=dict(geom_friction=torch.zeros((4, 2, 18)))), r"params\['geom_friction'\]"),
             (dict(ctrl=shared, params=dict(body_mass=mass[:3])), r"params\['body_mass'\]"),            # M
             (dict(ctrl=shared, params=dict(body_mass=mass.double())), r"params\['body_mass'\]"),       # dtype
             (dict(ctrl=shared, params=dict(body_mass=torch.zeros((4, 2, 3), device="meta"))), r"params\['body_mass'\]"),
             (dict(ctrl=shared, params=dict(body_mass=mass.numpy())), r"params\['body_mass'\]"),
             (dict(ctrl=shared, params=dict(body_mass=torch.zeros((4, 3, 2)).transpose(1, 2))), r"params\['body_mass'\]"),    # contiguity
             (dict(ctrl=shared, params=dict(body_mass=mass, dof_damping=torch.zeros((4, 3, 4)))), "K = 3"),      # disagreeing K
             (dict(ctrl=torch.zeros((4, 5, 3, 3)), params=ok), "K = 2"),                                # ... with a 4-D ctrl
             (dict(ctrl=shared, params=dict(qpos0=torch.zeros((4, 2, 5)))), "Go2 models only"),
             (dict(ctrl=shared, params=ok, fields=("qpos", "qacc")), "unknown"),
             (dict(ctrl=shared, params=ok, fields=()), "no fields"),
             (dict(ctrl=shared, params=ok, fields=("sensordata",)), "no sensors are set"),
             (dict(ctrl=shared, params=ok, nsteps=0), "nsteps must be >= 1"),
             (dict(ctrl=shared, params=ok, out={"qpos": torch.zeros((4, 2, 3, 4))}), "out\\['qpos'\\]"),
             (dict(ctrl=each, params=dict(geom_friction=fric, dof_damping=damp), out={"qvel": torch.zeros((4, 3, 3, 4))}), "out\\['qvel'\\]")]
    cases.append((dict(ctrl=shared, params=ok, out={"qvel": np.zeros((4, 2, 3, 4), np.float32)}), "out\\['qvel'\\]"))     # (once an AttributeError)
    refused(monkeypatch, p.param_rollouts, cases)
    # a good call is the one library call, and its inputs stay in its own slot, not copied
    rec = record(monkeypatch)
    p.param_rollouts(each, dict(geom_friction=fric, dof_damping=damp), env_ids=[0, 1, 2, 3])
    (sym, args), = rec.calls
    assert sym == "rsr_physics_param_rollouts" and len(args) == 11 and args[3] == each.data_ptr()
    assert all(any(t is x for x in p._held["param_rollouts"]) for t in (each, fric, damp))


class _FakePhys:
    """param_rollouts as a known function of the leaves: qpos[e, v, t, c] = (e + 1) * (t + 1) * damping[e, v, c] + c * mass[e, v, 0]"""

    def __init__(self):
        self.calls = []

    def param_rollouts(self, ctrl, params, nsteps=None, fields=("qpos", "qvel", "time"), env_ids=None, out=None):
        import torch
        self.calls.append(dict(ctrl=ctrl, params=params, fields=fields, env_ids=env_ids))
        M, T = ctrl.shape[0], ctrl.shape[1]
        damp = params["dof_damping"]
        assert damp.shape[0] == M and damp.is_contiguous() and damp.dtype == torch.float32
        mass = params["body_mass"] if "body_mass" in params else torch.zeros((M, damp.shape[1], 1))
        e = torch.arange(1, M + 1, dtype=torch.float32)[:, None, None, None]
        t = torch.arange(1, T + 1, dtype=torch.float32)[None, None, :, None]
        c = torch.arange(damp.shape[2], dtype=torch.float32)[None, None, None, :]
        return {fields[0]: e * t * damp[:, :, None, :] + c * mass[:, :, None, :1]}


def test_rollout_loss_reduces_and_broadcasts():
    import torch
    from rsr_mjx_amd import tuning
    sig = inspect.signature(tuning.RolloutLoss.__init__)
    assert list(sig.parameters) == ["self", "phys", "ctrl", "target", "field", "make_leaves", "weights", "env_ids"]
    assert sig.parameters["weights"].default is None and sig.parameters["env_ids"].default is None
    assert "epilogue" in tuning.RolloutLoss.__doc__ and "observation" in tuning.RolloutLoss.__doc__
    M, T, w = 3, 4, 2
    fake = _FakePhys()
    ctrl = torch.zeros((M, T, 5))
    truth = np.array([0.7, -0.2])
    leaves = lambda P: {"dof_damping": np.asarray(P, np.float32), "body_mass": np.ones((len(P), 6), np.float32) * 2.0}
    e, t = np.arange(1, M + 1)[:, None, None], np.arange(1, T + 1)[None, :, None]
    at_truth = {f: torch.as_tensor(v)[None].expand((M,) + v.shape).contiguous() for f, v in leaves(truth[None]).items()}
    target = fake.param_rollouts(ctrl, at_truth, fields=("qpos",))["qpos"][:, 0].numpy()          # the fake's own arithmetic: exact at the truth
    assert np.allclose(target, e * t * truth[None, None, :] + np.arange(w)[None, None, :] * 2.0, rtol=1e-6)
    fake.calls.clear()
    weights = np.array([1.0, 10.0], np.float32)
    loss = tuning.RolloutLoss(fake, ctrl, target, "qpos", leaves, weights=weights, env_ids=[2, 0, 1])
    P = np.array([[0.7, -0.2], [0.5, -0.2], [0.7, 0.3], [0.0, 0.0]])
    got = loss(P)
    assert got.shape == (4,)
    # sum over envs, steps and columns of |w_c (traj - target)| = sum_e (e+1) sum_t (t+1) sum_c w_c |p_c - truth_c|
    want = np.array([e.sum() * t.sum() * float((weights * np.abs(np.float32(row) - np.float32(truth))).sum()) for row in P])
    assert got[0] == 0.0 and np.allclose(got, want, rtol=1e-5), (got, want)
    call = fake.calls[-1]
    assert call["ctrl"] is ctrl and call["fields"] == ("qpos",) and call["env_ids"] == [2, 0, 1]          # one call, shared ctrl
    for name, per in (("dof_damping", P.astype(np.float32)), ("body_mass", np.full((4, 6), 2.0, np.float32))):
        leaf = call["params"][name]
        assert tuple(leaf.shape) == (M,) + per.shape and leaf.is_contiguous()
        for env in range(M):
            assert np.array_equal(leaf[env].numpy(), per), name                                           # every env gets every variant
    assert len(fake.calls) == 1
    # default weights are ones; a bad target or weight shape is refused
    plain = tuning.RolloutLoss(fake, ctrl, target, "qpos", leaves)
    assert np.allclose(plain(P[1:2]), e.sum() * t.sum() * np.abs(np.float32(0.5) - np.float32(0.7)), rtol=1e-5)
    with pytest.raises(ValueError, match="target"):
        tuning.RolloutLoss(fake, ctrl, target[:, :3], "qpos", leaves)
    with pytest.raises(ValueError, match="weights"):
        tuning.RolloutLoss(fake, ctrl, target, "qpos", leaves, weights=np.ones(3))
    # it is what adam_fd_minimise takes: 2 k + 1 variants per step, and the parameters move toward the minimum
    fake.calls.clear()
    p0 = np.array([0.2, 0.2])
    p, hist = tuning.adam_fd_minimise(loss, p0, -1.0, 1.0, num_steps=40, lr=0.02)
    assert len(fake.calls) == 40 and fake.calls[0]["params"]["dof_damping"].shape == (M, 5, 2)
    assert np.abs(p - truth).sum() < 0.5 * np.abs(p0 - truth).sum() and hist["loss"][-1] < 0.5 * hist["loss"][0]
