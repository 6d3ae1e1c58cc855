"""The Airbot step kernel outside the physics (step_kernel<C, ENV> for cube, sf and T-shape), by branch, against the float64 reference
of tests/airbot_epilogue_ref.py -- every config variant of tests/airbot_epilogue_cases.py, one teacher-forced step of the fixture's
states each.  The reference is fed what the device itself publishes after the step (qpos, xpos, site_xpos; T-shape: obs[7:13] and
xita) and the record from before it, so the physics is not re-tested and its fp32 noise does not enter: what is integer-valued, a
copy or a pass-through word must be equal, every other quantity within 4 x the recorded ref32-ref64 distance of the state's class
+ 2 ulp32, and equal to the float32 reference bit for bit where no libm call is involved (cases.NOT_BITWISE lists the rest).
An AutoReset variant is stepped next to its twin without AutoReset: the twin publishes the physics results of the envs AutoReset
restored, so those are compared in everything but the restored blocks, which must equal the first state's."""
import importlib.util
import json
import os

import numpy as np
import pytest

import airbot_epilogue_cases as CS
import airbot_epilogue_ref as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [(k, v) for k in CS.KINDS for v in CS.VARIANTS]


@pytest.fixture(scope="module")
def MK():
    spec = importlib.util.spec_from_file_location("make_airbot_epilogue_states", os.path.join(GOLDEN, "make_airbot_epilogue_states.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "airbot_epilogue_states.npz")))


@pytest.fixture(scope="module")
def tol():
    return json.load(open(os.path.join(GOLDEN, "airbot_epilogue_tolerances.json")))


def _envdef(kind, kw):
    from rsr_mjx_amd.envs.airbot import AirbotPlayBase, AirbotPlaySF, AirbotTShape
    return {"cube": AirbotPlayBase, "sf": AirbotPlaySF, "tshape": AirbotTShape}[kind](device="cuda:0", **kw)


def _forced_step(kind, name, f, auto=None, schedule=None):
    """reset, the fixture's record over the reset's, one step: (env, before, after) as numpy"""
    import torch
    kw, length, auto_v = CS.VARIANTS[name]
    n = len(f["cls"])
    env = _envdef(kind, kw).batched(n, episode_length=length, auto_reset=auto_v if auto is None else auto)
    assert env.dims.ncon_max == CS.NCON_CAP[kind]
    if schedule is not None:
        env.set_schedule(schedule[0]); env.set_whole_envs(schedule[1])
    env.reset(f["keys"])
    for k in CS.RECORD[kind]:                                          # teacher forcing
        env.view(k).copy_(torch.from_numpy(f[k].reshape(n, -1)))
    torch.cuda.synchronize()
    get = lambda k: env.view(k).cpu().numpy().copy()
    before = {k: get(k) for k in CS.READ[kind]}
    env.step(None, f["action"])
    torch.cuda.synchronize()
    after = {k: get(k) for k in CS.READ[kind] + tuple(CS.FIRST.values())}
    return env, before, after


@pytest.mark.gpu
@pytest.mark.parametrize("kind,name", CASES)
def test_airbot_step_epilogue_by_branch(MK, fx, tol, kind, name):
    f = MK.of_kind(fx, kind)
    names, cls, n = [str(s) for s in f["class_names"]], f["cls"], len(f["cls"])
    env, before, after = _forced_step(kind, name, f)
    K = CS.variant_constants(env.sys, kind, name)
    assert env.handoff_timeouts() == 0 and int(env.view("stats")[:, 3].min()) >= 0
    restored = (after["done"][:, 0] != 0) & K["autoreset"]
    live = ~restored
    phys = CS.phys_of(kind, after)
    if K["autoreset"]:
        _, _, twin = _forced_step(kind, name, f, auto=False)
        for k in ("qpos", "xpos", "site_xpos", "obs", "ctrl"):         # same kernel, same inputs: the same physics, bit for bit
            np.testing.assert_array_equal(after[k][live], twin[k][live], err_msg=k)
        for k in ("metrics", "reward", "info_site_pos", R.BODY_POS[kind], R.NEW_POS[kind]):
            np.testing.assert_array_equal(after[k], twin[k], err_msg=k)
        tp = CS.phys_of(kind, twin)
        phys = {k: np.where(restored.reshape((-1,) + (1,) * (v.ndim - 1)), tp[k], v) for k, v in phys.items()}
    # ---- the reference on the device's own record ----
    pre = CS.before_of(before, f["action"])
    got = R.from_record(K, after)
    r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
    np.testing.assert_array_equal(r32["restored"], restored)
    excluded = CS.excluded_states(K, r32)
    print(f"{kind} {name}: {int(excluded.sum())} of {n} states excluded (within {R.BAND_ULPS} ulp32 of a threshold), {int(restored.sum())} restored")
    assert excluded.sum() <= CS.MAX_EXCLUDED * n, int(excluded.sum())
    fails, report = CS.compare(K, tol[kind][name], names, cls, r64, got, live, excluded)
    same = CS.bitwise(K, r32, got, live, excluded)
    for nm, (dist, ratio) in report.items():
        print(f"  {nm:30s} max |device - ref64| {dist:9.3e}  = {ratio:5.2f} x bound  ref32 bit-identical: {same[nm]}")
        if nm not in CS.NOT_BITWISE and not same[nm]:
            fails.append(f"{nm}: not bit-identical to the float32 reference")
    keep = ~excluded
    # reward and the Episode sums from the device's own metrics: sums of published float32 values, so bit for bit
    if not (after["reward"][:, 0] == R.reward_from_metrics(K, after["metrics"], r32.get("unpublished_terms", ())))[keep].all():
        fails.append("reward: not the clamped float32 sum, in the kernel's order, of the metrics the step published")
    if K["episode"]:
        want = R.episode_sums_from_outputs(K, pre, after["reward"], after["metrics"])
        if not ((after["info_episode_metrics"] == want) | (np.isnan(want) & np.isnan(after["info_episode_metrics"]))).all():
            fails.append("episode sums: not the old sums plus the reward and metrics the step published")
    for k in CS.UNTOUCHED[kind]:
        if not (after[k] == before[k]).all():
            fails.append(f"{k}: a word no step writes has changed")
    if kind == "sf":
        held = r32["verdicts"]["hold"] & keep
        if not (after["info_last_action"][held] == before["info_last_action"][held]).all():
            fails.append("info_last_action: not kept where the wrist is held")
    assert not fails, (kind, name, fails)
    # ---- AutoReset: the restored blocks are the first state's; info and metrics are never restored ----
    if K["autoreset"]:
        assert restored.sum() >= 3 * CS.MIN_PER_CLASS and live.sum() >= 3 * CS.MIN_PER_CLASS
        for k, fk in CS.FIRST.items():
            np.testing.assert_array_equal(after[k][restored], after[fk][restored], err_msg=k)
    else:
        assert not restored.any()
    # ---- census on the device's own record ----
    c = CS.census(K, pre, after, r32)
    print(f"  census: {c}")
    short = {k: v for k, v in c.items() if v < CS.MIN_PER_CLASS}
    assert not short, (kind, name, short)
    # ---- one substep: derived data are from the forward pass at the pre-step pose, not from the integrated one ----
    if K["n_frames"] == 1:
        kt = tol[kind]["kinematics"]
        xpos, sites, geoms = MK.kinematics_batch(env.sys, before["qpos"], np.float64)
        ulp = float(np.spacing(np.float32(max(np.abs(xpos).max(), np.abs(sites).max(), np.abs(geoms).max()))))
        ids = K["ids"]
        checks = [("xpos", after["xpos"].reshape(xpos.shape), xpos, kt["xpos"]), ("site_xpos", after["site_xpos"].reshape(sites.shape), sites, kt["site_xpos"])]
        if kind == "tshape":
            tb, tv = before["info_target_base_pos"].astype(np.float64), before["info_target_vertical_pos"].astype(np.float64)
            checks += [("base_block", tb - after["obs"][:, 7:10], geoms[:, ids[R.TID_GBASE]], kt["geom_xpos"] + ulp),
                       ("vertical_block", tv - after["obs"][:, 10:13], geoms[:, ids[R.TID_GVERT]], kt["geom_xpos"] + ulp)]
        for nm, dev, ref, t in checks:
            d = float(np.abs(dev - ref).max())
            print(f"  forward pass at the pre-step pose, {nm}: max |device - fp64 kinematics| {d:.3e}, bound {CS.FACTOR * t + CS.ULPS * ulp:.3e}")
            assert d <= CS.FACTOR * t + CS.ULPS * ulp, (kind, nm, d)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CS.KINDS)
def test_prologue_and_epilogue_in_different_waves(MK, fx, kind):
    """set_schedule(4), set_whole_envs(0): every env is cut into four work units, so the prologue and the epilogue run in different
    waves and ctrl crosses through the record.  The record after the step is the one-unit record, bit for bit."""
    f = MK.of_kind(fx, kind)
    one, _, _ = _forced_step(kind, "autoreset", f, schedule=(1, -1))
    four, _, _ = _forced_step(kind, "autoreset", f, schedule=(4, 0))
    a, b = one.record.cpu().numpy().view(np.int32), four.record.cpu().numpy().view(np.int32)
    np.testing.assert_array_equal(a, b)
    assert one.handoff_timeouts() == 0 and four.handoff_timeouts() == 0
