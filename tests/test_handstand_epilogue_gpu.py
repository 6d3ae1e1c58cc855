"""The Go2 Handstand / Footstand step kernel (hs_step_kernel<HandDims>, hs_obs) and reset kernel outside the physics, by branch, against
the float64 reference of tests/handstand_epilogue_ref.py -- both tasks, every config variant of tests/handstand_epilogue_cases.py, one
teacher-forced step of the fixture states each, plus the same step with noise level 0 (the quiet twin, whose obs[6:9] is the clean
gravity triple).  The reference is fed what the device itself publishes after the step (privileged_obs[45:94], site_xpos, qpos,
qvel, qacc_warmstart) and the record from before it, so the physics is not re-tested and its fp32 noise does not enter: what is PRNG,
integer-valued or a copy must be equal, every other quantity within 4 x the recorded ref32-ref64 distance + 2 ulp32 (+ the recorded
share of reconstructing R[0], R[3] where the forward vector has x and y), and equal to the float32 reference bit for bit where no
libm call and no reconstruction is involved (cases.NOT_BITWISE lists the rest).

The contact flags.  Where n_frames = 1 the last forward pass runs at the fixture's own pose, and the reference forms `unwanted` /
`feet` from the float64 oracle's distance of all 30 pairs (cap off) stored with the fixture; no state is excluded, the generator kept
every pair out of the contact band.  The contact-cap classes hold the states on which a kernel that reads the flags off its capped
list of 12 contacts fails.  Where n_frames > 1 the flags are the device's own (tests/test_handstand.py checks those against the
oracle).  Envs that AutoReset restored take their physics results from the same step of a twin without AutoReset, whose metrics,
reward and info must be the same words."""
import json
import os

import numpy as np
import pytest

import handstand_epilogue_cases as CS
import handstand_epilogue_ref as R
from conftest import ROOT
from test_handstand_epilogue import check_reset

GOLDEN = os.path.join(ROOT, "tests", "golden")
_VIEW = {"priv_obs": "privileged_obs", "first_priv_obs": "first_privileged_obs"}


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "handstand_epilogue_states.npz")))


@pytest.fixture(scope="module")
def tol():
    return json.load(open(os.path.join(GOLDEN, "handstand_epilogue_tolerances.json")))


def _forced_step(task, name, fx, auto=None, quiet=False):
    """reset, the fixture's record over the reset's, one step: (env definition, before, after) as numpy"""
    import torch
    n = len(fx["cls"])
    jenv, env = CS.device_env(task, name, n, auto_reset=auto, quiet=quiet)
    assert env.dims.ncon_max == CS.NCON_CAP
    state = env.reset(fx["keys"])
    for k in CS.RECORD:                                               # teacher forcing
        env.view(k).copy_(torch.from_numpy(fx[k].reshape(n, -1)))
    torch.cuda.synchronize()
    get = lambda k: env.view(_VIEW.get(k, k)).cpu().numpy().copy()
    before = {k: get(k) for k in CS.RECORD}
    env.step(state, fx["action"])
    torch.cuda.synchronize()
    after = {k: get(k) for k in CS.READ + tuple(CS.FIRST.values()) + ("stats",)}
    return jenv, before, after


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CS.VARIANTS))
@pytest.mark.parametrize("task", list(CS.TASKS))
def test_handstand_step_epilogue_by_branch(fx, tol, task, name):
    n = len(fx["cls"])
    jenv, before, after = _forced_step(task, name, fx)
    _, _, quiet = _forced_step(task, name, fx, quiet=True)
    K = CS.variant_constants(jenv.sys, task, name)
    assert (K["n_frames"], K["episode"], K["autoreset"]) == (jenv.n_substeps, CS.VARIANTS[name]["length"] > 0, CS.VARIANTS[name]["auto"])
    # ---- the physics does not read the noise ----
    for k in after:
        if k not in CS.NOISY_WORDS:
            np.testing.assert_array_equal(after[k].view(np.int32), quiet[k].view(np.int32), err_msg=f"{k}: differs at noise level 0")
    restored = (after["done"][:, 0] != 0) & K["autoreset"]
    live = ~restored
    src, qsrc = after, quiet
    if K["autoreset"]:
        _, _, src = _forced_step(task, name, fx, auto=False)
        _, _, qsrc = _forced_step(task, name, fx, auto=False, quiet=True)
        for k in ("qpos", "qvel", "qacc_warmstart", "site_xpos", "obs", "priv_obs", "ctrl"):     # same kernel, same inputs: the same physics
            np.testing.assert_array_equal(after[k][live], src[k][live], err_msg=k)
        for k in ("metrics", "reward", "info_go2"):                   # never restored
            np.testing.assert_array_equal(after[k].view(np.int32), src[k].view(np.int32), err_msg=k)
    phys = CS.phys_of(K, jenv.sys, src, qsrc, fx, flags_from=after["metrics"])
    excluded = 0                                                      # nothing is: no band is needed (see the module docstring)
    print(f"{task} {name}: {excluded} of {n} states excluded, {int(restored.sum())} restored, "
          f"{int((after['stats'][:, 3] > 0).sum())} with contacts beyond the cap of {CS.NCON_CAP}")
    assert excluded <= CS.MAX_EXCLUDED * n
    # ---- the reference on the device's own record ----
    pre = CS.before_of(before, fx["action"])
    got = R.from_record(after)
    r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
    fails = []
    if not (r64["restored"] == restored).all():
        fails.append(f"done: {int((r64['restored'] != restored).sum())} envs restored that the reference does not end, or the reverse")
    f2, report = CS.compare(K, tol[task][name], tol["orientation_share"][task], r64, got, live)
    fails += f2
    same = CS.bitwise(K, r32, got, live)
    for nm, (dist, ratio) in report.items():
        print(f"  {nm:24s} max |device - ref64| {dist:9.3e}  = {ratio:5.2f} x bound  ref32 bit-identical: {same[nm]}")
        if nm not in CS.not_bitwise(K) and not same[nm]:
            fails.append(f"{nm}: not bit-identical to the float32 reference")
    # reward and the Episode sums from the device's own metrics: sums of published float32 values, so bit for bit
    if not (after["reward"][:, 0] == R.reward_from_metrics(K, after["metrics"])).all():
        fails.append("reward: not the clamped float32 sum, in the kernel's order, of the metrics the step published")
    if K["episode"] and not (after["info_episode_metrics"] == R.episode_sums_from_outputs(K, pre, after["reward"], after["metrics"])).all():
        fails.append("episode sums: not the old sums plus the reward and metrics the step published")
    # ---- by class: which states carry the failures of the flags ----
    names, wrong = [str(s) for s in fx["class_names"]], (got["metrics"][:, R.HM_TERM] != r64["metrics"][:, R.HM_TERM]) | (got["metrics"][:, R.HM_CONTACT] != r64["metrics"][:, R.HM_CONTACT])
    if wrong.any():
        by = {names[c]: int((wrong & (fx["cls"] == c)).sum()) for c in np.unique(fx["cls"][wrong])}
        fails.append(f"termination / contact metric wrong in {int(wrong.sum())} states, by the class they were built for: {by}")
    for f in fails:
        print("  FAIL:", f)
    assert not fails, (task, name, fails)
    # ---- AutoReset: the restored blocks are the first state's; info is never restored ----
    if K["autoreset"]:
        assert restored.sum() >= 3 * CS.MIN_PER_CLASS and live.sum() >= 3 * CS.MIN_PER_CLASS
        for k, fk in CS.FIRST.items():
            np.testing.assert_array_equal(after[k][restored], after[fk][restored], err_msg=k)
    else:
        assert not restored.any()
    # ---- census on the device's own record ----
    c = CS.census(K, pre, r32, phys, fx)
    short = {k: v for k, v in c.items() if v < CS.MIN_PER_CLASS}
    print(f"  census: {c}")
    assert not short, (task, name, short)


@pytest.mark.gpu
@pytest.mark.parametrize("task", list(CS.TASKS))
def test_handstand_reset_pose_on_device(task):
    """hs_reset_kernel against reset_pose for init_from_crouch in {0, 0.5, 1}: crouch choice, qvel, ctrl and key bit for bit; qpos bit
    for bit except the yaw quaternion (sinf / cosf), which gets the 2-ulp rule."""
    import torch
    from rsr_mjx_amd.envs import go2
    n = 256
    keys = CS.reset_keys(n)
    for p in (0.0, 0.5, 1.0):
        jenv = go2.load(task, config_overrides={"init_from_crouch": p})
        env = jenv.batched(n)
        env.reset(keys)
        torch.cuda.synchronize()
        st = {k: env.view(k).cpu().numpy().copy() for k in ("qpos", "qvel", "ctrl", "info_go2")}
        K = R.constants(jenv._fields_fn(jenv.sys), jenv.sys)
        assert K["F"][R.F_CROUCH] == np.float32(p)
        check_reset(K, st, R.reset_pose(K, keys, np.float32), R.reset_pose(K, keys, np.float64), p)
