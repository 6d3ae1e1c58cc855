"""The Go2 joystick step kernel outside the physics, by branch, against the float64 reference of tests/go2_epilogue_ref.py -- both
terrain instantiations (Go2FlatDims, Go2Dims), every config variant of tests/go2_epilogue_cases.py, one teacher-forced step of the
392 fixture states each.  The reference is fed what the device itself publishes after the step (privileged_obs[48:123], site_xpos,
qpos, qvel, the new LAST_CONTACT word) and the record from before it, so the physics is not re-tested and its fp32 noise does not
enter: what is PRNG, integer-valued or a copy must be equal, every other quantity within 4 x the recorded ref32-ref64 distance + 2
ulp32 (+ the share of the two gravity identities, cases.ROW_DEFECT), and equal to the float32 reference bit for bit where no libm
call and neither identity is involved (cases.NOT_BITWISE lists the rest).  Envs that AutoReset restored no longer publish the step's
physics results: they are compared in what does not need them, and in full by the variants without AutoReset."""
import json
import os

import numpy as np
import pytest

import go2_epilogue_cases as CS
import go2_epilogue_ref as R
from conftest import ROOT
from rsr_mjx_amd import prng

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_EXCLUDED = 0.02          # of the states, by the up[2] band and the contact-pinning band together
_VIEW = {"priv_obs": "privileged_obs", "first_priv_obs": "first_privileged_obs"}
_READ = ("qpos", "qvel", "ctrl", "qacc_warmstart", "time", "xpos", "site_xpos", "obs", "priv_obs", "metrics", "reward", "done", "info_go2",
         "info_steps", "info_truncation", "info_episode_done", "info_episode_metrics")
_FIRST = {"qpos": "first_qpos", "qvel": "first_qvel", "ctrl": "first_ctrl", "qacc_warmstart": "first_warmstart", "time": "first_time",
          "xpos": "first_xpos", "site_xpos": "first_site_xpos", "obs": "first_obs", "priv_obs": "first_priv_obs"}


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "go2_epilogue_states.npz")))


@pytest.fixture(scope="module")
def tol():
    return json.load(open(os.path.join(GOLDEN, "go2_epilogue_tolerances.json")))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CS.VARIANTS))
@pytest.mark.parametrize("task", ["Flat", "Rough"])
def test_go2_step_epilogue_by_branch(fx, tol, task, name):
    import torch
    from rsr_mjx_amd.envs import go2
    over, length, auto = CS.VARIANTS[name]
    n = len(fx["cls"])
    jenv = go2.load(f"Go2Joystick{task}Terrain", config_overrides=over)
    env = jenv.batched(n, episode_length=length, auto_reset=auto)
    K = CS.variant_constants(jenv.sys, name)
    ids = CS.variant_fields(jenv.sys, name)[1]["env_ids"]
    state = env.reset(fx["keys"])
    for k in CS.RECORD:                                               # teacher forcing: the fixture's record over the reset's
        env.view(k).copy_(torch.from_numpy(fx[k].reshape(n, -1)))
    torch.cuda.synchronize()
    get = lambda k: env.view(_VIEW.get(k, k)).cpu().numpy().copy()
    before = {k: get(k) for k in CS.RECORD}
    state = env.step(state, fx["action"])
    torch.cuda.synchronize()
    after = {k: get(k) for k in _READ + tuple(_FIRST.values())}
    restored = (after["done"][:, 0] != 0) & auto
    live = ~restored
    # ---- the device's own verdict on termination where the reference has no say ----
    dev_term = (after["metrics"][:, R.RW_TERM] != 0).astype(np.float64)
    in_band = live & (np.abs(after["priv_obs"][:, 56]) < CS.UP2_BAND)
    phys = CS.phys_of(after, ids[1:5])
    phys["done_env"] = np.where(restored | in_band, dev_term, np.nan)
    # ---- the contact flags, pinned on flat terrain: a foot sphere touches the plane z = 0 iff its centre is below its radius ----
    excluded = in_band.copy()
    if task == "Flat":
        A = jenv.sys.arrays
        for f in range(4):
            g, s = ids[6 + f], ids[1 + f]
            assert A["geom_bodyid"][g] == A["site_bodyid"][s] and (A["geom_pos"][g] == A["site_pos"][s]).all()
            gap = phys["feet_z"][:, f].astype(np.float64) - float(A["geom_size"][g][0])
            clear = live & (np.abs(gap) >= CS.CONTACT_BAND)
            np.testing.assert_array_equal(phys["contact"][clear, f] != 0, gap[clear] < 0, err_msg=f"contact flag of foot {f}")
            excluded |= live & ~clear
    print(f"{task} {name}: {int(excluded.sum())} of {n} states excluded ({int(in_band.sum())} by the up[2] band), {int(restored.sum())} restored")
    assert excluded.sum() <= MAX_EXCLUDED * n, int(excluded.sum())
    # ---- the reference on the device's own record ----
    pre = CS.before_of(before, fx["action"])
    with np.errstate(invalid="ignore"):
        got = R.from_record(after)
    r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
    np.testing.assert_array_equal(r64["restored"], restored)
    fails, report = CS.compare(K, tol[name], phys, r64, got, live)
    g32, gq = R.float_quantities(r32, K), R.float_quantities(got, K)
    for nm, (dist, ratio) in report.items():
        sel = live if R.needs_phys(nm) else slice(None)
        same = bool((np.asarray(g32[nm], np.float32)[sel] == np.asarray(gq[nm], np.float32)[sel]).all())
        print(f"  {nm:36s} max |device - ref64| {dist:9.3e}  = {ratio:5.2f} x bound  ref32 bit-identical: {same}")
        if nm not in CS.NOT_BITWISE and not same:
            fails.append(f"{nm}: not bit-identical to the float32 reference")
    # reward and the Episode sums from the device's own metrics: sums of published float32 values, so bit for bit
    if not (after["reward"][:, 0] == R.reward_from_metrics(K, after["metrics"])).all():
        fails.append("reward: not the clamped float32 sum, in the kernel's order, of the metrics the step published")
    if K["episode"] and not (after["info_episode_metrics"] == R.episode_sums_from_outputs(K, pre, after["reward"], after["metrics"])).all():
        fails.append("episode sums: not the old sums plus the reward and metrics the step published")
    assert not fails, (task, name, fails)
    # ---- AutoReset: the restored blocks are the first state's, the kick force is zero again; info is never restored ----
    if auto:
        assert restored.sum() >= 3 * CS.MIN_PER_CLASS
        for k, fk in _FIRST.items():
            np.testing.assert_array_equal(after[k][restored], after[fk][restored], err_msg=k)
        assert not after["info_go2"][restored, R.G["XFRC"]:R.G["XFRC"] + 3].any()
    else:
        assert not restored.any()
    # ---- census on the device's own record ----
    c = CS.census(K, pre, CS.after_of(after, restored))
    short = {k: v for k, v in c.items() if v < CS.MIN_PER_CLASS}
    print(f"  census: {c}")
    assert not short, (task, name, short)
