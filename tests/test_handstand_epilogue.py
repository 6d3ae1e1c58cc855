"""The Go2 Handstand / Footstand step outside the physics, by branch, on the CPU: the numpy reference (tests/handstand_epilogue_ref.py)
against the oracle's own step and reset, the census of the fixture's branch classes, the generator's contact band, the recorded
tolerance table, and the contact flags of the capped oracle against the uncapped one.  tests/test_handstand_epilogue_gpu.py runs the
same reference against the HIP kernels.

On the oracle comparison.  oracle/rsr_oracle.c evaluates the env's algebra in `float` in BOTH of its builds (only the physics is
`real`), and the record it hands back is float32.  What is asserted:
  * everything that is PRNG, integer-valued or a copy is equal, in both builds and all variants;
  * the float32 reference -- the oracle's own precision and operation order -- is bit-identical to the oracle in every float
    quantity that does not go through libm's expf (the height term, and the reward and sums that add it up) or, with a general
    forward vector, through the reconstruction of R[0], R[3];
  * the float64 reference is within the bound the GPU module uses (4 x the recorded ref32-ref64 distance + 2 ulp32 + the
    reconstruction's share) in every float quantity, so the reference the device is judged by is itself pinned here."""
import importlib.util
import json
import os

import numpy as np
import pytest

import handstand_epilogue_cases as CS
import handstand_epilogue_ref as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [(t, v) for t in CS.TASKS for v in CS.VARIANTS]


@pytest.fixture(scope="module")
def MK():
    spec = importlib.util.spec_from_file_location("make_handstand_epilogue_states", os.path.join(GOLDEN, "make_handstand_epilogue_states.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "handstand_epilogue_states.npz")))


@pytest.fixture(scope="module")
def tol():
    return json.load(open(os.path.join(GOLDEN, "handstand_epilogue_tolerances.json")))


@pytest.fixture(scope="module")
def model(MK):
    return MK.go2_model()


_CACHE = {}


def _stepped(MK, model, fx, task, name, prec):
    """one oracle step of the fixture per task, variant and build (with its quiet and AutoReset-free twins), computed once"""
    if (task, name, prec) not in _CACHE:
        _CACHE[task, name, prec] = MK.stepped(model, task, name, prec, fx)
    return _CACHE[task, name, prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("task,name", CASES)
def test_reference_reproduces_the_oracle(MK, model, oracle_mod, fx, tol, task, name, prec):
    K, before, after, quiet, phys = _stepped(MK, model, fx, task, name, prec)
    pre = CS.before_of(before, fx["action"])
    got = R.from_record(after)
    r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
    live = ~r64["restored"]
    assert K["autoreset"] == bool(r64["restored"].any())
    # the physics does not read the noise: the quiet twin differs in the observation words only
    for k in after:
        if after[k] is not None and k not in CS.NOISY_WORDS:
            np.testing.assert_array_equal(after[k].view(np.int32), quiet[k].view(np.int32), err_msg=f"{k}: differs at noise level 0")
    share = tol["orientation_share"][task]
    fails, report = CS.compare(K, tol[task][name], share, r64, got, live)
    assert not fails, (task, name, prec, fails)
    same = CS.bitwise(K, r32, got, live)
    odd = [nm for nm in same if nm not in CS.not_bitwise(K) and not same[nm]]
    assert not odd, (task, name, prec, "not bit-identical to the float32 reference", odd)
    # reward and the Episode sums from the oracle's own metrics: sums of published float32 values, so bit for bit
    np.testing.assert_array_equal(after["reward"].reshape(-1), R.reward_from_metrics(K, after["metrics"]))
    if K["episode"]:
        np.testing.assert_array_equal(after["info_episode_metrics"], R.episode_sums_from_outputs(K, pre, after["reward"], after["metrics"]))
    # AutoReset: the restored blocks are the first state's; info is never restored
    if K["autoreset"]:
        w = r64["restored"]
        assert w.sum() >= 3 * CS.MIN_PER_CLASS and live.sum() >= 3 * CS.MIN_PER_CLASS
        for k, fk in CS.FIRST.items():
            np.testing.assert_array_equal(after[k][w], after[fk][w], err_msg=k)


@pytest.mark.parametrize("task,name", CASES)
def test_every_class_is_reached(MK, model, oracle_mod, fx, task, name):
    K, before, after, quiet, phys = _stepped(MK, model, fx, task, name, "f32")
    pre = CS.before_of(before, fx["action"])
    c = CS.census(K, pre, R.step(K, pre, phys, np.float32), phys, fx)
    print(task, name, c)
    assert len(c) >= 20
    short = {k: v for k, v in c.items() if v < CS.MIN_PER_CLASS}
    assert not short, (task, name, short)


def test_contact_band_excludes_no_state(MK, model, oracle_mod, fx, tol):
    """The generator rejected every state with a pair inside the contact band, so where n_frames = 1 the fixture excludes nothing:
    the float32 oracle, the float64 oracle and the stored distances call every pair of every state the same way.  The band is 4 x
    the largest float32-float64 difference over the fixture and not below the bound the plane-primitive GPU test enforces."""
    band = tol["contact_band"]
    assert band["band"] >= 4 * band["max_f32_f64_pair_dist"] and band["band"] >= band["planeprim_dist_bound"] == CS.PLANEPRIM_DIST_BOUND
    assert (np.abs(fx["pair_dist"].astype(np.float64)) >= band["band"]).all()
    for prec in ("f32", "f64"):
        d = MK.contact_data(MK.variant_oracle(model, "Go2Handstand", "shipped_autoreset", prec), fx["qpos"])
        near = np.abs(d[0]) < 1.0
        assert np.abs(d[0] - fx["pair_dist"])[near].max() <= band["max_f32_f64_pair_dist"] + 2 * np.spacing(np.float32(1.0))
        np.testing.assert_array_equal(d[0] < 0, fx["pair_dist"] < 0)
        np.testing.assert_array_equal(d[1], fx["seen12"]); np.testing.assert_array_equal(d[2], fx["cut12"]); np.testing.assert_array_equal(d[3], fx["npen"])
    assert (fx["npen"] > CS.NCON_CAP).sum() >= 6 * CS.MIN_PER_CLASS


@pytest.mark.parametrize("task", list(CS.TASKS))
@pytest.mark.parametrize("name", [v for v in CS.VARIANTS if v.startswith("nf1")])
def test_capped_physics_leaves_the_flags_of_every_pair(MK, model, oracle_mod, fx, task, name):
    """With the oracle's physics capped at the kernel's 12 contacts, its termination and contact-cost flags on the n_frames = 1 states
    are those of the uncapped oracle, on every state: the cap limits the contacts the physics sees, not the pairs the env asks."""
    K = CS.variant_constants(model, task, name, auto_reset=False)
    orc = MK.variant_oracle(model, task, name, "f32", auto_reset=False)
    _, capped = MK.oracle_step(orc, fx, cap=CS.NCON_CAP)
    _, free = MK.oracle_step(orc, fx, cap=1 << 20)
    assert (capped["stats"][:, 3] > 0).sum() >= 6 * CS.MIN_PER_CLASS and not free["stats"][:, 3].any()
    for k in (R.HM_TERM, R.HM_CONTACT):
        np.testing.assert_array_equal(capped["metrics"][:, k], free["metrics"][:, k], err_msg=R.METRIC_NAMES[k])
    unwanted, feet = R.flags_from_pairs(K, fx["pair_dist"])
    np.testing.assert_array_equal(free["metrics"][:, R.HM_CONTACT] != 0, feet)
    assert ((free["metrics"][:, R.HM_TERM] != 0) | ~unwanted).all()


@pytest.mark.parametrize("task", list(CS.TASKS))
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_reset_pose_against_the_oracle(MK, model, oracle_mod, task, p):
    """reset_pose against the oracle's reset: crouch choice, qvel, ctrl and key bit for bit; qpos bit for bit except the yaw quaternion
    (sinf / cosf), which is within 2 ulp32 of a unit quaternion's magnitude."""
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import config
    from rsr_mjx_amd.model import model_fields, pack_blob
    n = 256
    keys = CS.reset_keys(n)
    c = config._merge(config.HANDSTAND_DEFAULT_CONFIG, {"init_from_crouch": p})
    fields = config.handstand_env_fields(model, c, 0, False, variant=CS.TASKS[task])
    f = model_fields(model); f.update(fields)
    orc = oracle_mod.Oracle(pack_blob(f))
    st = orc.new_state(n)
    orc.reset(st, keys)
    K = R.constants(fields, model)
    r32, r64 = R.reset_pose(K, keys, np.float32), R.reset_pose(K, keys, np.float64)
    check_reset(K, st, r32, r64, p)


def check_reset(K, st, r32, r64, p):
    """a record a reset left against reset_pose at both precisions"""
    crouch = st["qpos"][:, 7] == K["home"][19 + 7]
    np.testing.assert_array_equal(crouch, r32["crouch"])
    if p < 1.0:                                                       # a draw that equals p exactly is no crouch start: uniform(key) < p
        edge = r32["ub"] == np.float32(p)
        assert edge.sum() >= 4 and not crouch[edge].any()
    assert crouch.all() if p == 1.0 else (not crouch.any()) if p == 0.0 else (crouch.sum() >= 64 and (~crouch).sum() >= 64)
    assert not st["qvel"][crouch].any() and (p == 1.0 or st["qvel"][~crouch, :6].all())
    for k in ("qvel", "ctrl"):
        np.testing.assert_array_equal(st[k], r32[k].astype(np.float32), err_msg=k)
    np.testing.assert_array_equal(R.key_of(st["info_go2"]), r32["key"])
    rest = np.r_[0:3, 7:19]
    np.testing.assert_array_equal(st["qpos"][:, rest], r32["qpos"][:, rest].astype(np.float32))
    two_ulp = 2 * float(np.spacing(np.float32(1.0)))
    for r in (r32, r64):
        assert np.abs(st["qpos"][:, 3:7].astype(np.float64) - r["qpos"][:, 3:7]).max() <= two_ulp
    assert np.abs(r64["qpos"][:, rest] - st["qpos"][:, rest]).max() <= two_ulp and np.abs(r64["qvel"] - st["qvel"]).max() == 0


def test_fixture_and_tolerances_regenerate(fx, tol, MK):
    """the seeded make script gives the committed arrays byte for byte, and the committed tolerance table"""
    again = MK.generate()
    assert set(again) == set(fx)
    for k in fx:
        assert again[k].dtype == fx[k].dtype and again[k].tobytes() == fx[k].tobytes(), k
    assert MK.tolerances(again) == tol
    assert 300 <= len(fx["cls"]) <= 450 and os.path.getsize(os.path.join(GOLDEN, "handstand_epilogue_states.npz")) < 300 * 1024
