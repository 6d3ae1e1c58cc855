"""The Airbot step outside the physics (cube, sf, T-shape), by branch, on the CPU: the numpy reference (tests/airbot_epilogue_ref.py)
against the oracle's own step, the census of the fixture's branch classes, the threshold bands, and the recorded tolerance table.
tests/test_airbot_epilogue_gpu.py runs the same reference against the HIP kernel.

On the oracle comparison.  oracle/rsr_oracle.c evaluates the Airbot env algebra (step_env, tshape_step_env, wrappers_post) in `float`
in BOTH of its builds -- only the physics is `real`, and it is cast to float before the epilogue reads it -- and the record it hands
back is float32.  A float64 reference therefore cannot meet it at 1e-9.  What is asserted, in both builds and all variants:
  * everything that is integer-valued, a copy or a pass-through word is equal, the restored blocks equal the first state's;
  * the float32 reference -- the oracle's own precision and operation order -- is bit-identical to the oracle in every float quantity
    that does not go through libm's atan2f / sinf / cosf / tanhf / acosf (cases.NOT_BITWISE lists those);
  * the float64 reference is within the bound the GPU module uses (4 x the recorded ref32-ref64 distance of the state's class + 2 ulp32,
    + for xita the allowance for the unpublished geoms) in every float quantity;
  * no state's threshold quantity lies within the exclusion band of its threshold: 0 states are excluded."""
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


@pytest.fixture(scope="module")
def stepped(MK, fx, oracle_mod):
    """{(kind, variant, precision): (K, f, before, after, phys)}: one oracle step of the fixture per kind, variant and build, computed
    once.  The physics results come from the variant's twin without AutoReset where AutoReset would have restored them."""
    cache = {}

    def get(kind, name, prec):
        if (kind, name, prec) not in cache:
            m, f = MK.model(kind), MK.of_kind(fx, kind)
            K = CS.variant_constants(m, kind, name)
            orc = MK.variant_oracle(m, kind, name, prec)
            orc.set_ncon_cap(CS.NCON_CAP[kind])
            before, after = MK.oracle_step(orc, kind, f)
            twin = MK.oracle_step(MK.variant_oracle(m, kind, name, prec, auto_reset=False), kind, f)[1] if K["autoreset"] else after
            cache[kind, name, prec] = (K, f, before, after, CS.phys_of(kind, twin))
        return cache[kind, name, prec]
    return get


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind,name", CASES)
def test_reference_reproduces_the_oracle(stepped, tol, kind, name, prec):
    K, f, before, after, phys = stepped(kind, name, prec)
    names, cls = [str(s) for s in f["class_names"]], f["cls"]
    pre = CS.before_of(before, f["action"])
    got = R.from_record(K, after)
    r64, r32 = R.step(K, pre, phys, np.float64), R.step(K, pre, phys, np.float32)
    live = ~r64["restored"]
    assert K["autoreset"] == bool(r64["restored"].any())
    excluded = CS.excluded_states(K, r32)
    assert not excluded.any(), (kind, name, np.flatnonzero(excluded).tolist())
    fails, report = CS.compare(K, tol[kind][name], names, cls, r64, got, live, excluded)
    same = CS.bitwise(K, r32, got, live, excluded)
    fails += [f"{nm}: not bit-identical to the float32 reference" for nm, ok in same.items() if nm not in CS.NOT_BITWISE and not ok]
    assert not fails, (kind, name, prec, fails)
    # reward and the Episode sums from the oracle's own metrics: sums of published float32 values, so bit for bit
    np.testing.assert_array_equal(after["reward"].reshape(-1), R.reward_from_metrics(K, after["metrics"], r32.get("unpublished_terms", ())))
    if K["episode"]:
        np.testing.assert_array_equal(after["info_episode_metrics"], R.episode_sums_from_outputs(K, pre, after["reward"], after["metrics"]))
    for k in CS.UNTOUCHED[kind]:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    if kind == "sf":                                                   # written before the clamp: bitwise where held
        held = r32["verdicts"]["hold"]
        np.testing.assert_array_equal(after["info_last_action"][held], before["info_last_action"][held])
    w = r64["restored"]
    for k, fk in CS.FIRST.items():
        if K["autoreset"]:
            np.testing.assert_array_equal(after[k][w], after[fk][w], err_msg=k)


@pytest.mark.parametrize("kind,name", CASES)
def test_every_class_is_reached(stepped, kind, name):
    K, f, before, after, phys = stepped(kind, name, "f32")
    pre = CS.before_of(before, f["action"])
    c = CS.census(K, pre, after, R.step(K, pre, phys, np.float32))
    print(kind, name, c)
    assert len(c) >= 35
    short = {k: v for k, v in c.items() if v < CS.MIN_PER_CLASS}
    assert not short, (kind, name, short)


def test_reference_handles_the_bound_the_arm_cannot_reach(stepped):
    """site x > 1.0 (test/airbot.py:227) is beyond the arm's reach, so no fixture state takes it: the reference takes it on an edited
    record, alone, and the other four bounds are shown to be reached by the fixture (test_every_class_is_reached)."""
    K, f, before, after, phys = stepped("sf", "plain", "f32")
    pre = CS.before_of(before, f["action"])
    p2 = {k: np.array(v, copy=True) for k, v in phys.items()}
    sx = p2["site_xpos"].reshape(len(p2["qpos"]), -1, 3)
    assert (np.abs(sx[:, K["ids"][R.ID_SITE], 0]) < 0.8).all()
    sx[:, K["ids"][R.ID_SITE], 2] = 0.9
    base = R.step(K, pre, p2, np.float64)["unpublished_terms"][0]
    w = np.flatnonzero(base == K["W"][2])[:8]
    assert len(w) == 8
    sx[w, K["ids"][R.ID_SITE], 0] = 1.01
    moved = R.step(K, pre, p2, np.float64)["unpublished_terms"][0]
    assert (moved[w] == 0).all() and (np.delete(moved, w) == np.delete(base, w)).all()


def test_fixture_and_tolerances_regenerate(fx, tol, MK):
    """the seeded make script gives the committed arrays byte for byte, and the committed tolerance table"""
    again = MK.generate()
    assert set(again) == set(fx)
    for k in fx:
        assert again[k].dtype == fx[k].dtype and again[k].tobytes() == fx[k].tobytes(), k
    assert MK.tolerances(again) == tol
    for kind in CS.KINDS:
        assert 250 <= len(fx[kind + "__cls"]) <= 450
    assert os.path.getsize(os.path.join(GOLDEN, "airbot_epilogue_states.npz")) < 300 * 1024
