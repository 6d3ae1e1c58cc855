"""bench.py's host side: the State tensors --dump-outputs writes, the 64 MB cap on them, and the options of a plain run."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT
from rsr_mjx_amd.envs.airbot import PipelineState, State


def _state(n, nbody=3):
    rec = torch.arange(n * 40, dtype=torch.float32).reshape(n, 40)
    ps = PipelineState(qpos=rec[:, 0:4], qvel=rec[:, 4:8], ctrl=rec[:, 8:10], qacc_warmstart=rec[:, 10:14], time=rec[:, 14],
                       xpos=rec[:, 15:15 + 3 * nbody].unflatten(1, (nbody, 3)), site_xpos=rec[:, 24:27].unflatten(1, (1, 3)))
    st = State(pipeline_state=ps, obs=rec[:, 27:33], reward=rec[:, 33], done=rec[:, 34], metrics={"dist": rec[:, 35]},
               info={"steps": rec[:, 36], "episode_metrics": {"sum_reward": rec[:, 37]}, "first_pipeline_state": ps})
    st.data = ps                        # Go2: the same physics state under its Playground name
    st.obs_dict = {"state": st.obs, "privileged_state": rec[:, 38:40]}
    return st


def test_state_arrays_names_every_tensor_once():
    st = _state(4)
    a = bench.state_arrays(st)
    assert set(a) == {"pipeline_state.qpos", "pipeline_state.qvel", "pipeline_state.ctrl", "pipeline_state.qacc_warmstart",
                      "pipeline_state.time", "pipeline_state.xpos", "pipeline_state.site_xpos", "obs", "reward", "done",
                      "metrics.dist", "info.steps", "info.episode_metrics.sum_reward", "obs_dict.privileged_state"}
    assert a["obs"] is st.obs and a["pipeline_state.xpos"].shape == (4, 3, 3)


def test_dump_outputs_writes_float32_and_float64(tmp_path):
    st = _state(5)
    per_env = dict(bench.state_arrays(st), stats=torch.ones((5, 4), dtype=torch.int32))
    shared = {"rollout_metrics": torch.tensor([[5.0, 1.5, 0.0, 2.0]], dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path), per_env, shared, 5)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in [*per_env, *shared])
    assert np.load(tmp_path / "rollout_metrics.npy").dtype == np.float64
    assert np.load(tmp_path / "stats.npy").dtype == np.float32
    np.testing.assert_array_equal(np.load(tmp_path / "obs.npy"), st.obs.numpy())


def test_dump_outputs_keeps_a_fixed_sample_under_the_cap(tmp_path):
    n = 1000
    st = _state(n)
    limit = 20_000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), bench.state_arrays(st), {"rollout_metrics": torch.zeros((1, 4))}, n, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert "env_index.npy" in files
    idx = np.load(tmp_path / "a" / "env_index.npy").astype(np.int64)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= limit
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "obs.npy"), st.obs.numpy()[idx])
    assert np.load(tmp_path / "a" / "rollout_metrics.npy").shape == (1, 4)


def test_dump_outputs_never_samples_shared_arrays(tmp_path):
    """Shared arrays are written whole even when their leading dimension happens to equal the env count (--envs == GPU count)."""
    n = 4
    per_env = {"obs": torch.arange(n * 2000, dtype=torch.float32).reshape(n, 2000)}
    shared = {"rollout_metrics": torch.arange(n * 4, dtype=torch.float32).reshape(n, 4)}
    bench.dump_outputs(str(tmp_path), per_env, shared, n, limit=20_000)
    assert len(np.load(tmp_path / "env_index.npy")) < n
    np.testing.assert_array_equal(np.load(tmp_path / "rollout_metrics.npy"), shared["rollout_metrics"].numpy())
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "x"), {"bad": torch.zeros(3)}, {}, n)


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout and "--steps" in out.stdout
