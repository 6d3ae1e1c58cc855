"""Physics-only env-steps/s per model family (rsr_physics_step with nsteps = n_frames) beside the fused env step (rsr_step), both
timed with HIP events on the launch stream (rsr_timing_begin / rsr_timing_end).  One JSON line per family; --out also writes them
to a file.  Usage: python tools/physics_rates.py [--envs 8192] [--steps 50] [--warmup 10] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--families", default="cube,tshape,go2flat,go2rough,footstand")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.physics import Physics
    n = args.envs
    rows = []
    for kind in args.families.split(","):
        if kind in ("cube", "tshape"):
            envdef = airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
            dr = airbot.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(5), n)) if kind == "cube" else None
            scale = 1.0
        else:
            envdef = go2.load({"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain", "footstand": "Go2Footstand"}[kind])
            dr = go2.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(12), n))
            scale = 0.5
        env = envdef.batched(n, episode_length=1000, auto_reset=True, randomization=dr)
        env.reset(prng.split(prng.PRNGKey(0), n))
        rng = np.random.default_rng(0)
        acts = [torch.as_tensor(np.clip(rng.normal(size=(n, env.dims.nu)) * scale, -1, 1).astype(np.float32), device=env.device)
                for _ in range(8)]
        # fused env step
        for i in range(args.warmup):
            env.step(None, acts[i % 8])
        env.timing_begin()
        for i in range(args.steps):
            env.step(None, acts[i % 8])
        ms_env, launches = env.timing_end()
        ms_env /= launches
        # physics-only step of n_frames substeps from the states the rollout reached, under the ctrl the env step last wrote
        phys = Physics(env)
        ctrl = env.view("ctrl").clone()
        for _ in range(args.warmup):
            phys.step(ctrl)
        env.timing_begin()
        for _ in range(args.steps):
            phys.step(ctrl)
        ms_phys, launches = env.timing_end()
        ms_phys /= launches
        finite = bool(torch.isfinite(env.view("qpos")).all())
        row = dict(family=kind, num_envs=n, n_frames=int(env.dims.n_frames), env_step_ms=ms_env, physics_step_ms=ms_phys,
                   env_steps_per_s=n / (ms_env * 1e-3), physics_env_steps_per_s=n / (ms_phys * 1e-3),
                   physics_over_env=ms_phys / ms_env, finite=finite)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del phys, env
        torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
