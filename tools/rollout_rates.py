"""Rollout kernel (rsr_physics_rollout) against T x rsr_physics_step, per model family, T control steps of nsteps = n_frames.
Two comparisons, one JSON line per (family, batch size):
  kernel: one rollout launch vs T step launches, both timed with HIP events on the launch stream (rsr_timing_begin / _end;
          the rollout records qpos / qvel / time);
  python: trajectory collection as a user writes it, wall clock around torch.cuda.synchronize: Physics.rollout(ctrl) vs a loop
          of Physics.step(ctrl[:, t]) that clones qpos and qvel each step and stacks them.
Usage: python tools/rollout_rates.py [--envs 8192,1024] [--T 50] [--reps 5] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np

import rates_support as R


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="8192,1024")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--families", default="cube,tshape,go2flat,go2rough,footstand")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from rsr_mjx_amd.physics import Physics
    T, rows = args.T, []
    for n in (int(x) for x in args.envs.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, n, steps=0)
            env, rng = b.env, b.rng
            phys = Physics(env)
            nf = phys.n_substeps
            # controls around the state the reset left (the env's home ctrl plus a small perturbation): stays in range for T steps
            base = env.view("ctrl").clone()
            ctrl = (base[:, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(n, T, env.dims.nu)).astype(np.float32),
                                                       device=env.device)).contiguous()
            q0, v0, c0 = phys.qpos.clone(), phys.qvel.clone(), phys.ctrl.clone()

            def restart():                                        # ahead of every arm, in no window
                phys.set_state(q0, v0, c0); torch.cuda.synchronize()

            def step_loop(record):
                qs, vs = [], []
                for t in range(T):
                    phys.step(ctrl[:, t], nf)
                    if record:
                        qs.append(phys.qpos.clone()); vs.append(phys.qvel.clone())
                return (torch.stack(qs, 1), torch.stack(vs, 1)) if record else None

            out = {f: torch.empty((n, T, w), device=env.device) for f, w in (("qpos", env.dims.nq), ("qvel", env.dims.nv), ("time", 1))}
            # kernel time: HIP events around the launches only
            k_roll, k_step = R.alternate([restart, R.Arm(lambda: phys.rollout(ctrl, nf, out=out), env),
                                          restart, R.Arm(lambda: step_loop(False), env)], args.reps)
            # Python level: wall clock of collecting a qpos / qvel trajectory
            p_roll, p_step = [], []
            for rep in range(args.reps + 1):
                restart()
                t0 = time.perf_counter(); tr = phys.rollout(ctrl, nf, fields=("qpos", "qvel")); torch.cuda.synchronize()
                if rep: p_roll.append((time.perf_counter() - t0) * 1e3)
                restart()
                t0 = time.perf_counter(); ts = step_loop(True); torch.cuda.synchronize()
                if rep: p_step.append((time.perf_counter() - t0) * 1e3)
            same = bool(torch.equal(tr["qpos"].view(torch.int32), ts[0].view(torch.int32))
                        and torch.equal(tr["qvel"].view(torch.int32), ts[1].view(torch.int32)))
            med = R.median
            row = dict(family=kind, num_envs=n, T=T, nsteps=nf, csrc_sha16=bench.csrc_sha16(),
                       kernel_rollout_ms=med(k_roll), kernel_steps_ms=med(k_step),
                       kernel_speedup=med(k_step) / med(k_roll),
                       python_rollout_ms=med(p_roll), python_step_loop_ms=med(p_step),
                       python_speedup=med(p_step) / med(p_roll),
                       rollout_env_steps_per_s=n * T / (med(k_roll) * 1e-3),
                       kernel_spread=R.spread(k_roll, k_step),
                       bitwise_equal=same, finite=bool(torch.isfinite(tr["qpos"]).all()))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del phys, env, b
            torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
