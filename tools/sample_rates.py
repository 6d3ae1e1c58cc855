"""Sampled rollouts (rsr_physics_sample_rollouts) against what a planner had to do without them: Physics.rollout on a replica batch
of M * K envs that hold the same record rows and per-env leaves.  Per model family, K control sequences of T control steps of
nsteps = n_frames from the state M envs are in after a reset and a few env steps.  Both arms record sensordata only (what a
planner's cost reads), do the same arithmetic and are timed with HIP events on the launch stream (rsr_timing_begin / _end),
warmed up, alternating within one process; the replica arm's time leaves out building the replica batch and copying the M * K
record rows into it, which a planner would pay at every planning step (restore_ms: the copy alone, wall clock).  One JSON line per
(family, M, K).
Usage: python tools/sample_rates.py [--sizes 64x128,1024x8] [--T 32] [--reps 7] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x128,1024x8", help="MxK pairs")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--families", default="cube,tshape,go2flat,go2rough,footstand")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M, K)")
    args = ap.parse_args()
    import torch
    import bench
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.physics import Physics
    T, rows = args.T, []
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()
    for m, k in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        for kind in args.families.split(","):
            if kind in ("cube", "tshape"):
                envdef = airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
                dr = airbot.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(5), m)) if kind == "cube" else None
                spec, scale = [("pos", "framepos", "endpoint"), ("linvel", "framelinvel", "endpoint")], 1.0
            else:
                envdef = go2.load({"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain",
                                   "footstand": "Go2Footstand"}[kind])
                dr = go2.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(12), m))
                spec, scale = envdef.sensors, 0.5
            env = envdef.batched(m, randomization=dr)
            env.reset(prng.split(prng.PRNGKey(0), m))
            rng = np.random.default_rng(0)
            for _ in range(3):
                env.step(None, np.clip(rng.normal(size=(m, env.dims.nu)) * scale, -1, 1).astype(np.float32))
            rep = envdef.batched(m * k, randomization=None if dr is None else {f: np.repeat(np.asarray(v), k, 0) for f, v in dr.items()})
            rep.reset(prng.split(prng.PRNGKey(0), m * k))
            phys, prep = Physics(env, sensors=spec), Physics(rep, sensors=spec)
            nf, nsd = phys.n_substeps, phys.nsensordata
            # K noisy sequences around the ctrl the env steps left
            base = env.view("ctrl").clone()
            ctrl = (base[:, None, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(m, k, T, env.dims.nu)).astype(np.float32),
                                                             device=env.device)).contiguous()
            flat = ctrl.reshape(m * k, T, env.dims.nu)
            out_s = {"sensordata": torch.empty((m, k, T, nsd), device=env.device)}
            out_r = {"sensordata": torch.empty((m * k, T, nsd), device=env.device)}
            torch.cuda.synchronize()
            t_s, t_r, t_copy = [], [], []
            for r in range(args.reps + 1):                        # (the first round warms both arms up)
                env.timing_begin(); phys.sample_rollouts(ctrl, nf, fields=("sensordata",), out=out_s); ms, _ = env.timing_end()
                if r: t_s.append(ms)
                torch.cuda.synchronize()
                t0 = time.perf_counter(); rep.record.copy_(env.record.repeat_interleave(k, 0)); torch.cuda.synchronize()
                if r: t_copy.append((time.perf_counter() - t0) * 1e3)
                rep.timing_begin(); prep.rollout(flat, nf, fields=("sensordata",), out=out_r); ms, _ = rep.timing_end()
                if r: t_r.append(ms)
                torch.cuda.synchronize()
            same = bool(torch.equal(out_s["sensordata"].view(torch.int32).reshape(m * k, T, nsd), out_r["sensordata"].view(torch.int32)))
            med = lambda x: float(np.median(x))
            row = dict(family=kind, M=m, K=k, T=T, nsteps=nf, nsensordata=nsd, csrc_sha16=bench.csrc_sha16(),
                       sample_ms=med(t_s), replica_rollout_ms=med(t_r), replica_over_sample=med(t_r) / med(t_s),
                       restore_ms=med(t_copy), sample_env_steps_per_s=m * k * T / (med(t_s) * 1e-3),
                       spread=[min(t_s), max(t_s), min(t_r), max(t_r)], reps=args.reps,
                       bitwise_equal=same, finite=bool(torch.isfinite(out_s["sensordata"]).all()))
            print(json.dumps(row), flush=True)
            rows.append(row)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del phys, prep, env, rep
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
