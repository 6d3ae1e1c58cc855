"""Transition Jacobians along a trajectory (rsr_physics_trajectory_fd) against the loop the calls before it allow.  Per model family,
from the state M envs are in after a reset and a few env steps, with one control sequence [M, T, nu] per env: arm A is
Physics.trajectory_fd (two launches: the nominal run, then every column of every control step); arm B is, for t < T, ctrl[:, t]
into the record, Physics.transition_fd, a clone of its columns, Physics.step(ctrl[:, t]), and at the end the record put back:
2 T dependent launches of M x ncol and M waves, and the copies between them.  Both run T control steps of nsteps = n_frames,
centred, at the same eps, and are timed with HIP events on the launch stream (rsr_timing_begin / _end), one warm-up round then
`reps` rounds alternating the arms in one process.  The two arms' columns are compared bit for bit.  One JSON line per (family, M).
Usage: python tools/trajectory_fd_rates.py [--sizes 1,16,256] [--T 32] [--reps 7] [--families cube,go2flat] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256", help="M: envs, all of them listed")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--families", default="cube,go2flat")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M)")
    args = ap.parse_args()
    import torch
    import bench
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.physics import Physics
    T = args.T
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()
    for m in (int(v) for v in args.sizes.split(",")):
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
            phys = Physics(env, sensors=spec)
            nf, nsd = phys.n_substeps, phys.nsensordata
            nv, nu = int(env.dims.nv), int(env.dims.nu)
            ncol, w = 2 * nv + nu, 2 * nv + nsd
            # one noisy sequence per env around the ctrl the env steps left
            ctrl = (env.view("ctrl").clone()[:, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(m, T, nu)).astype(np.float32),
                                                                           device=env.device)).contiguous()
            steps = [ctrl[:, t].contiguous() for t in range(T)]
            out_a = {"columns": torch.empty((m, T, ncol, w), device=env.device)}
            loop = torch.empty((T, m, ncol, w), device=env.device)
            fd_cols = phys._fd_view("columns")                     # [M, ncol, 2 nv + RSR_MAX_SENSORDATA]
            torch.cuda.synchronize()
            start = env.record.clone()
            t_a, t_b = [], []
            for r in range(args.reps + 1):                        # (the first round warms both arms up)
                env.timing_begin()
                phys.trajectory_fd(ctrl, nf, eps=args.eps, nominal=False, out=out_a)
                ms, _ = env.timing_end()
                if r: t_a.append(ms)
                torch.cuda.synchronize()
                env.timing_begin()
                for t in range(T):
                    phys.ctrl.copy_(steps[t])
                    phys.transition_fd(nsteps=nf, eps=args.eps)
                    loop[t].copy_(fd_cols[:, :, :w])
                    phys.step(steps[t], nf)
                env.record.copy_(start)
                ms, _ = env.timing_end()
                if r: t_b.append(ms)
                torch.cuda.synchronize()
            med = lambda x: float(np.median(x))
            same = bool(torch.equal(out_a["columns"].view(torch.int32), loop.transpose(0, 1).contiguous().view(torch.int32)))
            row = dict(family=kind, M=m, T=T, nsteps=nf, ncol=ncol, nsensordata=nsd, eps=args.eps, csrc_sha16=bench.csrc_sha16(),
                       trajectory_fd_ms=med(t_a), loop_ms=med(t_b), loop_over_trajectory_fd=med(t_b) / med(t_a),
                       columns_per_s=m * T * ncol / (med(t_a) * 1e-3),
                       spread=[min(t_a), max(t_a), min(t_b), max(t_b)], reps=args.reps,
                       bitwise_equal=same, finite=bool(torch.isfinite(out_a["columns"]).all()))
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del phys, env
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
