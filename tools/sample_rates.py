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
import time

import numpy as np

import rates_support as R


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
    from physics_support import replica
    from rsr_mjx_amd.physics import Physics
    T, write = args.T, R.row_writer(args.out)
    for m, k in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, m)
            env, rng = b.env, b.rng
            rep = replica(kind, b.envdef, env, k, dr=b.dr)
            phys, prep = Physics(env, sensors=b.spec), Physics(rep, sensors=b.spec)
            nf, nsd = phys.n_substeps, phys.nsensordata
            # K noisy sequences around the ctrl the env steps left
            base = env.view("ctrl").clone()
            ctrl = (base[:, None, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(m, k, T, env.dims.nu)).astype(np.float32),
                                                             device=env.device)).contiguous()
            flat = ctrl.reshape(m * k, T, env.dims.nu)
            out_s = {"sensordata": torch.empty((m, k, T, nsd), device=env.device)}
            out_r = {"sensordata": torch.empty((m * k, T, nsd), device=env.device)}
            torch.cuda.synchronize()
            t_copy = []

            def restore():                                        # between the arms, in no window: the copy alone, wall clock
                t0 = time.perf_counter(); rep.record.copy_(env.record.repeat_interleave(k, 0)); torch.cuda.synchronize()
                t_copy.append((time.perf_counter() - t0) * 1e3)
            t_s, t_r = R.alternate([R.Arm(lambda: phys.sample_rollouts(ctrl, nf, fields=("sensordata",), out=out_s), env), restore,
                                    R.Arm(lambda: prep.rollout(flat, nf, fields=("sensordata",), out=out_r), rep)], args.reps)
            same = bool(torch.equal(out_s["sensordata"].view(torch.int32).reshape(m * k, T, nsd), out_r["sensordata"].view(torch.int32)))
            med = R.median
            row = dict(family=kind, M=m, K=k, T=T, nsteps=nf, nsensordata=nsd, csrc_sha16=bench.csrc_sha16(),
                       sample_ms=med(t_s), replica_rollout_ms=med(t_r), replica_over_sample=med(t_r) / med(t_s),
                       restore_ms=med(t_copy[1:]), sample_env_steps_per_s=m * k * T / (med(t_s) * 1e-3),
                       spread=R.spread(t_s, t_r), reps=args.reps,
                       bitwise_equal=same, finite=bool(torch.isfinite(out_s["sensordata"]).all()))
            write(row)
            del phys, prep, env, rep, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
