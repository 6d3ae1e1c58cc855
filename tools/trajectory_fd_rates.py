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

import numpy as np

import rates_support as R


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
    from rsr_mjx_amd.physics import Physics
    T, write = args.T, R.row_writer(args.out)
    for m in (int(v) for v in args.sizes.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, m)
            env, rng = b.env, b.rng
            phys = Physics(env, sensors=b.spec)
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

            def by_calls():                                       # arm B; putting the record back is part of what it costs
                for t in range(T):
                    phys.ctrl.copy_(steps[t])
                    phys.transition_fd(nsteps=nf, eps=args.eps)
                    loop[t].copy_(fd_cols[:, :, :w])
                    phys.step(steps[t], nf)
                env.record.copy_(start)
            t_a, t_b = R.alternate([R.Arm(lambda: phys.trajectory_fd(ctrl, nf, eps=args.eps, nominal=False, out=out_a), env),
                                    R.Arm(by_calls, env)], args.reps)
            med = R.median
            same = bool(torch.equal(out_a["columns"].view(torch.int32), loop.transpose(0, 1).contiguous().view(torch.int32)))
            row = dict(family=kind, M=m, T=T, nsteps=nf, ncol=ncol, nsensordata=nsd, eps=args.eps, csrc_sha16=bench.csrc_sha16(),
                       trajectory_fd_ms=med(t_a), loop_ms=med(t_b), loop_over_trajectory_fd=med(t_b) / med(t_a),
                       columns_per_s=m * T * ncol / (med(t_a) * 1e-3),
                       spread=R.spread(t_a, t_b), reps=args.reps,
                       bitwise_equal=same, finite=bool(torch.isfinite(out_a["columns"]).all()))
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
