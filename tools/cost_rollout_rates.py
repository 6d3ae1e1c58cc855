"""Cost rollouts (rsr_physics_cost_rollouts) against closed-loop rollouts that record what a host-side cost would have to read
(rsr_physics_feedback_rollouts), on the same inputs at the same M x K: what forming the running cost on the device costs or saves.
Per model family, from the state M envs are in after a reset and a few env steps, with the ctrl, gains, refs and clamp of
tools/feedback_rollout_rates.py: arm A is Physics.feedback_rollouts recording qpos, qvel, sensordata and the applied ctrl
[M, K, T, w]; arm B is Physics.cost_rollouts with all four terms (weights uniform in (0.5, 2), the refs the start state, zero ctrl
and sensor refs) and `cost` [M, K] alone.  Arm A's time is the launch only: the reduction of its rows to M K numbers, which a
planner still has to run, is not in it.  Both run T control steps of nsteps = n_frames and are timed with HIP events on the launch
stream (rsr_timing_begin / _end), one warm-up round then `reps` rounds alternating the arms in one process.  The trajectories are
the same bit for bit (tests/test_cost_rollouts_gpu.py), so the solver does the same work in both.  One JSON line per (family, M, K).
Usage: python tools/cost_rollout_rates.py [--sizes 8x8,128x8] [--T 32] [--reps 7] [--families cube,go2flat] [--out FILE]"""
from __future__ import annotations

import argparse

import numpy as np

import rates_support as R

RECORDED = ("qpos", "qvel", "sensordata", "ctrl")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8x8,128x8", help="MxK pairs")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gain", type=float, default=0.02, help="gains are N(0, 1) times this share of the actuator's ctrl range")
    ap.add_argument("--families", default="cube,go2flat")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M, K)")
    args = ap.parse_args()
    import torch
    import bench
    from rsr_mjx_amd.physics import Physics
    T, write = args.T, R.row_writer(args.out)
    for m, k in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, m)
            envdef, env, rng = b.envdef, b.env, b.rng
            phys = Physics(env, sensors=b.spec)
            nf, nsd = phys.n_substeps, phys.nsensordata
            nq, nv, nu = int(env.dims.nq), int(env.dims.nv), int(env.dims.nu)
            dev = env.device
            # one noisy sequence per sample around the ctrl the env steps left
            base = env.view("ctrl").clone()
            each = (base[:, None, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(m, k, T, nu)).astype(np.float32), device=dev)).contiguous()
            rg = envdef.sys.arrays["actuator_ctrlrange"]
            g = args.gain * (rg[:, 1] - rg[:, 0])[:, None]
            gain = torch.as_tensor((rng.normal(size=(m, k, T, nu, 2 * nv)) * g).astype(np.float32), device=dev).contiguous()
            qref = phys.qpos[:, None, None, :].expand(m, k, T, nq).contiguous()
            vref = phys.qvel[:, None, None, :].expand(m, k, T, nv).contiguous()
            weight = lambda w: torch.as_tensor(rng.uniform(0.5, 2.0, size=(m, T, w)).astype(np.float32), device=dev)
            cost = dict(qpos_ref=qref[:, 0].contiguous(), qvel_ref=vref[:, 0].contiguous(), w_qpos=weight(nv), w_qvel=weight(nv), w_ctrl=weight(nu),
                        w_sensor=weight(nsd))
            fb = dict(gain=gain, qpos_ref=qref, qvel_ref=vref)
            width = dict(qpos=nq, qvel=nv, sensordata=nsd, ctrl=nu)
            out_a = {f: torch.empty((m, k, T, width[f]), device=dev) for f in RECORDED}
            out_b = {"cost": torch.empty((m, k), device=dev)}
            torch.cuda.synchronize()
            t_a, t_b = R.alternate([
                R.Arm(lambda: phys.feedback_rollouts(each, gain, qref, vref, nsteps=nf, fields=RECORDED, clamp=True, out=out_a), env),
                R.Arm(lambda: phys.cost_rollouts(each, cost, feedback=fb, nsteps=nf, clamp=True, out=out_b), env)], args.reps)
            med = R.median
            # the two arms ran the same rollout: one more cost call that records arm A's rows gives them and arm B's cost, bit for bit
            same = phys.cost_rollouts(each, cost, feedback=fb, nsteps=nf, clamp=True, fields=RECORDED)
            row = dict(family=kind, M=m, K=k, T=T, nsteps=nf, nsensordata=nsd, gain=args.gain, clamp=True, csrc_sha16=bench.csrc_sha16(),
                       recorded=list(RECORDED), recorded_floats_per_sample=T * sum(width.values()),
                       feedback_ms=med(t_a), cost_ms=med(t_b), cost_over_feedback=med(t_b) / med(t_a),
                       cost_env_steps_per_s=m * k * T / (med(t_b) * 1e-3),
                       spread=R.spread(t_a, t_b), reps=args.reps,
                       same_rows=all(bool(torch.equal(same[f], out_a[f])) for f in RECORDED),
                       same_cost=bool(torch.equal(same["cost"], out_b["cost"])),
                       finite=bool(torch.isfinite(out_b["cost"]).all()))
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
