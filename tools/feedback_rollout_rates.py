"""Closed-loop rollouts (rsr_physics_feedback_rollouts) against parameter rollouts (rsr_physics_param_rollouts) at the same M x K:
what the control law at every control-step boundary costs.  Per model family, from the state M envs are in after a reset and a
few env steps: arm A is Physics.param_rollouts with per-sample ctrl [M, K, T, nu] and the env's own leaves; arm B is
Physics.feedback_rollouts on the same ctrl with non-zero per-sample gains (N(0, 1) x 2 % of each actuator's ctrl range per unit of
state error), the refs the state the rollout starts from, and the clamp on, so that the controls stay in the range over the T
steps.  Both record sensordata only, run T control steps of nsteps = n_frames and are timed with HIP events on the launch stream
(rsr_timing_begin / _end), one warm-up round then `reps` rounds alternating the arms in one process.  The trajectories differ (the
controls do), so the solver's iteration counts may too.  One JSON line per (family, M, K).
Usage: python tools/feedback_rollout_rates.py [--sizes 8x8,128x8] [--T 32] [--reps 7] [--families cube,go2flat] [--out FILE]"""
from __future__ import annotations

import argparse

import numpy as np

import rates_support as R


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
            # one noisy sequence per sample around the ctrl the env steps left
            base = env.view("ctrl").clone()
            each = (base[:, None, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(m, k, T, nu)).astype(np.float32),
                                                             device=env.device)).contiguous()
            rg = envdef.sys.arrays["actuator_ctrlrange"]
            g = args.gain * (rg[:, 1] - rg[:, 0])[:, None]
            gain = torch.as_tensor((rng.normal(size=(m, k, T, nu, 2 * nv)) * g).astype(np.float32), device=env.device).contiguous()
            qref = phys.qpos[:, None, None, :].expand(m, k, T, nq).contiguous()
            vref = phys.qvel[:, None, None, :].expand(m, k, T, nv).contiguous()
            out_a = {"sensordata": torch.empty((m, k, T, nsd), device=env.device)}
            out_b = {"sensordata": torch.empty((m, k, T, nsd), device=env.device)}
            torch.cuda.synchronize()
            t_a, t_b = R.alternate([
                R.Arm(lambda: phys.param_rollouts(each, {}, nf, fields=("sensordata",), out=out_a), env),
                R.Arm(lambda: phys.feedback_rollouts(each, gain, qref, vref, nsteps=nf, fields=("sensordata",), clamp=True, out=out_b), env)], args.reps)
            med = R.median
            row = dict(family=kind, M=m, K=k, T=T, nsteps=nf, nsensordata=nsd, gain=args.gain, clamp=True, csrc_sha16=bench.csrc_sha16(),
                       param_ms=med(t_a), feedback_ms=med(t_b), feedback_over_param=med(t_b) / med(t_a),
                       feedback_env_steps_per_s=m * k * T / (med(t_b) * 1e-3),
                       spread=R.spread(t_a, t_b), reps=args.reps,
                       differ=not bool(torch.equal(out_a["sensordata"], out_b["sensordata"])),
                       finite=bool(torch.isfinite(out_b["sensordata"]).all()))
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
