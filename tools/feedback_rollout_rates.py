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
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.physics import Physics
    T = args.T
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
            phys = Physics(env, sensors=spec)
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
            t_a, t_b = [], []
            for r in range(args.reps + 1):                        # (the first round warms both arms up)
                env.timing_begin(); phys.param_rollouts(each, {}, nf, fields=("sensordata",), out=out_a); ms, _ = env.timing_end()
                if r: t_a.append(ms)
                torch.cuda.synchronize()
                env.timing_begin(); phys.feedback_rollouts(each, gain, qref, vref, nsteps=nf, fields=("sensordata",), clamp=True, out=out_b); ms, _ = env.timing_end()
                if r: t_b.append(ms)
                torch.cuda.synchronize()
            med = lambda x: float(np.median(x))
            row = dict(family=kind, M=m, K=k, T=T, nsteps=nf, nsensordata=nsd, gain=args.gain, clamp=True, csrc_sha16=bench.csrc_sha16(),
                       param_ms=med(t_a), feedback_ms=med(t_b), feedback_over_param=med(t_b) / med(t_a),
                       feedback_env_steps_per_s=m * k * T / (med(t_b) * 1e-3),
                       spread=[min(t_a), max(t_a), min(t_b), max(t_b)], reps=args.reps,
                       differ=not bool(torch.equal(out_a["sensordata"], out_b["sensordata"])),
                       finite=bool(torch.isfinite(out_b["sensordata"]).all()))
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del phys, env
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
