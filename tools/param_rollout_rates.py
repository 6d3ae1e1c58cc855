"""Parameter rollouts (rsr_physics_param_rollouts) against sampled rollouts (rsr_physics_sample_rollouts) at the same M x K: what
the overlay of per-sample model leaves costs.  Per model family, from the state M envs are in after a reset and a few env steps:
arm A is Physics.param_rollouts with every leaf the family supports sampled (nine on the Go2 models, four on the Airbot ones,
within 5 % of each env's own value) and one ctrl sequence shared by an env's K samples; arm B is Physics.sample_rollouts with
that sequence repeated per sample and the env's own leaves, the kernel of the parent commit.  Both record sensordata only, run
T control steps of nsteps = n_frames and are timed with HIP events on the launch stream (rsr_timing_begin / _end), one warm-up
round then `reps` rounds alternating the arms in one process.  The trajectories differ (the leaves do), so the solver's iteration
counts may too; --leaf-spread 0 samples every leaf at exactly the env's own value, so that both arms do the same arithmetic
(`differ` is then false) and only the overlay is left between them.  One JSON line per (family, M, K).
Usage: python tools/param_rollout_rates.py [--sizes 64x128,1024x8] [--T 32] [--reps 7] [--leaf-spread 0.05] [--out FILE]"""
from __future__ import annotations

import argparse

import numpy as np

import rates_support as R

LEAVES = ["geom_friction", "body_mass", "dof_damping", "dof_frictionloss"]
GO2_LEAVES = ["body_ipos", "qpos0", "dof_armature", "actuator_gainprm", "actuator_biasprm"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x128,1024x8", help="MxK pairs")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leaf-spread", type=float, default=0.05, help="leaves are the env's own times U(1 - s, 1 + s); 0: the env's own")
    ap.add_argument("--families", default="cube,tshape,go2flat,go2rough,footstand")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M, K)")
    args = ap.parse_args()
    import torch
    import bench
    from physics_support import IMPLICIT
    from rsr_mjx_amd.physics import Physics
    T, write = args.T, R.row_writer(args.out)
    for m, k in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, m)
            envdef, env, dr, rng = b.envdef, b.env, b.dr, b.rng
            names = LEAVES if kind in IMPLICIT else LEAVES + GO2_LEAVES
            phys = Physics(env, sensors=b.spec)
            nf, nsd = phys.n_substeps, phys.nsensordata
            # one noisy sequence per env around the ctrl the env steps left; arm B gets it once per sample
            base = env.view("ctrl").clone()
            shared = (base[:, None, :] + torch.as_tensor(rng.normal(scale=0.05, size=(m, T, env.dims.nu)).astype(np.float32),
                                                         device=env.device)).contiguous()
            each = shared[:, None].expand(m, k, T, env.dims.nu).contiguous()
            # every leaf within leaf_spread of the env's own value (its per-env one, or the model's)
            arr, params = envdef.sys.arrays, {}
            for f in names:
                own = np.asarray(dr[f], np.float32) if dr is not None else np.tile(arr[f].astype(np.float32)[None], (m,) + (1,) * arr[f].ndim)
                v = own[:, None] * rng.uniform(1.0 - args.leaf_spread, 1.0 + args.leaf_spread, size=(m, k) + own.shape[1:])
                params[f] = torch.as_tensor(v.astype(np.float32), device=env.device).contiguous()
            out_a = {"sensordata": torch.empty((m, k, T, nsd), device=env.device)}
            out_b = {"sensordata": torch.empty((m, k, T, nsd), device=env.device)}
            torch.cuda.synchronize()
            t_a, t_b = R.alternate([R.Arm(lambda: phys.param_rollouts(shared, params, nf, fields=("sensordata",), out=out_a), env),
                                    R.Arm(lambda: phys.sample_rollouts(each, nf, fields=("sensordata",), out=out_b), env)], args.reps)
            med = R.median
            row = dict(family=kind, M=m, K=k, T=T, nsteps=nf, nsensordata=nsd, leaves=len(names), leaf_spread=args.leaf_spread, csrc_sha16=bench.csrc_sha16(),
                       param_ms=med(t_a), sample_ms=med(t_b), param_over_sample=med(t_a) / med(t_b),
                       param_env_steps_per_s=m * k * T / (med(t_a) * 1e-3),
                       spread=R.spread(t_a, t_b), reps=args.reps,
                       differ=not bool(torch.equal(out_a["sensordata"], out_b["sensordata"])),
                       finite=bool(torch.isfinite(out_a["sensordata"]).all()))
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
