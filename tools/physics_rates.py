"""Physics-only env-steps/s per model family (rsr_physics_step with nsteps = n_frames) beside the fused env step (rsr_step), both
timed with HIP events on the launch stream (rsr_timing_begin / rsr_timing_end).  One JSON line per family; --out also writes them
to a file.  --applied adds the rates with applied forces on (Physics.set_applied: a non-zero xfrc on every body and a qfrc on every
dof), for the step and for a rollout of --rollout-T control steps, beside the plain ones.  --dynamics adds ms per
rsr_physics_dynamics launch without Jacobian sites and with the family's example sites, beside ms per rsr_physics_forward launch
on the same batch.  --constraint adds ms per rsr_physics_constraint launch (Physics.constraint_forces) beside ms per
rsr_physics_forward launch, interleaved in blocks on the same batch and state (of the state, forward moves qacc_warmstart only).
--transition is a mode of its own: per family and for N = 64, 1024 and 8192 envs it times Physics.transition_fd at its defaults
beside the 2 ncol Physics.step launches that do the same work from Python, each after a restore of the record, in alternating
blocks on the same batch and state, and writes one row per family to profiles/transition_rates_<N>.jsonl (--out-dir).
--inverse is a mode of its own too: per family and for N = 1024 and 8192 envs, HIP events around --steps launches after --warmup
warm-up launches of Physics.inverse (at the qacc of the last forward pass), Physics.constraint_forces and Physics.dynamics (no
Jacobian sites) on the same batch and state, none of which moves the state; one row per family to profiles/inverse_rates_<N>.jsonl.
Usage: python tools/physics_rates.py [--envs 8192] [--steps 50] [--warmup 10] [--applied] [--dynamics] [--constraint]
                                     [--rollout-T 16] [--out FILE]
       python tools/physics_rates.py --transition [--transition-envs 64,1024,8192] [--families ...] [--out-dir profiles]
       python tools/physics_rates.py --inverse [--inverse-envs 1024,8192] [--families ...] [--out-dir profiles]"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

import rates_support as R

BATCH = dict(episode_length=1000, auto_reset=True)


def per_call(env, fn, args, per=1):
    """ms per call of one arm alone, fn(i) with i the call's index in its phase: args.warmup untimed calls, then one window of
    args.steps (forward, dynamics and the like do not count as env launches: the window is divided by the calls)"""
    for i in range(args.warmup):
        fn(i)
    calls = iter(range(args.steps))
    return R.alternate([R.Arm(lambda: fn(next(calls)), env, args.steps)], 1, warmup=0)[0][0] / per


def transition_rates(args) -> None:
    """ms per Physics.transition_fd() beside ms for the 2 ncol Physics.step launches it replaces (each after a record restore),
    from the states 10 env steps reach; blocks alternate (A B A B A B) and the medians are reported."""
    import torch
    from bench import csrc_sha16
    from physics_support import PIPE as pipe
    from rsr_mjx_amd.physics import Physics
    for n in [int(v) for v in args.transition_envs.split(",")]:
        write = R.row_writer(os.path.join(args.out_dir, f"transition_rates_{n}.jsonl"))
        for kind in args.families.split(","):
            b = R.batch(kind, n, steps=10, **BATCH)
            env = b.env
            phys = Physics(env)
            ncol = 2 * env.dims.nv + env.dims.nu
            saved = {k: env.view(k).clone() for k in pipe}
            ctrl = saved["ctrl"].clone()

            def restore():
                for k in pipe:
                    env.view(k).copy_(saved[k])

            def by_steps():
                for _ in range(2 * ncol):
                    restore()
                    phys.step(ctrl)
            phys.transition_fd()
            by_steps()
            fd, st = R.alternate([R.Arm(phys.transition_fd, env, args.transition_reps), R.Arm(by_steps, env)], 3, warmup=0)
            restore()
            torch.cuda.synchronize()
            write(dict(family=kind, num_envs=n, n_frames=int(env.dims.n_frames), ncol=ncol, eps=1e-3, centered=True,
                       transition_fd_ms=R.median(fd), step_launches=2 * ncol, steps_ms=R.median(st),
                       transition_fd_ms_blocks=fd, steps_ms_blocks=st, steps_over_transition_fd=R.median(st) / R.median(fd),
                       finite=bool(torch.isfinite(phys.fd_A).all() and torch.isfinite(phys.fd_B).all()), csrc_sha16=csrc_sha16()))
            del phys, env, saved, b
            torch.cuda.synchronize()


def inverse_rates(args) -> None:
    """ms per Physics.inverse() launch next to ms per constraint_forces() and per dynamics() launch of the same run, from the
    states 10 env steps reach"""
    import torch
    from bench import csrc_sha16
    from rsr_mjx_amd.physics import Physics
    for n in [int(v) for v in args.inverse_envs.split(",")]:
        write = R.row_writer(os.path.join(args.out_dir, f"inverse_rates_{n}.jsonl"))
        for kind in args.families.split(","):
            b = R.batch(kind, n, steps=10, **BATCH)
            env = b.env
            phys = Physics(env)
            phys.forward()
            qacc = phys.qacc.clone().contiguous()
            phys.set_jac_sites([])
            row = dict(family=kind, num_envs=n, launches=args.steps, warmup=args.warmup)
            row["inverse_ms"] = per_call(env, lambda i: phys.inverse(qacc), args)
            row["inverse_discrete_ms"] = per_call(env, lambda i: phys.inverse(qacc, discrete=True), args)
            row["constraint_ms"] = per_call(env, lambda i: phys.constraint_forces(), args)
            row["dynamics_ms"] = per_call(env, lambda i: phys.dynamics(), args)
            row["inverse_over_constraint"] = row["inverse_ms"] / row["constraint_ms"]
            row["inverse_over_dynamics"] = row["inverse_ms"] / row["dynamics_ms"]
            row["ordered"] = bool(row["dynamics_ms"] < row["inverse_ms"] < row["constraint_ms"])
            row["finite"] = bool(torch.isfinite(phys.qfrc_inverse).all())
            row["csrc_sha16"] = csrc_sha16()
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--families", default="cube,tshape,go2flat,go2rough,footstand")
    ap.add_argument("--applied", action="store_true")
    ap.add_argument("--dynamics", action="store_true")
    ap.add_argument("--constraint", action="store_true")
    ap.add_argument("--rollout-T", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--transition", action="store_true")
    ap.add_argument("--transition-envs", default="64,1024,8192")
    ap.add_argument("--transition-reps", type=int, default=5)
    ap.add_argument("--inverse", action="store_true")
    ap.add_argument("--inverse-envs", default="1024,8192")
    ap.add_argument("--out-dir", default=os.path.join(R.ROOT, "profiles"))
    args = ap.parse_args()
    if args.transition:
        transition_rates(args)
        return
    if args.inverse:
        inverse_rates(args)
        return
    import torch
    from bench import csrc_sha16
    from physics_support import IMPLICIT
    from rsr_mjx_amd.physics import Physics
    n = args.envs
    rows = []
    for kind in args.families.split(","):
        b = R.batch(kind, n, steps=0, **BATCH)
        envdef, env, rng = b.envdef, b.env, b.rng
        acts = [torch.as_tensor(np.clip(rng.normal(size=(n, env.dims.nu)) * b.scale, -1, 1).astype(np.float32), device=env.device)
                for _ in range(8)]
        # fused env step
        ms_env = per_call(env, lambda i: env.step(None, acts[i % 8]), args)
        # physics-only step of n_frames substeps from the states the rollout reached, under the ctrl the env step last wrote
        phys = Physics(env)
        ctrl = env.view("ctrl").clone()
        ms_phys = per_call(env, lambda i: phys.step(ctrl), args)
        row = dict(family=kind, num_envs=n, n_frames=int(env.dims.n_frames), env_step_ms=ms_env, physics_step_ms=ms_phys,
                   env_steps_per_s=n / (ms_env * 1e-3), physics_env_steps_per_s=n / (ms_phys * 1e-3),
                   physics_over_env=ms_phys / ms_env)
        if args.applied:
            T = args.rollout_T
            cr = ctrl[:, None, :].expand(n, T, env.dims.nu).contiguous()
            rollout = lambda i: phys.rollout(cr, fields=("qpos", "qvel"))
            row["rollout_step_ms"] = per_call(env, rollout, args, T)
            # small forces (2 % of each body's weight, a matching torque, 0.05 on every dof): the state stays near the plain one
            mass = torch.as_tensor(envdef.sys.arrays["body_mass"], dtype=torch.float32, device=env.device)
            g = torch.Generator(device="cpu").manual_seed(0)
            x = torch.randn((n, env.dims.nbody, 6), generator=g).to(env.device) * 0.02 * 9.81 * mass[None, :, None].clamp(min=0.05)
            q = torch.randn((n, env.dims.nv), generator=g).to(env.device) * 0.05
            phys.set_applied(x, q)
            row["applied_step_ms"] = per_call(env, lambda i: phys.step(ctrl), args)
            row["applied_rollout_step_ms"] = per_call(env, rollout, args, T)
            row["applied_over_plain_step"] = row["applied_step_ms"] / ms_phys
            row["applied_over_plain_rollout"] = row["applied_rollout_step_ms"] / row["rollout_step_ms"]
            row["rollout_T"] = T
        if args.dynamics:
            sites = ["endpoint"] if kind in IMPLICIT else ["imu", "FR", "FL", "RR", "RL"]
            row["forward_ms"] = per_call(env, lambda i: phys.forward(), args)
            phys.set_jac_sites([])
            row["dynamics_ms"] = per_call(env, lambda i: phys.dynamics(), args)
            phys.set_jac_sites(sites)
            row["dynamics_sites_ms"] = per_call(env, lambda i: phys.dynamics(), args)
            row["jac_sites"] = len(sites)
            row["dynamics_over_forward"] = row["dynamics_sites_ms"] / row["forward_ms"]
            row["csrc_sha16"] = csrc_sha16()
        if args.constraint:
            # forward and constraint_forces in alternating blocks (A B A B A B), medians of the blocks
            for _ in range(args.warmup):
                phys.forward()
                phys.constraint_forces()
            fwd, con = R.alternate([R.Arm(phys.forward, env, args.steps), R.Arm(phys.constraint_forces, env, args.steps)], 3, warmup=0)
            row["forward_ms"] = R.median(fwd)
            row["constraint_ms"] = R.median(con)
            row["forward_ms_blocks"], row["constraint_ms_blocks"] = fwd, con
            row["constraint_over_forward"] = row["constraint_ms"] / row["forward_ms"]
            row["csrc_sha16"] = csrc_sha16()
        row["finite"] = bool(torch.isfinite(env.view("qpos")).all())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del phys, env, b
        torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
