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
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _make_env(kind, n):
    """(envdef, env batch with the family's randomisation, action scale)"""
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    if kind in ("cube", "tshape"):
        envdef = airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
        dr = airbot.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(5), n)) if kind == "cube" else None
        scale = 1.0
    else:
        envdef = go2.load({"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain", "footstand": "Go2Footstand"}[kind])
        dr = go2.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(12), n))
        scale = 0.5
    return envdef, envdef.batched(n, episode_length=1000, auto_reset=True, randomization=dr), scale


def transition_rates(args) -> None:
    """ms per Physics.transition_fd() beside ms for the 2 ncol Physics.step launches it replaces (each after a record restore),
    from the states 10 env steps reach; blocks alternate (A B A B A B) and the medians are reported."""
    import torch
    from bench import csrc_sha16
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.physics import Physics
    pipe = ("qpos", "qvel", "ctrl", "qacc_warmstart", "time", "xpos", "site_xpos")
    for n in [int(v) for v in args.transition_envs.split(",")]:
        rows = []
        for kind in args.families.split(","):
            envdef, env, scale = _make_env(kind, n)
            env.reset(prng.split(prng.PRNGKey(0), n))
            rng = np.random.default_rng(0)
            for _ in range(10):
                env.step(None, np.clip(rng.normal(size=(n, env.dims.nu)) * scale, -1, 1).astype(np.float32))
            phys = Physics(env)
            ncol = 2 * env.dims.nv + env.dims.nu
            saved = {k: env.view(k).clone() for k in pipe}
            ctrl = saved["ctrl"].clone()

            def by_steps():
                for _ in range(2 * ncol):
                    for k in pipe:
                        env.view(k).copy_(saved[k])
                    phys.step(ctrl)

            def block(fn, reps):
                env.timing_begin()
                for _ in range(reps):
                    fn()
                return env.timing_end()[0] / reps
            phys.transition_fd()
            by_steps()
            fd, st = [], []
            for _ in range(3):
                fd.append(block(phys.transition_fd, args.transition_reps))
                st.append(block(by_steps, 1))
            for k in pipe:
                env.view(k).copy_(saved[k])
            torch.cuda.synchronize()
            row = dict(family=kind, num_envs=n, n_frames=int(env.dims.n_frames), ncol=ncol, eps=1e-3, centered=True,
                       transition_fd_ms=float(np.median(fd)), step_launches=2 * ncol, steps_ms=float(np.median(st)),
                       transition_fd_ms_blocks=fd, steps_ms_blocks=st, steps_over_transition_fd=float(np.median(st) / np.median(fd)),
                       finite=bool(torch.isfinite(phys.fd_A).all() and torch.isfinite(phys.fd_B).all()), csrc_sha16=csrc_sha16())
            print(json.dumps(row), flush=True)
            rows.append(row)
            del phys, env, saved
            torch.cuda.synchronize()
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"transition_rates_{n}.jsonl"), "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


def inverse_rates(args) -> None:
    """ms per Physics.inverse() launch next to ms per constraint_forces() and per dynamics() launch of the same run, from the
    states 10 env steps reach"""
    import torch
    from bench import csrc_sha16
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.physics import Physics
    for n in [int(v) for v in args.inverse_envs.split(",")]:
        rows = []
        for kind in args.families.split(","):
            envdef, env, scale = _make_env(kind, n)
            env.reset(prng.split(prng.PRNGKey(0), n))
            rng = np.random.default_rng(0)
            for _ in range(10):
                env.step(None, np.clip(rng.normal(size=(n, env.dims.nu)) * scale, -1, 1).astype(np.float32))
            phys = Physics(env)
            phys.forward()
            qacc = phys.qacc.clone().contiguous()
            phys.set_jac_sites([])

            def per_launch(fn):
                for _ in range(args.warmup):
                    fn()
                env.timing_begin()
                for _ in range(args.steps):
                    fn()
                return env.timing_end()[0] / args.steps
            row = dict(family=kind, num_envs=n, launches=args.steps, warmup=args.warmup)
            row["inverse_ms"] = per_launch(lambda: phys.inverse(qacc))
            row["inverse_discrete_ms"] = per_launch(lambda: phys.inverse(qacc, discrete=True))
            row["constraint_ms"] = per_launch(phys.constraint_forces)
            row["dynamics_ms"] = per_launch(phys.dynamics)
            row["inverse_over_constraint"] = row["inverse_ms"] / row["constraint_ms"]
            row["inverse_over_dynamics"] = row["inverse_ms"] / row["dynamics_ms"]
            row["ordered"] = bool(row["dynamics_ms"] < row["inverse_ms"] < row["constraint_ms"])
            row["finite"] = bool(torch.isfinite(phys.qfrc_inverse).all())
            row["csrc_sha16"] = csrc_sha16()
            print(json.dumps(row), flush=True)
            rows.append(row)
            del phys, env
            torch.cuda.synchronize()
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"inverse_rates_{n}.jsonl"), "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


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
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    args = ap.parse_args()
    if args.transition:
        transition_rates(args)
        return
    if args.inverse:
        inverse_rates(args)
        return
    import torch
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.physics import Physics
    n = args.envs
    rows = []
    for kind in args.families.split(","):
        if kind in ("cube", "tshape"):
            envdef = airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
            dr = airbot.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(5), n)) if kind == "cube" else None
            scale = 1.0
        else:
            envdef = go2.load({"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain", "footstand": "Go2Footstand"}[kind])
            dr = go2.domain_randomize(envdef.sys, prng.split(prng.PRNGKey(12), n))
            scale = 0.5
        env = envdef.batched(n, episode_length=1000, auto_reset=True, randomization=dr)
        env.reset(prng.split(prng.PRNGKey(0), n))
        rng = np.random.default_rng(0)
        acts = [torch.as_tensor(np.clip(rng.normal(size=(n, env.dims.nu)) * scale, -1, 1).astype(np.float32), device=env.device)
                for _ in range(8)]
        # fused env step
        for i in range(args.warmup):
            env.step(None, acts[i % 8])
        env.timing_begin()
        for i in range(args.steps):
            env.step(None, acts[i % 8])
        ms_env, launches = env.timing_end()
        ms_env /= launches
        # physics-only step of n_frames substeps from the states the rollout reached, under the ctrl the env step last wrote
        phys = Physics(env)
        ctrl = env.view("ctrl").clone()
        for _ in range(args.warmup):
            phys.step(ctrl)
        env.timing_begin()
        for _ in range(args.steps):
            phys.step(ctrl)
        ms_phys, launches = env.timing_end()
        ms_phys /= launches
        row = dict(family=kind, num_envs=n, n_frames=int(env.dims.n_frames), env_step_ms=ms_env, physics_step_ms=ms_phys,
                   env_steps_per_s=n / (ms_env * 1e-3), physics_env_steps_per_s=n / (ms_phys * 1e-3),
                   physics_over_env=ms_phys / ms_env)
        if args.applied:
            def timed(fn, per):
                for _ in range(args.warmup):
                    fn()
                env.timing_begin()
                for _ in range(args.steps):
                    fn()
                ms, launches = env.timing_end()
                return ms / launches / per
            T = args.rollout_T
            cr = ctrl[:, None, :].expand(n, T, env.dims.nu).contiguous()
            row["rollout_step_ms"] = timed(lambda: phys.rollout(cr, fields=("qpos", "qvel")), T)
            # small forces (2 % of each body's weight, a matching torque, 0.05 on every dof): the state stays near the plain one
            mass = torch.as_tensor(envdef.sys.arrays["body_mass"], dtype=torch.float32, device=env.device)
            g = torch.Generator(device="cpu").manual_seed(0)
            x = torch.randn((n, env.dims.nbody, 6), generator=g).to(env.device) * 0.02 * 9.81 * mass[None, :, None].clamp(min=0.05)
            q = torch.randn((n, env.dims.nv), generator=g).to(env.device) * 0.05
            phys.set_applied(x, q)
            row["applied_step_ms"] = timed(lambda: phys.step(ctrl), 1)
            row["applied_rollout_step_ms"] = timed(lambda: phys.rollout(cr, fields=("qpos", "qvel")), T)
            row["applied_over_plain_step"] = row["applied_step_ms"] / ms_phys
            row["applied_over_plain_rollout"] = row["applied_rollout_step_ms"] / row["rollout_step_ms"]
            row["rollout_T"] = T
        if args.dynamics:
            def per_launch(fn):                     # (forward and dynamics do not count as env launches: divide by the calls)
                for _ in range(args.warmup):
                    fn()
                env.timing_begin()
                for _ in range(args.steps):
                    fn()
                return env.timing_end()[0] / args.steps
            sites = ["endpoint"] if kind in ("cube", "tshape") else ["imu", "FR", "FL", "RR", "RL"]
            row["forward_ms"] = per_launch(phys.forward)
            phys.set_jac_sites([])
            row["dynamics_ms"] = per_launch(phys.dynamics)
            phys.set_jac_sites(sites)
            row["dynamics_sites_ms"] = per_launch(phys.dynamics)
            row["jac_sites"] = len(sites)
            row["dynamics_over_forward"] = row["dynamics_sites_ms"] / row["forward_ms"]
            from bench import csrc_sha16
            row["csrc_sha16"] = csrc_sha16()
        if args.constraint:
            # forward and constraint_forces in alternating blocks (A B A B A B), medians of the blocks: a drift of the clocks
            # over the run falls on both
            def block(fn):
                env.timing_begin()
                for _ in range(args.steps):
                    fn()
                return env.timing_end()[0] / args.steps
            for _ in range(args.warmup):
                phys.forward()
                phys.constraint_forces()
            fwd, con = [], []
            for _ in range(3):
                fwd.append(block(phys.forward))
                con.append(block(phys.constraint_forces))
            row["forward_ms"] = float(np.median(fwd))
            row["constraint_ms"] = float(np.median(con))
            row["forward_ms_blocks"], row["constraint_ms_blocks"] = fwd, con
            row["constraint_over_forward"] = row["constraint_ms"] / row["forward_ms"]
            from bench import csrc_sha16
            row["csrc_sha16"] = csrc_sha16()
        row["finite"] = bool(torch.isfinite(env.view("qpos")).all())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del phys, env
        torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
