"""Inverse kinematics on site pose targets (rsr_physics_ik) against the loop a user writes without it.  Per model family, on a
batch of M envs with one problem per env (tests/ik_ref.py's reachable cases, position targets only, a hinge-and-slide dof mask so that
the loop's integrate is an add): arm A is Physics.ik, one launch, iters iterations with both tolerances 0; arm B is the same
iteration on the parent's API, per iteration set_state (a whole mjx.forward), dynamics() for jacp and jac_site_xpos,
torch.linalg.solve of J^T J + lambda I, the step cap, the add and the clamp in torch, no host sync inside.  Both are timed with HIP
events on the launch stream (rsr_timing_begin / _end) around `inner` calls of arm A and one pass of arm B, one warm-up round then
`reps` rounds alternating the arms in one process; times are per call.  The arms' final qpos are compared.  One JSON line per
(family, M).
Usage: python tools/ik_rates.py [--sizes 64,1024] [--iters 20] [--reps 7] [--inner 20] [--families cube,go2flat] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TASKS = {"cube": ["endpoint"], "tshape": ["endpoint"], "go2flat": ["FR", "FL", "RR", "RL"]}


def torch_loop(phys, start, target, mask, qadr, dadr, lo, hi, lam, iters, max_step):
    """arm B; set_jac_sites was called.  Returns the final qpos [M, nq]"""
    import torch
    M, nv = start.shape[0], mask.shape[0]
    q = start.clone()
    eye = lam * torch.eye(nv, device=start.device)
    for _ in range(iters):
        phys.set_state(qpos=q)
        phys.dynamics()
        b = (target - phys.jac_site_xpos).reshape(M, -1, 1)
        J = phys.jacp.reshape(M, -1, nv) * mask
        Jt = J.transpose(1, 2)
        dq = torch.linalg.solve(Jt @ J + eye, Jt @ b)[:, :, 0]
        mx = dq.abs().amax(1, keepdim=True)
        dq = dq * torch.where(mx > max_step, max_step / mx, torch.ones_like(mx))
        q[:, qadr] = torch.minimum(torch.maximum(q[:, qadr] + dq[:, dadr], lo), hi)
    return q


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024", help="M: problems, one per env")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls of arm A per timed window")
    ap.add_argument("--damping", type=float, default=1e-3)
    ap.add_argument("--max-step", type=float, default=0.3)
    ap.add_argument("--families", default="cube,go2flat")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M)")
    args = ap.parse_args()
    import torch
    import bench
    import ik_ref
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.physics import Physics
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()
    for m in (int(v) for v in args.sizes.split(",")):
        for kind in args.families.split(","):
            if kind in ("cube", "tshape"):
                envdef = airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
            else:
                envdef = go2.load({"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain", "footstand": "Go2Footstand"}[kind])
            env = envdef.batched(m)
            env.reset(prng.split(prng.PRNGKey(0), m))
            phys = Physics(env)
            A = envdef.sys.arrays
            sites = [int(envdef.sys.id("site", n)) for n in TASKS[kind]]
            c = ik_ref.cases(A, sites, m, 0, 0.2, with_quat=False)
            dev = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), dtype=dt, device=env.device)
            start, target = dev(c["start"]), dev(c["target_pos"])
            js = [j for j in range(len(A["jnt_type"])) if int(A["jnt_type"][j]) in (2, 3)]
            assert all(int(A["jnt_limited"][j]) for j in js)
            qadr, dadr = dev([A["jnt_qposadr"][j] for j in js], torch.int64), dev([A["jnt_dofadr"][j] for j in js], torch.int64)
            lo, hi = dev([A["jnt_range"][j][0] for j in js]), dev([A["jnt_range"][j][1] for j in js])
            mask = torch.zeros(int(env.dims.nv), device=env.device)
            mask[dadr] = 1.0
            phys.set_jac_sites(sites)
            lam = torch.full((m,), args.damping, device=env.device)
            out = dict(qpos=torch.empty((m, int(env.dims.nq)), device=env.device), err=torch.empty((m, 2), device=env.device),
                       info=torch.empty((m, 2), dtype=torch.int32, device=env.device))
            kw = dict(sites=sites, target_pos=target, dofs=dadr.tolist(), qpos0=start, damping=lam, iters=args.iters, tol_pos=0.0, tol_rot=0.0,
                      max_step=args.max_step, limits=True, out=out)
            torch.cuda.synchronize()
            t_a, t_b = [], []
            for r in range(args.reps + 1):                        # (the first round warms both arms up)
                env.timing_begin()
                for _ in range(args.inner):
                    phys.ik(**kw)
                ms, _ = env.timing_end()
                if r: t_a.append(ms / args.inner)
                torch.cuda.synchronize()
                env.timing_begin()
                q_b = torch_loop(phys, start, target, mask, qadr, dadr, lo, hi, args.damping, args.iters, args.max_step)
                ms, _ = env.timing_end()
                if r: t_b.append(ms)
                torch.cuda.synchronize()
            med = lambda x: float(np.median(x))
            row = dict(family=kind, M=m, iters=args.iters, nsite=len(sites), ndof=len(js), damping=args.damping, max_step=args.max_step,
                       csrc_sha16=bench.csrc_sha16(), ik_ms=med(t_a), torch_loop_ms=med(t_b), torch_loop_over_ik=med(t_b) / med(t_a),
                       problems_per_s=m / (med(t_a) * 1e-3), iterations_per_s=m * args.iters / (med(t_a) * 1e-3),
                       spread=[min(t_a), max(t_a), min(t_b), max(t_b)], reps=args.reps, inner=args.inner,
                       qpos_max_abs_diff=float((out["qpos"][:, qadr] - q_b[:, qadr]).abs().max()),
                       perr_max=float(out["err"][:, 0].max()), perr_median=float(out["err"][:, 0].median()),
                       ran_all_iterations=float((out["info"][:, 0] == args.iters).float().mean()), finite=bool(torch.isfinite(out["qpos"]).all()))
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del phys, env
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
