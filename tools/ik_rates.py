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

import numpy as np

import rates_support as R

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
    from rsr_mjx_amd.physics import Physics
    write = R.row_writer(args.out)
    for m in (int(v) for v in args.sizes.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, m, steps=0, dr=False)
            envdef, env = b.envdef, b.env
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
            loop = {}

            def torch_arm():
                loop["q"] = torch_loop(phys, start, target, mask, qadr, dadr, lo, hi, args.damping, args.iters, args.max_step)
            t_a, t_b = R.alternate([R.Arm(lambda: phys.ik(**kw), env, args.inner), R.Arm(torch_arm, env)], args.reps)
            med, q_b = R.median, loop["q"]
            row = dict(family=kind, M=m, iters=args.iters, nsite=len(sites), ndof=len(js), damping=args.damping, max_step=args.max_step,
                       csrc_sha16=bench.csrc_sha16(), ik_ms=med(t_a), torch_loop_ms=med(t_b), torch_loop_over_ik=med(t_b) / med(t_a),
                       problems_per_s=m / (med(t_a) * 1e-3), iterations_per_s=m * args.iters / (med(t_a) * 1e-3),
                       spread=R.spread(t_a, t_b), reps=args.reps, inner=args.inner,
                       qpos_max_abs_diff=float((out["qpos"][:, qadr] - q_b[:, qadr]).abs().max()),
                       perr_max=float(out["err"][:, 0].max()), perr_median=float(out["err"][:, 0].median()),
                       ran_all_iterations=float((out["info"][:, 0] == args.iters).float().mean()), finite=bool(torch.isfinite(out["qpos"]).all()))
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
