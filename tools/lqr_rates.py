"""The LQR backward pass (rsr_physics_lqr_backward) against the loop a user writes without it.  Per model family (the handle gives
nv and nu; nothing of the env is read), on M seeded problems of T steps (tests/lqr_ref.py's inputs, columns packed tight): arm A is
Physics.lqr_backward, one launch; arm B is the same recursion as a batched torch loop over t on the same device tensors (A_t, B_t
as the transposed views trajectory_fd returns, torch.linalg.cholesky_ex and cholesky_solve, no host sync inside), which is what a
user of the parent commit runs.  Both are timed with HIP events on the launch stream (rsr_timing_begin / _end) around `inner` calls
of arm A and one pass of arm B, one warm-up round then `reps` rounds alternating the arms in one process; times are per call.  The
arms' gains are compared (relative to the largest entry: they sum in different orders).  One JSON line per (family, M).
Usage: python tools/lqr_rates.py [--sizes 64,1024] [--T 50] [--reps 7] [--inner 20] [--families cube,go2flat,tshape] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_backward(col, lx, lu, lxx, luu, lux, mu, nx):
    """the recursion of include/rsr_physics.h (flags = 0) as a batched torch loop; returns gain [M, T, nu, nx], k [M, T, nu], dV [M, 2]"""
    import torch
    M, T = col.shape[0], col.shape[1]
    nu = col.shape[2] - nx
    A, B = col[:, :, :nx, :nx].transpose(2, 3), col[:, :, nx:, :nx].transpose(2, 3)
    eye = torch.eye(nu, device=col.device)
    gain, k = torch.empty((M, T, nu, nx), device=col.device), torch.empty((M, T, nu), device=col.device)
    dV = torch.zeros((M, 2), device=col.device)
    Vx, Vxx = lx[:, T], lxx[:, T]
    for t in range(T - 1, -1, -1):
        a, b = A[:, t], B[:, t]
        at, bt = a.transpose(1, 2), b.transpose(1, 2)
        Qx = lx[:, t] + (at @ Vx[:, :, None])[:, :, 0]
        Qu = lu[:, t] + (bt @ Vx[:, :, None])[:, :, 0]
        W = Vxx @ a
        Qxx, Qux, Quu = lxx[:, t] + at @ W, lux[:, t] + bt @ W, luu[:, t] + bt @ (Vxx @ b)
        L = torch.linalg.cholesky_ex(Quu + mu[:, None, None] * eye).L
        sol = -torch.cholesky_solve(torch.cat([Qu[:, :, None], Qux], dim=2), L)
        kt, Kt = sol[:, :, 0], sol[:, :, 1:]
        Ktt = Kt.transpose(1, 2)
        Vx = Qx + (Ktt @ (Quu @ kt[:, :, None] + Qu[:, :, None]))[:, :, 0] + (Qux.transpose(1, 2) @ kt[:, :, None])[:, :, 0]
        Vxx = Qxx + Ktt @ (Quu @ Kt + Qux) + Qux.transpose(1, 2) @ Kt
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
        dV[:, 0] += (kt * Qu).sum(1)
        dV[:, 1] += 0.5 * (kt * (Quu @ kt[:, :, None])[:, :, 0]).sum(1)
        gain[:, t], k[:, t] = Kt, kt
    return gain, k, dV


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024", help="M: independent problems")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls of arm A per timed window")
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--families", default="cube,go2flat,tshape")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M)")
    args = ap.parse_args()
    import torch
    import bench
    import lqr_ref
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import airbot, go2
    from rsr_mjx_amd.physics import Physics
    T = args.T
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()
    for m in (int(v) for v in args.sizes.split(",")):
        for kind in args.families.split(","):
            if kind in ("cube", "tshape"):
                envdef = airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
            else:
                envdef = go2.load({"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain", "footstand": "Go2Footstand"}[kind])
            env = envdef.batched(4)
            env.reset(prng.split(prng.PRNGKey(0), 4))
            phys = Physics(env)
            nx, nu = 2 * int(env.dims.nv), int(env.dims.nu)
            inp = lqr_ref.inputs(m, T, nx, nu, seed=0)
            dev = lambda a: torch.as_tensor(a, device=env.device)
            col = dev(lqr_ref.pack(inp["A"], inp["B"]))
            lx, lu, lxx, luu, lux = (dev(inp[k]) for k in ("lx", "lu", "lxx", "luu", "lux"))
            mu = torch.full((m,), args.mu, device=env.device)
            out = dict(gain=torch.empty((m, T, nu, nx), device=env.device), k=torch.empty((m, T, nu), device=env.device),
                       dV=torch.empty((m, 2), device=env.device), status=torch.empty((m,), device=env.device))
            torch.cuda.synchronize()
            t_a, t_b = [], []
            for r in range(args.reps + 1):                        # (the first round warms both arms up)
                env.timing_begin()
                for _ in range(args.inner):
                    phys.lqr_backward(col, lx, lu, lxx, luu, lux=lux, mu=mu, out=out)
                ms, _ = env.timing_end()
                if r: t_a.append(ms / args.inner)
                torch.cuda.synchronize()
                env.timing_begin()
                g_b, k_b, dv_b = torch_backward(col, lx, lu, lxx, luu, lux, mu, nx)
                ms, _ = env.timing_end()
                if r: t_b.append(ms)
                torch.cuda.synchronize()
            med = lambda x: float(np.median(x))
            scale = float(g_b.abs().max())
            row = dict(family=kind, M=m, T=T, nx=nx, nu=nu, mu=args.mu, csrc_sha16=bench.csrc_sha16(),
                       lqr_backward_ms=med(t_a), torch_loop_ms=med(t_b), torch_loop_over_lqr_backward=med(t_b) / med(t_a),
                       problems_per_s=m / (med(t_a) * 1e-3), steps_per_s=m * T / (med(t_a) * 1e-3),
                       spread=[min(t_a), max(t_a), min(t_b), max(t_b)], reps=args.reps, inner=args.inner,
                       gain_max_rel_diff=float((out["gain"] - g_b).abs().max()) / scale,
                       k_max_abs_diff=float((out["k"] - k_b).abs().max()), dV_max_rel_diff=float(((out["dV"] - dv_b).abs() / dv_b.abs().clamp(min=1)).max()),
                       all_succeeded=bool((out["status"] == -1).all()), finite=bool(torch.isfinite(out["gain"]).all()))
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del phys, env
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
