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

import rates_support as R


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
    from rsr_mjx_amd.physics import Physics
    T, write = args.T, R.row_writer(args.out)
    for m in (int(v) for v in args.sizes.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, 4, steps=0, dr=False)
            env = b.env
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
            loop = {}

            def torch_arm():
                loop["gain"], loop["k"], loop["dV"] = torch_backward(col, lx, lu, lxx, luu, lux, mu, nx)
            t_a, t_b = R.alternate([R.Arm(lambda: phys.lqr_backward(col, lx, lu, lxx, luu, lux=lux, mu=mu, out=out), env, args.inner),
                                    R.Arm(torch_arm, env)], args.reps)
            med = R.median
            g_b, k_b, dv_b = loop["gain"], loop["k"], loop["dV"]
            scale = float(g_b.abs().max())
            row = dict(family=kind, M=m, T=T, nx=nx, nu=nu, mu=args.mu, csrc_sha16=bench.csrc_sha16(),
                       lqr_backward_ms=med(t_a), torch_loop_ms=med(t_b), torch_loop_over_lqr_backward=med(t_b) / med(t_a),
                       problems_per_s=m / (med(t_a) * 1e-3), steps_per_s=m * T / (med(t_a) * 1e-3),
                       spread=R.spread(t_a, t_b), reps=args.reps, inner=args.inner,
                       gain_max_rel_diff=float((out["gain"] - g_b).abs().max()) / scale,
                       k_max_abs_diff=float((out["k"] - k_b).abs().max()), dV_max_rel_diff=float(((out["dV"] - dv_b).abs() / dv_b.abs().clamp(min=1)).max()),
                       all_succeeded=bool((out["status"] == -1).all()), finite=bool(torch.isfinite(out["gain"]).all()))
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
