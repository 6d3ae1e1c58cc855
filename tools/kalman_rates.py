"""The Kalman filter and RTS smoother (rsr_physics_kalman) against the loops a user writes without it.  Per model family (the handle
gives nv and nu; nothing of the env is read), on M seeded problems of T steps and ny sensor entries (tests/kalman_ref.py's inputs,
columns packed tight): arm A is Physics.kalman_smooth, one launch, filter only and with the smoother; arm B is the same recursion as
a batched torch loop over t on the same device tensors (A_t, C_t as the transposed views trajectory_fd returns, the measurement
update one sensor entry at a time, torch.linalg.cholesky_ex and cholesky_solve in the smoother, no host sync inside); arm C is the
batch form of the update a user may write instead (S = C P C^T + R factorised once per step: equal in exact arithmetic).  All are
timed with HIP events on the launch stream (rsr_timing_begin / _end) around `inner` calls of arm A and one pass of arm B or C, one
warm-up round then `reps` rounds alternating the arms in one process; times are per call.  The arms' results are compared (relative
to the largest entry: they sum in different orders).  One JSON line per (family, M, smooth).
Usage: python tools/kalman_rates.py [--sizes 64,1024] [--T 50] [--ny 55] [--reps 5] [--inner 10] [--families cube,go2flat,tshape] [--out FILE]"""
from __future__ import annotations

import argparse

import rates_support as R


def torch_kalman(col, dy, r, q, x0, P0, nx, smooth, batch_update):
    """the recursion of include/rsr_physics.h as a batched torch loop (batch_update: the update of a step in one piece); returns
    xf [M, T+1, nx], xs or None, nll [M]"""
    import math
    import torch
    M, T = col.shape[0], col.shape[1]
    ny = col.shape[3] - nx
    A, Cm = col[:, :, :nx, :nx].transpose(2, 3), col[:, :, :nx, nx:].transpose(2, 3)
    dev = col.device
    xf, Pf = torch.empty((M, T + 1, nx), device=dev), torch.empty((M, T + 1, nx, nx), device=dev)
    nll = torch.zeros((M,), device=dev)
    log2pi = math.log(2.0 * math.pi)
    x, P = x0, P0

    def predict(a, p, qt):
        s = a @ p @ a.transpose(1, 2)
        return 0.5 * (s + s.transpose(1, 2)) + torch.diag_embed(qt)

    for t in range(T):
        c = Cm[:, t]
        if batch_update:
            pc = P @ c.transpose(1, 2)
            L = torch.linalg.cholesky_ex(c @ pc + torch.diag_embed(r[:, t])).L
            nu = dy[:, t] - (c @ x[:, :, None])[:, :, 0]
            k = torch.cholesky_solve(pc.transpose(1, 2), L).transpose(1, 2)
            x = x + (k @ nu[:, :, None])[:, :, 0]
            P = P - k @ pc.transpose(1, 2)
            z = torch.linalg.solve_triangular(L, nu[:, :, None], upper=False)[:, :, 0]
            nll = nll + 0.5 * ((z * z).sum(1) + 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1) + ny * log2pi)
        else:
            for j in range(ny):
                cj = c[:, j]
                w = (P @ cj[:, :, None])[:, :, 0]
                s = (cj * w).sum(1) + r[:, t, j]
                nu = dy[:, t, j] - (cj * x).sum(1)
                g = nu / s
                x = x + w * g[:, None]
                P = P - (w[:, :, None] * w[:, None, :]) / s[:, None, None]
                nll = nll + 0.5 * (nu * g + torch.log(s) + log2pi)
        xf[:, t], Pf[:, t] = x, P
        x = (A[:, t] @ x[:, :, None])[:, :, 0]
        P = predict(A[:, t], P, q[:, t])
    xf[:, T], Pf[:, T] = x, P
    if not smooth:
        return xf, None, nll
    xs = torch.empty_like(xf)
    xs[:, T] = x
    Ps = P
    for t in range(T - 1, -1, -1):
        a, pf = A[:, t], Pf[:, t]
        Pm = predict(a, pf, q[:, t])
        L = torch.linalg.cholesky_ex(Pm).L
        G = torch.cholesky_solve(a @ pf, L).transpose(1, 2)
        xs[:, t] = xf[:, t] + (G @ (xs[:, t + 1] - (a @ xf[:, t, :, None])[:, :, 0])[:, :, None])[:, :, 0]
        E = G @ (Ps - Pm) @ G.transpose(1, 2)
        Ps = pf + 0.5 * (E + E.transpose(1, 2))
    return xf, xs, nll


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024", help="M: independent problems")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--ny", type=int, default=55, help="sensor entries (55: the Go2 joystick env's table)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls of arm A per timed window")
    ap.add_argument("--families", default="cube,go2flat,tshape")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M, smooth)")
    args = ap.parse_args()
    import torch
    import bench
    import kalman_ref
    from rsr_mjx_amd.physics import Physics
    T, ny, write = args.T, args.ny, R.row_writer(args.out)
    for m in (int(v) for v in args.sizes.split(",")):
        for kind in args.families.split(","):
            b = R.batch(kind, 4, steps=0, dr=False)
            env = b.env
            phys = Physics(env)
            nx, nu = 2 * int(env.dims.nv), int(env.dims.nu)
            inp = kalman_ref.inputs(m, T, nx, ny, seed=0)
            dev = lambda a: torch.as_tensor(a, device=env.device)
            col = dev(kalman_ref.pack(inp["A"], inp["C"], nu))
            dy, r, q, x0, P0 = (dev(inp[k]) for k in ("dy", "r", "q", "x0", "P0"))
            for smooth in (False, True):
                shapes = dict(xf=(m, T + 1, nx), Pf=(m, T + 1, nx, nx), nll=(m,), status=(m, 2), **({"xs": (m, T + 1, nx)} if smooth else {}))
                out = {k: torch.empty(s, device=env.device) for k, s in shapes.items()}
                torch.cuda.synchronize()
                loop = {}

                def torch_arm(batch_update):
                    loop[batch_update] = torch_kalman(col, dy, r, q, x0, P0, nx, smooth, batch_update)
                t_a, t_b, t_c = R.alternate([R.Arm(lambda: phys.kalman_smooth(col, dy, r, q, P0, x0=x0, smooth=smooth, out=out), env, args.inner),
                                             R.Arm(lambda: torch_arm(False), env), R.Arm(lambda: torch_arm(True), env)], args.reps)
                med = R.median
                name = "xs" if smooth else "xf"
                diffs = {}
                for tag, key in (("sequential", False), ("batch", True)):
                    xf_b, xs_b, nll_b = loop[key]
                    ref = xs_b if smooth else xf_b
                    diffs[f"{name}_max_rel_diff_{tag}"] = float((out[name] - ref).abs().max()) / float(ref.abs().max())
                    diffs[f"nll_max_rel_diff_{tag}"] = float(((out["nll"] - nll_b).abs() / nll_b.abs().clamp(min=1)).max())
                row = dict(family=kind, M=m, T=T, nx=nx, ny=ny, smooth=smooth, csrc_sha16=bench.csrc_sha16(),
                           kalman_smooth_ms=med(t_a), torch_loop_ms=med(t_b), torch_batch_update_ms=med(t_c),
                           torch_loop_over_kalman_smooth=med(t_b) / med(t_a), torch_batch_update_over_kalman_smooth=med(t_c) / med(t_a),
                           problems_per_s=m / (med(t_a) * 1e-3), steps_per_s=m * T / (med(t_a) * 1e-3),
                           spread=R.spread(t_a, t_b, t_c), reps=args.reps, inner=args.inner, **diffs,
                           all_succeeded=bool((out["status"] == -1).all()), finite=bool(torch.isfinite(out[name]).all()))
                write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
