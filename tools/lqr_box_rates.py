"""The control-limited backward pass (rsr_physics_lqr_box) against the plain one (rsr_physics_lqr_backward): what the QP inside the
recursion costs.  Per model family (the handle gives nv and nu; nothing of the env is read), on M seeded problems of T steps
(tests/lqr_ref.py's inputs, columns packed tight) with the bounds of tests/lqr_box_ref.py (a seventh of the controls unbounded, a
twentieth with zero infeasible): arm A is Physics.lqr_backward_box, arm B Physics.lqr_backward on the same inputs, one launch each.
Both are timed with HIP events on the launch stream around `inner` calls, one warm-up round then `reps` rounds alternating the arms
in one process; times are per call.  The row also says what the QPs did: the share of clamped controls, the Newton steps per step
and the codes.  One JSON line per (family, M).
Usage: python tools/lqr_box_rates.py [--sizes 64,1024] [--T 50] [--reps 7] [--inner 20] [--families cube,go2flat,tshape] [--out FILE]"""
from __future__ import annotations

import argparse

import rates_support as R


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024", help="M: independent problems")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls of an arm per timed window")
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--max-iter", type=int, default=32)
    ap.add_argument("--families", default="cube,go2flat,tshape")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M)")
    args = ap.parse_args()
    import torch
    import bench
    import lqr_box_ref
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
            lo, hi = (dev(a) for a in lqr_box_ref.bounds(m, T, nu, 700))
            mu = torch.full((m,), args.mu, device=env.device)
            new = lambda *s: torch.empty(s, device=env.device)
            out_a = dict(gain=new(m, T, nu, nx), k=new(m, T, nu), dV=new(m, 2), status=new(m), clamped=new(m, T, nu), qp=new(m, T, 2))
            out_b = dict(gain=new(m, T, nu, nx), k=new(m, T, nu), dV=new(m, 2), status=new(m))
            torch.cuda.synchronize()
            box_arm = lambda: phys.lqr_backward_box(col, lx, lu, lxx, luu, lo, hi, lux=lux, mu=mu, max_iter=args.max_iter, report=True, out=out_a)
            plain_arm = lambda: phys.lqr_backward(col, lx, lu, lxx, luu, lux=lux, mu=mu, out=out_b)
            t_a, t_b = R.alternate([R.Arm(box_arm, env, args.inner), R.Arm(plain_arm, env, args.inner)], args.reps)
            med = R.median
            qp = out_a["qp"]
            row = dict(family=kind, M=m, T=T, nx=nx, nu=nu, mu=args.mu, max_iter=args.max_iter, csrc_sha16=bench.csrc_sha16(),
                       lqr_backward_box_ms=med(t_a), lqr_backward_ms=med(t_b), box_over_plain=med(t_a) / med(t_b),
                       problems_per_s=m / (med(t_a) * 1e-3), steps_per_s=m * T / (med(t_a) * 1e-3),
                       spread=R.spread(t_a, t_b), reps=args.reps, inner=args.inner,
                       clamped_share=float((out_a["clamped"] != 0).float().mean()), newton_steps_mean=float(qp[..., 0].mean()),
                       newton_steps_max=int(qp[..., 0].max()), codes={str(c): int((qp[..., 1] == c).sum()) for c in range(4)},
                       all_succeeded=bool((out_a["status"] == -1).all() and (out_b["status"] == -1).all()),
                       finite=bool(torch.isfinite(out_a["gain"]).all()))
            write(row)
            del phys, env, b
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
