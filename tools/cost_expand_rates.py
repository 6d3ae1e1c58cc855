"""The cost expansion (rsr_physics_cost_expand) against the same expansion written as batched torch einsums on the device.  Per model
family (the handle gives nv and nu; nothing of the env is read), on M seeded problems of T steps with every term of the cost on and
ny the width of the family's full sensor table (tests/physics_support.sensor_spec), and with the sensor term off: arm A is
Physics.cost_expand into caller-owned outputs, one launch; arm B the torch form (the products C^T W C, D^T W C, D^T W D and the
gradients as einsums over the sensor slice of the columns, diag_embed for the state and ctrl parts), as a user without the call
would write it.  Both are timed with HIP events on the launch stream around `inner` calls, one warm-up round then `reps` rounds
alternating the arms in one process; times are per call.  The row also gives the bytes the call has to move (the five outputs written,
the sensor slice of the columns and the cost and residual rows read) over arm A's time, and the largest relative difference between
the two arms' outputs, and physics_sha16, a hash of csrc/physics/ and include/rsr_physics.h (the kernel that was timed; csrc_sha16
covers the env kernels only).  One JSON line per (family, M, sensor on / off); `--out` may hold {M}: one file per size.
Usage: python tools/cost_expand_rates.py [--sizes 64,1024] [--T 50] [--reps 7] [--inner 20] [--families cube,go2flat,tshape] [--out FILE]"""
from __future__ import annotations

import argparse

import rates_support as R


def physics_sha16() -> str:
    """SHA-256 (first 16 hex digits) of the sources the timed kernel is built from, which bench.csrc_sha16() does not cover:
    rsr_mjx_amd/csrc/physics/*.hip, *.hpp and include/rsr_physics.h, in name order"""
    import hashlib
    import os
    h = hashlib.sha256()
    d = os.path.join(R.ROOT, "rsr_mjx_amd", "csrc", "physics")
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hip", ".hpp")))
    for f in files + [os.path.join(R.ROOT, "include", "rsr_physics.h")]:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def torch_expand(c, src, col, nv, sensor):
    """the expansion in batched torch ops: {lx, lu, lxx, luu, lux}"""
    import torch
    nx = 2 * nv
    M, T, nu = c["w_ctrl"].shape
    w = torch.cat([c["w_qpos"], c["w_qvel"]], -1)
    lx, lxx = w.new_zeros(M, T + 1, nx), w.new_zeros(M, T + 1, nx, nx)
    lx[:, 1:] = w * src["dx"]
    lxx[:, 1:] = torch.diag_embed(w)
    lu, luu = c["w_ctrl"] * (src["ctrl"] - c["ctrl_ref"]), torch.diag_embed(c["w_ctrl"])
    if not sensor:
        return dict(lx=lx, lu=lu, lxx=lxx, luu=luu, lux=w.new_zeros(M, T, nu, nx))
    ws = c["w_sensor"]
    cd = col[..., nx:nx + ws.shape[2]]                               # [M, T, ncol, ny]
    cm, dm = cd[:, :, :nx], cd[:, :, nx:]
    g = ws * (src["sensordata"] - c["sensor_ref"])
    wc, wd = cm * ws[:, :, None, :], dm * ws[:, :, None, :]
    lx[:, :T] += torch.einsum("mtaj,mtj->mta", cm, g)
    lu = lu + torch.einsum("mtpj,mtj->mtp", dm, g)
    lxx[:, :T] += torch.einsum("mtaj,mtbj->mtab", wc, cm)
    luu = luu + torch.einsum("mtpj,mtqj->mtpq", wd, dm)
    return dict(lx=lx, lu=lu, lxx=lxx, luu=luu, lux=torch.einsum("mtpj,mtaj->mtpa", wd, cm))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024", help="M: independent problems")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls of an arm per timed window")
    ap.add_argument("--families", default="cube,go2flat,tshape")
    ap.add_argument("--out", default=None, help="JSON lines, one per (family, M, sensor); {M} in the name: one file per size")
    args = ap.parse_args()
    import torch
    import bench
    import physics_support as S
    from rsr_mjx_amd.physics import Physics
    T = args.T
    for m in (int(v) for v in args.sizes.split(",")):
        write = R.row_writer(args.out.format(M=m) if args.out else None)
        for kind in args.families.split(","):
            b = R.batch(kind, 4, steps=0, dr=False)
            env = b.env
            phys = Physics(env, sensors=S.sensor_spec(kind, b.envdef))
            nv, nu, ny = int(env.dims.nv), int(env.dims.nu), phys.nsensordata
            nx, ncol = 2 * nv, 2 * nv + nu
            gen = torch.Generator(device=env.device).manual_seed(0)
            uni = lambda *s: 2.0 * torch.rand(s, device=env.device, generator=gen)
            nrm = lambda scale, *s: scale * torch.randn(s, device=env.device, generator=gen)
            cost = dict(w_qpos=uni(m, T, nv), w_qvel=uni(m, T, nv), w_ctrl=uni(m, T, nu), w_sensor=uni(m, T, ny),
                        ctrl_ref=nrm(0.1, m, T, nu), sensor_ref=nrm(0.1, m, T, ny))
            src = dict(dx=nrm(0.1, m, T, nx), ctrl=nrm(0.1, m, T, nu), sensordata=nrm(0.1, m, T, ny))
            col = nrm(1.0, m, T, ncol, nx + ny)
            new = lambda *s: torch.empty(s, device=env.device)
            out = dict(lx=new(m, T + 1, nx), lu=new(m, T, nu), lxx=new(m, T + 1, nx, nx), luu=new(m, T, nu, nu), lux=new(m, T, nu, nx))
            torch.cuda.synchronize()
            for sensor in (True, False):
                c = cost if sensor else {k: v for k, v in cost.items() if "sensor" not in k}
                kw = dict(src, columns=col) if sensor else dict(dx=src["dx"], ctrl=src["ctrl"])
                call_arm = lambda: phys.cost_expand(c, out=out, **kw)
                torch_arm = lambda: torch_expand(cost, src, col, nv, sensor)
                t_a, t_b = R.alternate([R.Arm(call_arm, env, args.inner), R.Arm(torch_arm, env, args.inner)], args.reps)
                got, ref = call_arm(), torch_arm()
                torch.cuda.synchronize()
                diff = max(float(((got[k] - ref[k]).abs().amax() / ref[k].abs().amax().clamp_min(1.0))) for k in out)
                floats = sum(t.numel() for t in out.values()) + m * T * (2 * nx + 3 * nu) + (m * T * (ncol * ny + 3 * ny) if sensor else 0)
                med = R.median
                write(dict(family=kind, M=m, T=T, nx=nx, nu=nu, ny=ny if sensor else 0, w_sensor=sensor, csrc_sha16=bench.csrc_sha16(), physics_sha16=physics_sha16(),
                           cost_expand_ms=med(t_a), torch_einsum_ms=med(t_b), torch_over_call=med(t_b) / med(t_a),
                           problems_per_s=m / (med(t_a) * 1e-3), steps_per_s=m * (T + 1) / (med(t_a) * 1e-3),
                           bytes_moved=4 * floats, gb_per_s=4 * floats / (med(t_a) * 1e-3) / 1e9,
                           spread=R.spread(t_a, t_b), reps=args.reps, inner=args.inner, max_rel_diff=diff,
                           finite=bool(all(torch.isfinite(t).all() for t in got.values()))))
            del phys, env, b, col
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
