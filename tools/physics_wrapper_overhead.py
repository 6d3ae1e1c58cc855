"""Host-side cost of rsr_mjx_amd/physics.py per call, in microseconds, without a device: the methods run on the handle-less Physics
of tests/api_support.py against its recording library, so what is timed is the wrapper's own Python (checks, output tensors, ctypes
structs) and nothing of the library.  Inputs are the smallest that pass the checks: num_envs = 4, K = 2, T = 3.

    python tools/physics_wrapper_overhead.py [--module PATH] [--label NAME] [--repeats 7] [--calls 2000]

--module: a physics.py to time in the package's place (another revision's, for an A/B; run the two alternately).  One JSON line
per method: the median over the repeats of the mean time per call, with the repeats' min and max (one more repeat runs first and is
dropped)."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--module", default=None)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be >= 5")
    import torch
    import rsr_mjx_amd
    from rsr_mjx_amd import _lib
    if a.module:
        spec = importlib.util.spec_from_file_location("rsr_mjx_amd.physics", a.module)
        mod = sys.modules["rsr_mjx_amd.physics"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        rsr_mjx_amd.physics = mod
    import api_support
    rec = api_support.Recorder()
    _lib.lib = lambda: rec
    p = api_support.standin()
    p.__dict__.setdefault("_ids_in", {})              # (a revision from before the held inputs were one dict)
    d = p.dims
    M, K, T, nu, nq, nv = p.num_envs, 2, 3, d.nu, d.nq, d.nv
    nx = 2 * nv
    z = lambda *s: torch.zeros(s)
    ctrl, c3, c4 = z(M, nu), z(M, T, nu), z(M, K, T, nu)
    gain, qref, vref = z(M, T, nu, nx), z(M, T, nq), z(M, T, nv)
    col, lx, lu, lxx, luu = z(M, T, nx + nu, nx), z(M, T + 1, nx), z(M, T, nu), z(M, T + 1, nx, nx), z(M, T, nu, nu)
    tpos = z(M, 1, 3)
    methods = dict(step=lambda: p.step(ctrl), sample_rollouts=lambda: p.sample_rollouts(c4),
                   feedback_rollouts=lambda: p.feedback_rollouts(c4, gain, qref, vref), trajectory_fd=lambda: p.trajectory_fd(c3),
                   lqr_backward=lambda: p.lqr_backward(col, lx, lu, lxx, luu), ik=lambda: p.ik(["tip"], tpos))
    for name, call in methods.items():
        call()
        assert len(rec.calls) == 1, (name, rec.calls)                                  # it got as far as the library
        us = []
        for _ in range(a.repeats + 1):
            rec.calls.clear()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            us.append((time.perf_counter() - t0) / a.calls * 1e6)
        us = us[1:]                                                                    # (the first repeat warms up)
        rec.calls.clear()
        print(json.dumps(dict(tool="physics_wrapper_overhead", label=a.label, method=name, us_per_call=round(statistics.median(us), 3),
                              min=round(min(us), 3), max=round(max(us), 3), repeats=a.repeats, calls=a.calls)), flush=True)


if __name__ == "__main__":
    main()
