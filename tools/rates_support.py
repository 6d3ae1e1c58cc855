"""What the tools/*_rates.py share: the batch a tool measures on, the alternating timer and the row writer.  The family table is
rsr_mjx_amd/envs/families.py; the seeded randomisation and the action scale are the tests' (tests/physics_support.py).

The protocol (alternate): `warmup` untimed rounds, then `rounds` timed ones, every round running the arms in the order given
(A B A B ...) in one process, so that a drift of the clocks over the run falls on all of them.  An arm is a callable, the env batch
whose timing_begin / timing_end (HIP events on the launch stream, rsr_timing_begin / _end) bracket `inner` calls of it, and that
count; the device is synchronised after every window; the time of a window is reported per call.  A tool quotes the median of an
arm's windows and their [min, max] (median, spread), one JSON line per cell with bench.csrc_sha16() in it (row_writer)."""
from __future__ import annotations

import collections
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# what a planner's cost reads on the Airbot models; the Go2 models take their env's own sensors
AIRBOT_SPEC = [("pos", "framepos", "endpoint"), ("linvel", "framelinvel", "endpoint")]

Arm = collections.namedtuple("Arm", "fn env inner", defaults=(1,))


def batch(kind, n, steps=3, dr=True, **kw):
    """The batch of a cell: families.envdef(kind).batched(n, **kw) with the family's default randomisation (dr=False: none), after
    reset(PRNGKey(0)) and `steps` env steps under clipped N(0, 1) x the action scale drawn from default_rng(0).  Returns a namespace
    of envdef, env, dr (the dict or None), scale, spec (the rollout tools' sensor table) and rng, the generator after those draws."""
    import physics_support as S
    from rsr_mjx_amd import prng
    from rsr_mjx_amd.envs import families
    envdef = families.envdef(kind)
    rand = S.default_dr(kind, envdef, n) if dr else None
    scale = S.action_scale(kind)
    env = envdef.batched(n, randomization=rand, **kw)
    env.reset(prng.split(prng.PRNGKey(0), n))
    rng = np.random.default_rng(0)
    for _ in range(steps):
        env.step(None, np.clip(rng.normal(size=(n, env.dims.nu)) * scale, -1, 1).astype(np.float32))
    return types.SimpleNamespace(envdef=envdef, env=env, dr=rand, scale=scale, rng=rng,
                                 spec=AIRBOT_SPEC if kind in S.IMPLICIT else envdef.sensors)


def alternate(arms, rounds, warmup=1, sync=None):
    """Per Arm of `arms`, the list of its `rounds` window times in ms per call (see the module docstring).  An entry of `arms` that is
    a plain callable runs in its place in every round, outside every window: a tool's own untimed step between two arms."""
    if sync is None:
        import torch
        sync = torch.cuda.synchronize
    times = [[] for a in arms if isinstance(a, Arm)]
    for r in range(warmup + rounds):
        kept = iter(times)
        for arm in arms:
            if not isinstance(arm, Arm):
                arm()
                continue
            arm.env.timing_begin()
            for _ in range(arm.inner):
                arm.fn()
            ms = arm.env.timing_end()[0]
            sync()
            t = next(kept)
            if r >= warmup:
                t.append(ms / arm.inner)
    return times


def median(x):
    return float(np.median(x))


def spread(*arms):
    """[min, max] of every arm's windows, arm after arm"""
    return [f(t) for t in arms for f in (min, max)]


def row_writer(out):
    """write(row): prints the row as one JSON line and appends it to `out` (None: prints only), which is truncated here, once"""
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").close()

    def write(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(line + "\n")
    return write
