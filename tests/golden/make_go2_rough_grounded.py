"""Rough-terrain Go2 states that stand on the terrain, for the physics-layer tests (tests/test_go2_rough_grounded_gpu.py): the reset
distribution spawns the robots clear of the ground, so the states of physics_support.random_states hardly ever touch the height
field.  Generated with this repository's fp64 oracle: the oracle's reset states of Go2JoystickRoughTerrain for PRNGKey(SEED),
position targets at the reset pose (the home keyframe), SETTLE physics substeps so that the robots land, then the perturbation of
random_states (hinge angles + N(0, 0.05), qvel + N(0, 0.2)) with the ctrl kept within N(0, 0.02) of the pose so that the feet stay
loaded, the trunk lowered to where a third foot touches and the velocity perturbation of an env halved until each of its contacts
carries load (both below; 12 halvings in all).  Written to
tests/golden/go2_rough_grounded_states.npz: inputs only (qpos, qvel, ctrl of 256 envs, float32).

On the CPU, for SEED = 11 and SETTLE = 250 (printed by this script; the test's docstring repeats them):
    the f64 oracle lists >= 3 contacts in 256 of 256 envs (needed: >= 90 %), 815 contacts in all;
    the f32 and f64 oracles disagree on (ne, nf, nl, ncon) in 0 of 256 envs (allowed: <= 2 %)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import make_go2_blob
from oracle import oracle as O
from rsr_mjx_amd import prng
from rsr_mjx_amd.envs import config
from rsr_mjx_amd.mjcf import CompiledModel

N, SEED, SETTLE = 256, 11, 250


def counts(orc, qpos, qvel, ctrl, ncon_cap):
    """[n, 4] (ne, nf, nl, ncon) of Oracle.forward from a zero warm start; condim 3: four pyramid rows per contact"""
    orc.set_ncon_cap(ncon_cap)
    out = []
    for e in range(len(qpos)):
        orc.forward(qpos[e], qvel[e], ctrl[e], np.zeros(qvel.shape[1]), step=False)
        nefc, ne, nf, ncon = (int(x) for x in orc.get("counts")[:4])
        out.append((ne, nf, nefc - ne - nf - 4 * ncon, ncon))
    return np.array(out)


def main():
    O.build()
    m = config.go2_apply_overrides(CompiledModel.load(os.path.join(ROOT, "rsr_mjx_amd", "assets", "go2_rough.npz")), config.GO2_DEFAULT_CONFIG)
    blob = make_go2_blob(m)
    A = m.arrays
    assert (A["pair_condim"] == 3).all()
    o64, o32 = O.Oracle(blob, "f64"), O.Oracle(blob, "f32")
    cap = 4                                                   # the four feet: every pair of the model (the kernel's capacity is no smaller)
    st = o64.new_state(N)
    o64.reset(st, prng.split(prng.PRNGKey(SEED), N))
    qpos, qvel = st["qpos"].astype(np.float64), st["qvel"].astype(np.float64)
    home = qpos[:, 7:].copy()
    o64.set_ncon_cap(1 << 20)
    for e in range(N):
        q, v = qpos[e], qvel[e]
        o64.forward(q, v, home[e], np.zeros(m.nv), step=False)
        for _ in range(SETTLE):
            o64.forward(q, v, home[e], o64.get("qacc"), step=True)
            q, v = o64.get("qpos"), o64.get("qvel")
        qpos[e], qvel[e] = q, v
    rng = np.random.default_rng(SEED)
    jt, qa = A["jnt_type"], A["jnt_qposadr"]
    for j in range(len(jt)):
        if jt[j] in (2, 3):
            qpos[:, qa[j]] += rng.normal(scale=0.05, size=N)
    settled_qvel = qvel.copy()
    qvel += rng.normal(scale=0.2, size=qvel.shape)
    lo, hi = A["actuator_ctrlrange"][:, 0], A["actuator_ctrlrange"][:, 1]
    ctrl = np.clip(home + rng.normal(scale=0.02, size=home.shape), lo, hi)
    # the hinge perturbation moves a foot by about a centimetre, far more than a standing foot's penetration, and lifts half the
    # feet off the ground: set each robot down again, the trunk lowered (by bisection on the f64 oracle, at most 5 cm) to where a
    # third foot touches, and 1 mm further so that the contact is no rounding matter
    o64.set_ncon_cap(cap)
    def ncon_at(e, dz):
        q = qpos[e].copy(); q[2] -= dz
        o64.forward(q, qvel[e], ctrl[e], np.zeros(m.nv), step=False)
        return int(o64.get("counts")[3])
    for e in range(N):
        if ncon_at(e, 0.0) >= 3:
            continue
        lo_, hi_ = 0.0, 0.05
        if ncon_at(e, hi_) < 3:
            continue
        for _ in range(12):
            mid = 0.5 * (lo_ + hi_)
            lo_, hi_ = (lo_, mid) if ncon_at(e, mid) >= 3 else (mid, hi_)
        qpos[e, 2] -= hi_ + 1e-3
    # a foot that the velocity perturbation lifts faster than the contact's reference acceleration asks for carries no force:
    # halve that env's velocity perturbation until every listed contact is loaded in the f64 oracle (floor: 1e-3 N)
    def loaded(e, v):
        o64.forward(qpos[e].astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64), ctrl[e].astype(np.float32),
                    np.zeros(m.nv), step=False)
        nefc, ncon = int(o64.get("counts")[0]), int(o64.get("counts")[3])
        return ncon >= 3 and o64.get("efc_force")[nefc - 4 * ncon:].reshape(ncon, 4).sum(1).min() > 1e-3
    halved = 0
    for e in range(N):
        dv = qvel[e] - settled_qvel[e]
        for k in range(6):
            if loaded(e, settled_qvel[e] + dv):
                break
            dv, halved = 0.5 * dv, halved + 1
        qvel[e] = settled_qvel[e] + dv
    print("velocity perturbation halved %d times in all" % halved)
    qpos, qvel, ctrl = qpos.astype(np.float32), qvel.astype(np.float32), ctrl.astype(np.float32)
    c64 = counts(o64, qpos.astype(np.float64), qvel.astype(np.float64), ctrl, cap)
    c32 = counts(o32, qpos.astype(np.float64), qvel.astype(np.float64), ctrl, cap)
    n3, flips = int((c64[:, 3] >= 3).sum()), int((c64 != c32).any(1).sum())
    print("f64 oracle: >= 3 contacts in %d of %d envs, %d contacts in all; f32 vs f64 row counts differ in %d envs" % (n3, N, c64[:, 3].sum(), flips))
    assert n3 >= 0.9 * N and flips <= 0.02 * N
    np.savez(os.path.join(ROOT, "tests", "golden", "go2_rough_grounded_states.npz"), qpos=qpos, qvel=qvel, ctrl=ctrl)


if __name__ == "__main__":
    main()
