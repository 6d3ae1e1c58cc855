"""Physics-level API (rsr_physics_step / rsr_physics_forward / rsr_physics_view, rsr_mjx_amd/physics.py) on every built family:
bit-identity with the fused env step, parity with the CPU oracle's forward / step, the contacts view, set_state semantics."""
import numpy as np
import pytest

from boxbox_cases import by_pair, match_sets
from planeprim_cases import PAIR_PLANE_CAPSULE, PAIR_PLANE_CYLINDER, PAIR_PLANE_SPHERE
from physics_support import FAMILIES, PIPE, assert_unchanged, bits, handle_snapshot, make, random_states, rel, rule
from rsr_mjx_amd import prng

PRIMITIVE_KINDS = (PAIR_PLANE_SPHERE, PAIR_PLANE_CAPSULE, PAIR_PLANE_CYLINDER)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_physics_step_is_bit_identical_to_env_step(kind):
    """Teacher-forced: S0 after a few env steps; env.step(a) -> S1 with its ctrl; S0 written into a second batch with the same DR;
    physics.step(ctrl, n_frames) there must land on S1 bit for bit."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 1024
    dr_on = kind != "tshape"                 # (the Airbot randomisation of domain_randomize.py is the cube scene's)
    _, A, dr, scale = make(kind, n, dr_on)
    _, B, _, _ = make(kind, n, dr_on)
    rng = np.random.default_rng(3)
    nu = A.dims.nu
    act = lambda: np.clip(rng.normal(size=(n, nu)) * scale, -1, 1).astype(np.float32)
    A.reset(prng.split(prng.PRNGKey(7), n))
    B.reset(prng.split(prng.PRNGKey(8), n))
    for _ in range(3):
        A.step(None, act())
    for k in ("qpos", "qvel", "qacc_warmstart", "time", "xpos", "site_xpos", "ctrl"):
        B.view(k).copy_(A.view(k))
    A.step(None, act())
    ctrl1 = A.view("ctrl").clone()
    phys = Physics(B)
    assert phys.n_substeps == A.dims.n_frames
    keep = {k: B.view(k).clone() for k in ("obs", "reward", "done", "metrics", "first_qpos", "info_go2", "stats")}
    phys.step(ctrl1, phys.n_substeps)
    torch.cuda.synchronize()
    for k in ("qpos", "qvel", "qacc_warmstart", "time", "xpos", "site_xpos", "ctrl"):
        a, b = A.view(k).cpu().numpy(), B.view(k).cpu().numpy()
        bad = np.nonzero((a.view(np.int32) != b.view(np.int32)).any(1))[0]
        assert bad.size == 0, f"{kind} {k}: {bad.size} envs differ, first {bad[:5]}, max |d| {np.abs(a - b).max():.3e}"
    # the physics call leaves the env's bookkeeping alone
    for k, v in keep.items():                 # (bitwise: the Go2 info block holds PRNG key words, some of them NaN patterns)
        assert torch.equal(B.view(k).view(torch.int32), v.view(torch.int32)), k
    # and the side buffer holds the last forward pass: qacc = the warm start it leaves
    np.testing.assert_array_equal(phys.qacc.cpu().numpy(), B.view("qacc_warmstart").cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_physics_oracle_parity(oracle_mod, kind):
    """forward and step (nsteps 1 and n_frames) against the oracle's debug forward / step, per env, DR off.  Kinematic fields
    (xpos, xquat, site_xpos) within 1e-5 everywhere; dynamic fields (qacc, qvel, actuator_force, and qpos after n_frames) under
    the rule of tests/physics_support.py (its 3 x arm is met by the acceleration-level fields of the ill-conditioned Airbot solves).
    An env whose active contact set differs from the f64 oracle's (a contact mode flip) is counted, and the count is bounded (2 %),
    not the error."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 256
    envdef, E, _, _ = make(kind, n, False)
    E.reset(prng.split(prng.PRNGKey(1), n))
    qpos, qvel, ctrl = random_states(envdef, kind, n, 11)
    phys = Physics(E)
    nf = phys.n_substeps
    o32 = oracle_mod.Oracle(E.blob); o32.set_ncon_cap(E.dims.ncon_max)
    o64 = oracle_mod.Oracle(E.blob, "f64"); o64.set_ncon_cap(E.dims.ncon_max)
    fields = ("qpos", "qvel", "qacc", "actuator_force", "xpos", "xquat", "site_xpos")
    fails = []
    for mode, nsteps in (("forward", 0), ("step1", 1), ("stepN", nf)):
        phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
        if nsteps:
            phys.step(None, nsteps)
        torch.cuda.synchronize()
        hip = {f: getattr(phys, f).cpu().numpy().reshape(n, -1) for f in fields}
        ref = {p: {f: np.zeros((n, hip[f].shape[1])) for f in fields} for p in ("f32", "f64")}
        ncon = {p: np.zeros(n, int) for p in ("f32", "f64")}
        for e in range(n):
            for p, o in (("f32", o32), ("f64", o64)):
                # set_state = mjx_env.init: forward from a zero warm start, which leaves qacc_warmstart = qacc; each substep
                # warm-starts from the previous forward pass's qacc (the Go2 solve is one Newton iteration: the start matters)
                q, v = qpos[e].astype(np.float64), qvel[e].astype(np.float64)
                o.forward(q, v, ctrl[e], np.zeros(E.dims.nv), step=False)
                for s in range(nsteps):
                    w = o.get("qacc")
                    o.forward(q, v, ctrl[e], w, step=True)
                    q, v = o.get("qpos"), o.get("qvel")
                for f in fields:
                    ref[p][f][e] = o.get(f)
                ncon[p][e] = int(o.get("counts")[3])
        hip_ncon = phys.contacts()["ncon"].cpu().numpy()
        flips = (hip_ncon != ncon["f64"]) | (ncon["f32"] != ncon["f64"])
        print(kind, mode, "contact-mode flips in %d of %d envs" % (flips.sum(), n))
        if flips.mean() > 0.02:
            fails.append(f"{kind} {mode}: contact-mode flips in {flips.sum()} of {n} envs")
        keep = ~flips
        for f in fields:
            err = rel(hip[f], ref["f64"][f])[keep]
            spread = rel(ref["f32"][f], ref["f64"][f])[keep]
            if f in ("xpos", "xquat", "site_xpos") and mode == "forward":
                print(kind, mode, f, "max %.2e" % err.max())
                if err.max() > 1e-5:
                    fails.append(f"{kind} {mode} {f}: max {err.max():.2e}")
            else:
                rule(kind, f"{mode} {f}", err, spread, fails)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAMILIES)
def test_physics_contacts_view(oracle_mod, kind):
    """Active contacts after forward() against the oracle's narrow phase on the same state (f64, contacts on the oracle's own
    geom_xpos / geom_xmat): count, depth and normal per (geom1, geom2) pair, and for plane-sphere, -capsule and -cylinder pairs
    also pos, set-matched per pair within 2e-5; ncon_dropped = uncapped count - capped count."""
    import torch
    from rsr_mjx_amd.physics import Physics
    n = 256
    envdef, E, _, _ = make(kind, n, False)
    E.reset(prng.split(prng.PRNGKey(2), n))
    qpos, qvel, ctrl = random_states(envdef, kind, n, 12)
    if kind == "footstand":                          # lower the trunk onto the floor: capsule / cylinder contacts, over the cap
        qpos[: n // 2, 2] = 0.08
    phys = Physics(E)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    torch.cuda.synchronize()
    c = {k: v.cpu().numpy() for k, v in phys.contacts().items()}
    cap = E.dims.ncon_max
    A = envdef.sys.arrays
    pg1, pg2 = A["pair_geom1"], A["pair_geom2"]
    o = oracle_mod.Oracle(E.blob, "f64")
    pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(pg1, pg2))}
    mismatch = pos_checked = 0
    for e in range(n):
        o.set_ncon_cap(1 << 20)
        o.forward(qpos[e], qvel[e], ctrl[e], None)
        total = int(o.get("counts")[3])
        o.set_ncon_cap(cap)
        o.forward(qpos[e], qvel[e], ctrl[e], None)
        rc = o.get("contacts").reshape(-1, 10)
        nc = int(c["ncon"][e])
        if nc != len(rc) or nc + int(c["ncon_dropped"][e]) != total:
            mismatch += 1
            continue
        assert nc == min(total, cap)
        hip = sorted(zip(c["geom1"][e, :nc], c["geom2"][e, :nc], c["dist"][e, :nc], map(tuple, c["normal"][e, :nc])))
        orc = sorted(zip(pg1[rc[:, 9].astype(int)], pg2[rc[:, 9].astype(int)], rc[:, 0], map(tuple, rc[:, 4:7])))
        for h, r in zip(hip, orc):
            assert (h[0], h[1]) == (r[0], r[1]), (kind, e, h, r)
            assert abs(h[2] - r[2]) <= 2e-5, (kind, e, h[2], r[2])
            assert np.abs(np.array(h[3]) - np.array(r[3])).max() <= 1e-4, (kind, e)      # (height-field facet normals: 2e-5 in fp32)
        assert (c["geom1"][e, nc:] == -1).all() and (c["dist"][e, nc:] == 0).all()
        # spheres, capsules and cylinders against a plane have no selection step: the points of a pair are the same set, so pos too
        hp = by_pair([pair_of[(int(a), int(b))] for a, b in zip(c["geom1"][e, :nc], c["geom2"][e, :nc])], c["dist"][e, :nc], c["pos"][e, :nc], c["normal"][e, :nc])
        for p, (_, opos, _) in by_pair(rc[:, 9], rc[:, 0], rc[:, 1:4], rc[:, 4:7]).items():
            if int(A["pair_kind"][p]) in PRIMITIVE_KINDS:
                assert p in hp and len(hp[p][1]) == len(opos), (kind, e, p)
                assert match_sets(opos, hp[p][1])[1] <= 2e-5, (kind, e, p, opos, hp[p][1])
                pos_checked += 1
    assert mismatch <= max(2, n // 100), f"{kind}: contact count differs from the oracle in {mismatch} of {n} envs"
    assert pos_checked > 0 or kind in ("cube", "tshape", "go2rough"), kind
    if kind == "footstand":
        assert (c["ncon_dropped"] > 0).any() and (c["ncon"] == cap).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "go2flat"])
def test_set_state_semantics(oracle_mod, kind):
    import ctypes as C
    import torch
    from rsr_mjx_amd import _lib, mjcf
    from rsr_mjx_amd.physics import Physics
    n = 128
    envdef, E, _, scale = make(kind, n, False)
    E.reset(prng.split(prng.PRNGKey(4), n))
    rng = np.random.default_rng(0)
    E.step(None, np.clip(rng.normal(size=(n, E.dims.nu)) * scale, -1, 1).astype(np.float32))
    phys = Physics(E)
    phys.forward()
    torch.cuda.synchronize()
    qpos, qvel, ctrl = random_states(envdef, kind, n, 13)
    # subset write: the other envs' record and physics outputs are bit-unchanged
    before = handle_snapshot(phys, ("record", "side"))
    ids = np.array([3, 17, 64, 100])
    phys.set_state(qpos=qpos[ids], qvel=qvel[ids], ctrl=ctrl[ids], env_ids=ids)
    others = np.setdiff1d(np.arange(n), ids)
    rows = lambda snap: {k: v[others] for k, v in snap.items()}
    assert_unchanged(rows(before), rows(handle_snapshot(phys, ("record", "side"))))
    np.testing.assert_array_equal(phys.qpos[ids].cpu().numpy(), qpos[ids])
    np.testing.assert_array_equal(phys.qacc_warmstart[ids].cpu().numpy(), phys.qacc[ids].cpu().numpy())
    # every env: kinematics consistent with the state that was set (fp64 forward kinematics, oracle site positions)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    torch.cuda.synchronize()
    xpos, xquat, sx = (phys.xpos.cpu().numpy(), phys.xquat.cpu().numpy(), phys.site_xpos.cpu().numpy())
    o = oracle_mod.Oracle(E.blob, "f64")
    for e in range(0, n, 8):
        kin = mjcf.forward_kinematics(envdef.sys, qpos[e].astype(np.float64))
        np.testing.assert_allclose(xpos[e], kin["xpos"], atol=1e-5)
        q, r = xquat[e], kin["xquat"]
        assert np.minimum(np.abs(q - r).max(1), np.abs(q + r).max(1)).max() <= 1e-5
        o.forward(qpos[e], qvel[e], ctrl[e], None)
        np.testing.assert_allclose(sx[e].ravel(), o.get("site_xpos"), atol=1e-5)
    # set_state then env.step == the fused step from the same pipeline state written directly into another batch
    _, F, _, _ = make(kind, n, False)
    F.reset(prng.split(prng.PRNGKey(9), n))
    for k in PIPE:
        F.view(k).copy_(E.view(k))
    for k in ("info_target_pos", "info_new_cube_pos", "info_go2"):
        F.view(k).copy_(E.view(k))
    a = np.clip(rng.normal(size=(n, E.dims.nu)) * scale, -1, 1).astype(np.float32)
    E.step(None, a)
    F.step(None, a)
    torch.cuda.synchronize()
    for k in PIPE + ("obs", "reward"):
        assert torch.equal(bits(E.view(k)), bits(F.view(k))), k
    # argument errors
    with pytest.raises(ValueError):
        phys.step(np.zeros((n, E.dims.nu + 1), np.float32))
    with pytest.raises(ValueError):
        phys.step(None, 0)
    with pytest.raises(ValueError):
        phys.set_state(qpos=qpos[:5], env_ids=[0, 1])
    with pytest.raises(ValueError):
        phys.set_state(qpos=qpos[:1], env_ids=[n])
    assert _lib.lib().rsr_physics_step(phys._h, None, 0, None) == -1
    assert _lib.lib().rsr_physics_step(phys._h, None, -3, None) == -1
    assert _lib.lib().rsr_physics_forward_envs(phys._h, None, 1, None) == -1
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    assert _lib.lib().rsr_physics_view(phys._h, len(_lib.PHYS_FIELDS), C.byref(ptr), shape, stride) == -1
