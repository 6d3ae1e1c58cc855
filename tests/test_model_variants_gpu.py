"""The constraint rows of the kernels at model constants no shipped model takes (tests/model_variants.py): make_constraint and kbi
(csrc/rsr_device.hpp), the contact filter of collision(), and the host's lane records that feed them, against the CPU oracle, which
reads the raw arrays of the same blob.  For every (variant, family): the rows through Physics.inverse() (efc_force at a given
acceleration: no solver in the way), the rows through constraint_forces(), and the row counts and contact lists.

States: model_variants.device_states: random_states(envdef, kind, 256, 11) of the shipped model plus model_variants.offsets.
The reference, the error, the rule (p99 <= 1e-5 or <= 3 x the f32 oracle's p99; every env within max(1e-4, 20 x the f32 oracle's
max)) and the exclusion of envs whose row counts flip (at most 2 %): tests/physics_support.py; no bound here is new.  That the
reference itself is right at these constants, that the states reach the branches (impedance regimes, the margin band, the three
friction rules, the refsafe clamp) and that every variant moves efc_force away from the shipped model's: tests/test_model_variants.py,
on the CPU, where the f32-vs-f64 part of the exclusion leaves out 0 of 256 envs in all 18 cases.  Measured on an MI355X: the kernel's
row counts equal the f64 oracle's in every env of every case as well (0 excluded); margin go2flat lists 96 contacts with dist > 0 of
869, margin footstand 158 of 3072, and the cube's margin variant has 91 limits active at a positive limit distance."""
import numpy as np
import pytest

import model_variants as V
from physics_support import (inverse_inputs, inverse_ref, keep_constraint, keep_inverse, oracle_pass, rel, rule, setup)
from physics_support import npyr as npyr_of

N = V.N


def _start(oracle_mod, variant, kind):
    """(envdef, E, phys, ref, qpos, qvel, ctrl): the variant's batch with the states written by set_state, and oracle_pass on its
    blob (shared by the three tests of a case)"""
    envdef, E, phys, _, _, _ = setup(kind, n=N, seed=V.SEED, variant=variant)
    qpos, qvel, ctrl = V.device_states(envdef, kind)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    ref = oracle_pass(oracle_mod, E.blob, E.dims, qpos, qvel, ctrl)
    return envdef, E, phys, ref, qpos, qvel, ctrl


def _dev(x, phys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=phys.device).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("variant,kind", V.CASES)
def test_rows_through_inverse(oracle_mod, variant, kind):
    """inverse_efc_force and inverse_qfrc_constraint at a = zeros and at the noisy acceleration of the inverse parity test, against
    physics_support.inverse_ref on the f64 oracle's rows of the variant's blob (spread: the same on the f32 oracle's rows in
    fp32).  The blob is the one model_variants.blob_of builds on the CPU."""
    import torch
    envdef, E, phys, ref, qpos, qvel, ctrl = _start(oracle_mod, variant, kind)
    assert E.blob == V.blob_of(envdef)
    d, npyr = E.dims, npyr_of(E)
    fails, keep, biggest = [], None, 0.0
    inputs = inverse_inputs(ref["f64"], V.SEED)
    for name in ("zeros", "noisy"):
        a = inputs[name]
        phys.inverse(_dev(a, phys))
        torch.cuda.synchronize()
        if keep is None:
            keep = keep_inverse(f"{variant} {kind}", phys, ref, npyr)
        r64 = [inverse_ref(ref["f64"][e], a[e], np.float64, d.nefc_max) for e in range(N)]
        r32 = [inverse_ref(ref["f32"][e], a[e], np.float32, d.nefc_max) for e in range(N)]
        views = dict(efc_force=phys.inverse_efc_force, qfrc_constraint=phys.inverse_qfrc_constraint)
        for f, t in views.items():
            h = t.cpu().numpy().astype(np.float64)
            s64, s32 = np.stack([r[f] for r in r64]), np.stack([r[f] for r in r32])
            rule(f"{variant} {kind}", f"{f} at {name}", rel(h, s64)[keep], rel(s32, s64)[keep], fails)
        nefc = phys.inverse_efc_counts[:, 0].cpu().numpy().astype(int)
        ef = phys.inverse_efc_force.cpu().numpy()
        assert all((ef[e, nefc[e]:] == 0).all() for e in range(N))
        biggest = max(biggest, float(np.abs(ef).max()))
    assert biggest > 1.0, "no constraint force anywhere: the test shows nothing"
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("variant,kind", V.CASES)
def test_rows_through_the_forward_path(oracle_mod, variant, kind):
    """efc_force, qfrc_constraint, constraint_qacc and efc_counts after set_state + constraint_forces() from a zeroed warm start
    against Oracle.forward(q, v, ctrl, zeros) on the variant's blob, as test_constraint_gpu.test_constraint_forces_match_the_oracle
    does on the shipped models."""
    import torch
    envdef, E, phys, ref, qpos, qvel, ctrl = _start(oracle_mod, variant, kind)
    phys.qacc_warmstart.zero_()                                    # (set_state leaves the forward pass's qacc there)
    phys.constraint_forces()
    torch.cuda.synchronize()
    keep = keep_constraint(f"{variant} {kind}", phys, ref, npyr_of(E))
    hip = dict(efc_force=phys.efc_force, qfrc_constraint=phys.qfrc_constraint, qacc=phys.constraint_qacc)
    fails = []
    for f, t in hip.items():
        h = t.cpu().numpy().astype(np.float64)
        r64, r32 = (np.stack([r[f] for r in ref[p]]) for p in ("f64", "f32"))
        rule(f"{variant} {kind}", f, rel(h, r64)[keep], rel(r32, r64)[keep], fails)
    nefc = phys.efc_counts[:, 0].cpu().numpy().astype(int)
    ef = phys.efc_force.cpu().numpy()
    assert all((ef[e, nefc[e]:] == 0).all() for e in range(N))
    assert (nefc[keep] == np.array([r["nefc"] for r in ref["f64"]])[keep]).all()
    assert np.abs(ef).max() > 1.0, "no constraint force anywhere: the test shows nothing"
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("variant,kind", V.CASES)
def test_counts_and_contacts(oracle_mod, variant, kind):
    """efc_counts and contacts() against the f64 oracle on every kept env: ncon, ncon_dropped against the oracle's count without
    the contact cap, the geom ids in the oracle's order, dist to 2e-5 (the bound of test_physics_contacts_view;
    as there, the points of one geom pair are matched by depth).  On every env:
    each listed contact has dist < margin - gap of its pair, in the fp32 the kernel compares in.  With a margin (variants margin
    and combined) on the Go2 families, contacts with 0 < dist < margin - gap are on the device, in 5 % of its contacts at the
    least; on the cube active limits with a positive limit distance, one per 10 envs at the least (the counts of
    tests/test_model_variants.py, here on the device's own lists)."""
    import torch
    envdef, E, phys, ref, qpos, qvel, ctrl = _start(oracle_mod, variant, kind)
    A = envdef.sys.arrays
    c = {k: v.cpu().numpy() for k, v in phys.contacts().items()}
    phys.constraint_forces()
    torch.cuda.synchronize()
    npyr, cap = npyr_of(E), E.dims.ncon_max
    keep = keep_constraint(f"{variant} {kind}", phys, ref, npyr)            # (the order of the geom ids on the kept envs included)
    assert (phys.contact_forces()["ncon"].cpu().numpy() == c["ncon"]).all()
    o = oracle_mod.Oracle(E.blob, "f64")
    o.set_ncon_cap(1 << 20)
    uncapped = []
    for e in range(N):
        o.forward(qpos[e], qvel[e], ctrl[e], None)
        uncapped.append(int(o.get("counts")[3]))
    incl = (np.asarray(A["pair_margin"]) - np.asarray(A["pair_gap"])).astype(np.float32)
    hc = phys.efc_counts.cpu().numpy().astype(int)
    in_band = total = 0
    for e in np.nonzero(keep)[0]:
        r = ref["f64"][e]
        nc = int(c["ncon"][e])
        assert nc == r["ncon"] == min(uncapped[e], cap) and nc + int(c["ncon_dropped"][e]) == uncapped[e], (variant, kind, e)
        assert [hc[e, 1], hc[e, 2]] == [r["ne"], r["nf"]] and hc[e, 3] == r["nefc"] - r["ne"] - r["nf"] - npyr * r["ncon"]
        pairs = r["contacts"][:, 9].astype(int)
        assert (c["geom1"][e, :nc] == A["pair_geom1"][pairs]).all() and (c["geom2"][e, :nc] == A["pair_geom2"][pairs]).all(), (variant, kind, e)
        order = lambda dist: np.lexsort((dist, pairs))              # (the points of one manifold come in either order: by depth)
        hd, rd = c["dist"][e, :nc], r["contacts"][:, 0]
        assert np.abs(hd[order(hd)] - rd[order(rd)]).max(initial=0.0) <= 2e-5, (variant, kind, e)
        assert (c["dist"][e, :nc] < incl[pairs]).all(), (variant, kind, e)
        assert (c["geom1"][e, nc:] == -1).all() and (c["dist"][e, nc:] == 0).all()
        in_band += int((c["dist"][e, :nc] > 0).sum())
        total += nc
    # every env, kept or not: no listed contact at or beyond the largest margin - gap, none at a positive distance without a margin
    live = np.arange(cap)[None, :] < c["ncon"][:, None]
    assert (c["dist"][live] < incl.max()).all()
    print(variant, kind, "contacts on kept envs: %d, with dist > 0: %d" % (total, in_band))
    assert total > N // 4
    if variant in ("margin", "combined"):
        if kind == "cube":
            lim = sum(len(V.positive_limits(A, qpos[e])) for e in np.nonzero(keep)[0])
            print(variant, kind, "active limits with a positive limit distance:", lim)
            assert lim >= N / 10
        else:
            assert in_band >= 0.05 * total, (in_band, total)
    else:
        assert in_band == 0
