"""The reference of tests/test_model_variants_gpu.py, pinned on the CPU before the kernels are judged against it: for every
(variant, family) of tests/model_variants.py the f64 oracle's efc_R, efc_D and efc_aref of every row against a closed form written
in numpy fp64 from MuJoCo's definitions (engine_core_constraint: getimpedance, getsolparam, mj_makeImpedance; the pyramid weight
as MJX's constraint.py states it), the host's lane records of the variant against impedance_consts and a double-precision (k, b),
the friction-rule word against geom_priority, and the conditions under which the device tests show anything: the exclusion, the
impedance regimes, the margin band, the friction rules, the equality's offset, the refsafe clamp, and that the variant moves the
f64 oracle's efc_force away from the shipped model's.

States: model_variants.oracle_states: the f32 oracle's reset of the shipped model for PRNGKey(11), physics_support.perturb with
seed 11, model_variants.offsets.  256 envs.

Bound of the closed form: relative 1e-9 per row (both sides are double precision; the one amplification is (1 - d) / d near
d = 0.9999, at most 1e4 x 1e-15).  Measured: R and D <= 3.3e-15, aref <= 3.4e-12 over the 18 cases.  Finding: the oracle formed
three sums of the blob's fp32 constants in fp32 also in its f64 build (margin - gap, the two body_invweight0 of a contact, the two
dof_invweight0 of an equality).  Against the closed form the second showed as 5.8e-8 on the R of every Airbot contact row (the
other two are exact at these constants; on the Go2 models the floor's invweight is 0).  oracle/rsr_oracle.c now widens the terms
first; the f32 build computes what it computed.

Measured on the CPU, these states, f64 oracle.  The f32-vs-f64 part of the exclusion leaves out 0 of 256 envs in all 18 cases.
Contacts by x = |pos| / width (x < mid / mid <= x < 1 / x >= 1), of them with dist > 0; active limits the same way, of them with a
positive limit distance; contacts by friction rule 0 / 1 / 2 (all between geoms of different friction); contacts on pairs with the
time constant under 2 dt / not; envs with |dif| > 1e-2 of the equality; envs whose efc_force moved by > 1e-3 against the shipped model:
  impedance  cube       contacts  792 /  558 /  591; limits 323 / 220 / 219; moved 256
  impedance  go2flat    contacts  143 /  137 /  493; no active limit;        moved 223
  impedance  footstand  contacts  204 /  220 / 2648; no active limit;        moved 256
  margin     cube       contacts 1941, dist > 0: 0; limits 853, dist > 0: 91 (762 active without the margin); moved 256
  margin     go2flat    contacts  869, dist > 0:  96 (773 without the margin); moved 231
  margin     footstand  contacts 3072 (the cap of 12 in every env), dist > 0: 158; moved 256
  impratio   cube 1941 contacts, moved 252; go2flat 773 contacts, moved 215
  friction_rule  cube       rules 471 / 506 / 964;   moved 254
  friction_rule  footstand  rules 976 / 1074 / 1022; moved 256
  solref (and solref_refsafe_off)  cube     clamped 1009, not 932; moved 256 (256)
  solref (and solref_refsafe_off)  go2flat  clamped  382, not 391; moved 228 (229)
  eq_poly    cube |dif| > 1e-2 in 219 envs, moved 255; tshape 217, moved 256
  combined   cube       contacts 599 / 1121 / 221; limits 73 / 129 / 651, dist > 0: 91; rules 471 / 506 / 964; clamped 1009, not 932;
                        |dif| > 1e-2 in 219; moved 256
  combined   footstand  contacts 230 / 205 / 2637, dist > 0: 158; rules 957 / 1078 / 1037; clamped 1521, not 1551; moved 256
"""
import numpy as np
import pytest

import model_variants as V
import physics_support as S

MINIMP, MAXIMP, MINVAL = 1e-4, 0.9999, 1e-15
_CASES = {}


def case(oracle_mod, variant, kind):
    """dict of one (variant or None, family): envdef, A (its arrays as the blob carries them: fp32, widened), blob, dims, the CPU
    states and oracle_pass on them; built once"""
    if (variant, kind) not in _CASES:
        envdef = V.envdef_of(kind, variant)
        blob = V.blob_of(envdef)
        dims = V.dims_of(blob)
        qpos, qvel, ctrl = V.oracle_states(oracle_mod, kind)
        ref = S.oracle_pass(oracle_mod, blob, dims, qpos, qvel, ctrl)
        A = {k: (np.asarray(v).astype(np.float32).astype(np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v))
             for k, v in envdef.sys.arrays.items()}
        _CASES[(variant, kind)] = dict(envdef=envdef, A=A, blob=blob, dims=dims, qpos=qpos, qvel=qvel, ctrl=ctrl, ref=ref, npyr=S.npyr(envdef))
    return _CASES[(variant, kind)]


# ---- MuJoCo's definitions, fp64

def impedance(solimp, pos):
    """(d, x) of getimpedance: x = |pos| / width; y = x^p / mid^(p-1) below the midpoint, 1 - (1-x)^p / (1-mid)^(p-1) above it,
    1 from x = 1 on; d = d0 + y (d_width - d0)"""
    d0, dw, mid = (min(max(float(v), MINIMP), MAXIMP) for v in (solimp[0], solimp[1], solimp[3]))
    width, power = max(float(solimp[2]), MINVAL), max(float(solimp[4]), 1.0)
    x = abs(pos) / width
    if x >= 1.0:
        return dw, x
    y = x ** power / mid ** (power - 1.0) if x < mid else 1.0 - (1.0 - x) ** power / (1.0 - mid) ** (power - 1.0)
    return d0 + y * (dw - d0), x


def stiffness_damping(solref, solimp, dt, refsafe):
    """(k, b) of mj_makeImpedance: positive solref is (time constant, damping ratio), the time constant kept >= 2 dt unless
    refsafe is disabled; non-positive solref is (-stiffness, -damping); both scaled by d_width"""
    dw = min(max(float(solimp[1]), MINIMP), MAXIMP)
    tc, dr = float(solref[0]), float(solref[1])
    if refsafe:
        tc = max(tc, 2.0 * dt)
    k = 1.0 / (dw * dw * tc * tc * dr * dr) if solref[0] > 0 else -float(solref[0]) / (dw * dw)
    b = 2.0 / (dw * tc) if solref[1] > 0 else -float(solref[1]) / dw
    return k, b


def rule_of(A, pair):
    g1, g2 = int(A["pair_geom1"][pair]), int(A["pair_geom2"][pair])
    p1, p2 = int(A["geom_priority"][g1]), int(A["geom_priority"][g2])
    return 0 if p1 == p2 else (1 if p1 > p2 else 2)


def contact_friction(A, pair):
    """(sliding, torsional) of a contact: the higher-priority geom's, the element-wise maximum at equal priority"""
    g1, g2 = int(A["pair_geom1"][pair]), int(A["pair_geom2"][pair])
    f1, f2 = A["geom_friction"][g1], A["geom_friction"][g2]
    f = (np.maximum(f1, f2), f1, f2)[rule_of(A, pair)]
    return float(f[0]), float(f[1])


def rows_of(A, r, qpos):
    """The rows of oracle env r (one of oracle_pass's) in MuJoCo's order -- active equalities, dofs with friction loss, active
    limits, contacts (2 (condim - 1) pyramid edges each) -- as dicts(type, pos, invweight, solref, solimp, id), from the model
    arrays, qpos and the oracle's contact list alone."""
    q = np.asarray(qpos, np.float64)
    out = []
    for e in range(len(A["eq_obj1id"])):
        if not A["eq_active0"][e]:
            continue
        j1, j2 = int(A["eq_obj1id"][e]), int(A["eq_obj2id"][e])
        a1 = int(A["jnt_qposadr"][j1])
        iw = A["dof_invweight0"][int(A["jnt_dofadr"][j1])]
        dif = 0.0
        if j2 >= 0:
            a2 = int(A["jnt_qposadr"][j2])
            dif = q[a2] - A["qpos0"][a2]
            iw = iw + A["dof_invweight0"][int(A["jnt_dofadr"][j2])]
        c = A["eq_data"][e]
        pos = (q[a1] - A["qpos0"][a1]) - (c[0] + c[1] * dif + c[2] * dif ** 2 + c[3] * dif ** 3 + c[4] * dif ** 4)
        out.append(dict(type="eq", pos=pos, invweight=iw, solref=A["eq_solref"][e], solimp=A["eq_solimp"][e], id=e, dif=dif))
    for i in range(len(A["dof_frictionloss"])):
        if A["dof_frictionloss"][i] > 0:
            out.append(dict(type="fric", pos=0.0, invweight=A["dof_invweight0"][i], solref=A["dof_solref"][i], solimp=A["dof_solimp"][i], id=i))
    for j in range(len(A["jnt_type"])):
        if not A["jnt_limited"][j] or int(A["jnt_type"][j]) not in (2, 3):
            continue
        x = q[int(A["jnt_qposadr"][j])]
        dist = min(x - A["jnt_range"][j, 0], A["jnt_range"][j, 1] - x)
        pos = dist - A["jnt_margin"][j]
        if pos < 0:
            out.append(dict(type="limit", pos=pos, invweight=A["dof_invweight0"][int(A["jnt_dofadr"][j])], solref=A["jnt_solref"][j],
                            solimp=A["jnt_solimp"][j], id=j, dist=dist))
    condim = int(A["pair_condim"][0])
    for c in r["contacts"]:
        p = int(c[9])
        pos = c[0] - (A["pair_margin"][p] - A["pair_gap"][p])
        t = A["body_invweight0"][int(c[7]), 0] + A["body_invweight0"][int(c[8]), 0]
        mu = contact_friction(A, p)[0]
        iw = (t + mu * mu * t) * 2.0 * mu * mu / A["opt_impratio"][0]
        for _ in range(2 * (condim - 1)):
            out.append(dict(type="contact", pos=pos, invweight=iw, solref=A["pair_solref"][p], solimp=A["pair_solimp"][p], id=p, dist=c[0]))
    return out


def closed_form(A, r, qpos, qvel):
    """(R, D, aref, rows) of oracle env r: R = invweight (1 - d) / d floored at mjMINVAL, D = 1 / R,
    aref = -b (J . qvel) - k d pos with the oracle's own efc_J"""
    rows = rows_of(A, r, qpos)
    dt, refsafe = float(A["opt_timestep"][0]), int(A["opt_disable_refsafe"][0]) == 0
    vel = r["efc_J"] @ np.asarray(qvel, np.float64)
    R, aref = np.zeros(len(rows)), np.zeros(len(rows))
    for i, w in enumerate(rows):
        d, w["x"] = impedance(w["solimp"], w["pos"])
        w["k"], w["b"] = stiffness_damping(w["solref"], w["solimp"], dt, refsafe)
        R[i] = max(w["invweight"] * (1.0 - d) / d, MINVAL)
        aref[i] = -w["b"] * vel[i] - w["k"] * d * w["pos"] if len(vel) == len(rows) else np.nan
    return R, 1.0 / R, aref, rows


def all_rows(c):
    """closed_form of every env of a case: [(R, D, aref, rows)]; cached on the case"""
    if "closed" not in c:
        c["closed"] = [closed_form(c["A"], c["ref"]["f64"][e], c["qpos"][e], c["qvel"][e]) for e in range(V.N)]
    return c["closed"]


# ---- the tests

@pytest.mark.parametrize("variant,kind", V.CASES)
def test_the_oracle_rows_match_the_closed_form(oracle_mod, variant, kind):
    """efc_R, efc_D and efc_aref of every row of every env, relative 1e-9; the row count and the friction-loss rows first."""
    c = case(oracle_mod, variant, kind)
    worst = dict(R=0.0, D=0.0, aref=0.0)
    nrows = 0
    for e in range(V.N):
        r = c["ref"]["f64"][e]
        R, D, aref, rows = all_rows(c)[e]
        assert len(rows) == r["nefc"], (variant, kind, e, len(rows), r["nefc"])
        assert [w["type"] for w in rows].count("eq") == r["ne"] and [w["type"] for w in rows].count("fric") == r["nf"]
        for name, mine, his in (("R", R, r["efc_R"]), ("D", D, r["efc_D"]), ("aref", aref, r["efc_aref"])):
            err = np.abs(mine - his) / np.maximum(np.abs(his), 1e-300)
            err[(mine == 0) & (his == 0)] = 0.0
            worst[name] = max(worst[name], float(err.max()))
            assert (err <= 1e-9).all(), (variant, kind, e, name, int(err.argmax()), rows[int(err.argmax())]["type"], float(err.max()))
        nrows += len(rows)
    print(variant, kind, "rows %d, worst relative error R %.1e D %.1e aref %.1e" % (nrows, worst["R"], worst["D"], worst["aref"]))
    assert nrows > 10 * V.N


@pytest.mark.parametrize("variant,kind", V.CASES)
def test_the_lane_records_carry_the_variant(variant, kind):
    """model.lane_records of every variant: the quads of the friction-loss rows (23-25), the limits (27-29), the pairs (34-35, the
    margin of 30, the friction-rule word of 32) and the equalities (38-40) against impedance_consts, the raw arrays and a
    double-precision (k, b) to fp32 rounding: what test_mjcf.test_lane_records_restate_the_model_tables checks on the shipped
    models, here with negative solref, refsafe off, power != 2, margins and priorities."""
    from rsr_mjx_amd import model as M
    envdef = V.envdef_of(kind, variant)
    m, A = envdef.sys, envdef.sys.arrays
    topo = M.topology_tables(m)
    fields = M.model_fields(m)
    rec = fields["lane_rec"]
    fv = rec.view(np.float32)
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    dt, refsafe = float(np.float32(A["opt_timestep"][0])), int(A["opt_disable_refsafe"][0]) == 0
    kb = lambda solref, solimp: stiffness_damping(f32(solref).astype(np.float64), f32(solimp).astype(np.float64), dt, refsafe)
    for l, i in enumerate(topo["fric_dofs"]):
        i = int(i)
        assert rec[23, l, 0] == i
        np.testing.assert_allclose(fv[23, l, 2:], kb(A["dof_solref"][i], A["dof_solimp"][i]), rtol=1e-6)
        np.testing.assert_array_equal([*fv[24, l], fv[25, l, 0]], M.impedance_consts(A["dof_solimp"][i]))
    for l, j in enumerate(topo["limit_jnts"]):
        j = int(j)
        assert fv[27, l, 0] == np.float32(A["jnt_margin"][j]) and rec[29, l, 1] == j
        np.testing.assert_allclose(fv[27, l, 2:], kb(A["jnt_solref"][j], A["jnt_solimp"][j]), rtol=1e-6)
        np.testing.assert_array_equal([*fv[28, l], fv[29, l, 0]], M.impedance_consts(A["jnt_solimp"][j]))
    A64 = {k: np.asarray(v) for k, v in A.items()}
    for q in range(m.npair):
        np.testing.assert_allclose(fv[30, q, 3], float(A["pair_margin"][q]) - float(A["pair_gap"][q]), rtol=1e-6, atol=0)
        assert fv[30, q, 3] == fields["pair_incl"][q]
        assert rec[32, q, 3] == rule_of(A64, q)
        np.testing.assert_allclose(fv[34, q, :2], kb(A["pair_solref"][q], A["pair_solimp"][q]), rtol=1e-6)
        np.testing.assert_array_equal([*fv[34, q, 2:], *fv[35, q, :3]], M.impedance_consts(A["pair_solimp"][q]))
    for e in range(len(A["eq_obj1id"])):
        np.testing.assert_array_equal([*fv[38, e], fv[39, e, 0]], f32(A["eq_data"][e]))
        np.testing.assert_allclose(fv[39, e, 1:3], kb(A["eq_solref"][e], A["eq_solimp"][e]), rtol=1e-6)
        np.testing.assert_array_equal([fv[39, e, 3], *fv[40, e]], M.impedance_consts(A["eq_solimp"][e]))
    # the constants the variant sets did arrive: one spot check per variant on what the records carry
    if variant in ("impedance", "combined"):
        assert set(fv[35, :m.npair, 2].tolist()) == {np.float32(V.IMP_A[4]), np.float32(V.IMP_B[4])}
        assert set(fv[35, :m.npair, 1].tolist()) == {np.float32(V.IMP_A[3]), np.float32(V.IMP_B[3])}
    if variant in ("solref", "solref_refsafe_off", "combined"):
        assert (fv[27, :len(topo["limit_jnts"]), 2] > 800.0).all()             # -solref[0] / d_width^2
    if variant == "solref_refsafe_off":
        safe = M.model_fields(V.envdef_of(kind, "solref").sys)["lane_rec"].view(np.float32)
        clamped = f32(A["pair_solref"])[:, 0] < 2 * dt
        assert clamped.any() and (~clamped).any()
        assert (fv[34, :m.npair, 0][clamped] > 1.5 * safe[34, :m.npair, 0][clamped]).all()      # (2 dt / 0.004)^2 = 1.56 (Airbot), 4 (Go2)
        np.testing.assert_array_equal(fv[34, :m.npair, 0][~clamped], safe[34, :m.npair, 0][~clamped])


def coverage(c, variant, kind):
    """what the coverage conditions count on a case, as a dict of numbers"""
    A, ref = c["A"], c["ref"]
    c64, c32 = S.counts_of(ref["f64"], c["npyr"]), S.counts_of(ref["f32"], c["npyr"])
    out = dict(excluded=int((c64 != c32).any(1).sum()))
    closed = all_rows(c)
    con = [w for _, _, _, rows in closed for w in rows[::1] if w["type"] == "contact"][::c["npyr"]]
    lim = [w for _, _, _, rows in closed for w in rows if w["type"] == "limit"]
    out["contacts"], out["limits"] = len(con), len(lim)
    for name, ws in (("con", con), ("lim", lim)):
        x = np.array([w["x"] for w in ws])
        mid = np.array([min(max(w["solimp"][3], MINIMP), MAXIMP) for w in ws])
        out[name + "_below_mid"], out[name + "_mid_to_1"], out[name + "_from_1"] = int((x < mid).sum()), int(((x >= mid) & (x < 1)).sum()), int((x >= 1).sum())
    out["con_dist_pos"] = sum(w["dist"] > 0 for w in con)
    out["lim_dist_pos"] = sum(w["dist"] > 0 for w in lim)
    rules = np.array([rule_of(A, w["id"]) for w in con])
    differ = np.array([(A["geom_friction"][int(A["pair_geom1"][w["id"]])][:2] != A["geom_friction"][int(A["pair_geom2"][w["id"]])][:2]).all()
                       for w in con], bool)
    for k in (0, 1, 2):
        out["rule%d" % k] = int(((rules == k) & differ).sum()) if len(con) else 0
    out["eq_dif_big"] = sum(any(w["type"] == "eq" and abs(w["dif"]) > 1e-2 for w in rows) for _, _, _, rows in closed)
    dt = float(A["opt_timestep"][0])
    out["con_clamped"] = sum(0 < w["solref"][0] < 2 * dt for w in con)
    out["con_unclamped"] = sum(w["solref"][0] >= 2 * dt for w in con)
    return out


@pytest.mark.parametrize("variant,kind", V.CASES)
def test_the_states_cover_what_the_variant_changes(oracle_mod, variant, kind):
    """The conditions that keep the device tests honest, on the reference alone:
      exclusion   : the f32 and the f64 oracle differ in their row counts in at most 2 % of the envs (keep's cap);
      impedance   : each of x < mid, mid <= x < 1 and x >= 1 (x = |pos| / width) holds >= 5 % of the contacts; the limit rows
                    of the cube's impedance variant hold >= 5 % in each of the first two (the Go2 states reach no limit);
      margin      : >= 5 % of the contacts of the Go2 families have dist > 0; on the cube >= 1 active limit per 10 envs has a
                    positive limit distance;
      friction    : each of the rules 0, 1, 2 is on >= 20 contacts whose two geoms differ in sliding and in torsional friction;
      equality    : |dif| > 1e-2 in at least half the envs;
      solref      : contacts on clamped (time constant < 2 dt) and on unclamped pairs; with refsafe off the k of the clamped pairs' rows (closed form, which the
                    oracle's aref matches) is (2 dt / time constant)^2 times the refsafe run's, the other rows' k the same;
      every case  : the f64 oracle's efc_force differs from the shipped model's on the same states by more than 1e-3 (per env,
                    relative as physics_support.rel) in at least half the envs."""
    c = case(oracle_mod, variant, kind)
    n = coverage(c, variant, kind)
    print(variant, kind, n)
    assert n["excluded"] <= 0.02 * V.N
    if variant in ("impedance", "combined"):
        for k in ("con_below_mid", "con_mid_to_1", "con_from_1"):
            assert n[k] >= 0.05 * n["contacts"], (k, n)
        if variant == "impedance" and kind == "cube":          # (no limit is ever active in the Go2 states)
            assert min(n["lim_below_mid"], n["lim_mid_to_1"]) >= 0.05 * n["limits"], n
    if variant in ("margin", "combined"):
        if kind == "cube":
            assert n["lim_dist_pos"] >= V.N / 10, n
        else:
            assert n["con_dist_pos"] >= 0.05 * n["contacts"], n
    if variant in ("friction_rule", "combined"):
        assert min(n["rule0"], n["rule1"], n["rule2"]) >= 20, n
    if variant in ("eq_poly", "combined") and kind in ("cube", "tshape"):
        assert n["eq_dif_big"] >= V.N / 2, n
    if variant in ("solref", "solref_refsafe_off", "combined"):
        assert n["con_clamped"] > 0 and n["con_unclamped"] > 0, n
    if variant == "solref_refsafe_off":
        safe = case(oracle_mod, "solref", kind)
        dt, seen = float(c["A"]["opt_timestep"][0]), 0
        for e in range(V.N):
            for w, v in zip(all_rows(c)[e][3], all_rows(safe)[e][3]):
                if w["type"] == "contact" and 0 < w["solref"][0] < 2 * dt:
                    seen += 1
                    assert abs(w["k"] / v["k"] - (2 * dt / w["solref"][0]) ** 2) <= 1e-12 and w["k"] > 1.5 * v["k"]
                else:
                    assert w["k"] == v["k"]
        assert seen > 0
    base = case(oracle_mod, None, kind)
    f = lambda cc: np.stack([r["efc_force"] for r in cc["ref"]["f64"]])
    far = int((S.rel(f(c), f(base)) > 1e-3).sum())
    print(variant, kind, "efc_force moved in %d of %d envs" % (far, V.N))
    assert far >= V.N / 2
