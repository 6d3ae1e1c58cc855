"""C-ABI library: loads, exports every symbol include/rsr_mjx.h declares, host-side entry points work without
a GPU, and compute entry points fail loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, make_blob


@pytest.fixture(scope="module")
def lib():
    from rsr_mjx_amd import _lib, build
    build.build()
    return _lib.lib()


def test_header_symbols_are_exported(lib):
    from rsr_mjx_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsr_mjx.h")).read()
    declared = set(re.findall(r"\b(rsr_[a-z_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for s in declared:
        assert getattr(lib, s) is not None


def test_model_create_and_dims_on_host(lib, cube_model):
    from rsr_mjx_amd import _lib
    blob = make_blob(cube_model, episode_length=1200, auto_reset=True)
    h = C.c_void_p()
    _lib.check(lib.rsr_model_create(C.create_string_buffer(blob, len(blob)), len(blob), C.byref(h)))
    d = _lib.Dims()
    _lib.check(lib.rsr_model_dims(h, C.byref(d)))
    assert (d.nq, d.nv, d.nu, d.nbody, d.npair, d.obs_dim, d.n_frames, d.episode_length) == (22, 20, 5, 14, 45, 23, 4, 1200)
    assert d.rec_floats % 16 == 0 and d.rec_floats >= 2 * (22 + 20 + 5 + 20 + 1 + 42 + 3) + 2 * 23
    assert d.ncon_max >= 16 and d.nefc_max == 17 + 6 * d.ncon_max and 0 < d.lds_bytes <= 64 * 1024
    lib.rsr_model_destroy(h)


def test_errors_are_reported_not_thrown(lib, cube_model):
    h = C.c_void_p()
    assert lib.rsr_model_create(b"junkjunkjunkjunkjunkjunkjunkjunkjunk", 36, C.byref(h)) == -1
    assert b"RSRM" in lib.rsr_last_error()
    # a model whose dims have no compiled kernel
    from rsr_mjx_amd.model import model_fields, pack_blob
    from rsr_mjx_amd.envs.config import cube_env_fields
    f = model_fields(cube_model)
    f.update(cube_env_fields(cube_model))
    f["dims"] = f["dims"].copy(); f["dims"][1] = 19
    blob = pack_blob(f)
    assert lib.rsr_model_create(C.create_string_buffer(blob, len(blob)), len(blob), C.byref(h)) == -2
    assert lib.rsr_step(None, None, None) == -1
    assert lib.rsr_batch_check(None, None, None) == -1 and lib.rsr_batch_set_fault_injection(None, 0, -1) == -1


def test_no_cpu_fallback(lib, cube_model):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path needs a GPU-less host")
    from rsr_mjx_amd import _lib
    blob = make_blob(cube_model)
    h, b = C.c_void_p(), C.c_void_p()
    _lib.check(lib.rsr_model_create(C.create_string_buffer(blob, len(blob)), len(blob), C.byref(h)))
    rc = lib.rsr_batch_create(h, 8, 0, None, C.byref(b))
    assert rc == -3 and b"no HIP device" in lib.rsr_last_error()
    lib.rsr_model_destroy(h)
    from rsr_mjx_amd.envs.airbot import AirbotPlayBase
    with pytest.raises(RuntimeError):
        AirbotPlayBase(device="cpu").batched(4)


def test_product_does_not_import_the_oracle():
    """The shipped package must not import, call or link anything under oracle/."""
    pkg = os.path.join(ROOT, "rsr_mjx_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                text = open(os.path.join(dirpath, fn), errors="ignore").read()
                assert "from oracle" not in text and "import oracle" not in text and "liboracle" not in text, fn
                assert "rsr_oracle.c" not in text, fn


def test_passive_forces_that_are_not_built_are_refused(cube_model):
    """model_fields refuses a model with a joint spring (jnt_stiffness, in every asset and all zero) or with gravity compensation
    (body_gravcomp: the compiler refuses the attribute itself and emits no such array, a model loaded from elsewhere may carry one) and names the field: nothing reads either, so such a model would be
    simulated without them.  All-zero arrays pass."""
    import copy
    import numpy as np
    from rsr_mjx_amd.model import model_fields
    assert "jnt_stiffness" in cube_model.arrays and not np.any(cube_model.arrays["jnt_stiffness"])
    for field in ("jnt_stiffness", "body_gravcomp"):
        m = copy.copy(cube_model)
        m.arrays = dict(cube_model.arrays)
        n = cube_model.njnt if field == "jnt_stiffness" else cube_model.nbody
        m.arrays[field] = np.zeros(n)
        model_fields(m)
        stiff = np.zeros(n)
        stiff[2] = 5.0
        m.arrays[field] = stiff
        with pytest.raises(NotImplementedError, match=field):
            model_fields(m)
    model_fields(cube_model)


def test_velocity_gains_under_implicitfast_are_refused(cube_model, go2_model, tmp_path):
    """implicitfast here solves (M + h D) alone, without the actuators' velocity derivative that MuJoCo's implicitfast adds, so a
    model with biasprm[:, 2] or gainprm[:, 2] != 0 under implicitfast is refused, by field name; the same model under Euler, and
    the per-env leaves' check on batched arrays, pass or refuse alike.  And the compiler refuses a body with gravcomp."""
    import copy
    import numpy as np
    from rsr_mjx_amd import mjcf
    from rsr_mjx_amd.model import check_velocity_gains, model_fields
    assert int(cube_model.arrays["opt_integrator"][0]) == 3 and int(go2_model.arrays["opt_integrator"][0]) == 0
    for field in ("actuator_biasprm", "actuator_gainprm"):
        for base, refused in ((cube_model, True), (go2_model, False)):
            m = copy.copy(base)
            m.arrays = dict(base.arrays)
            a = np.array(base.arrays[field], dtype=np.float64)
            a[1, 2] = -0.5
            m.arrays[field] = a
            if refused:
                with pytest.raises(NotImplementedError, match=field):
                    model_fields(m)
                m.arrays["opt_integrator"] = np.array([0], np.int32)
            model_fields(m)
    leaf = np.zeros((4, 5, 3), np.float32)
    check_velocity_gains(3, leaf, leaf)
    check_velocity_gains(3, None, None)
    leaf[3, 2, 2] = 1.0
    check_velocity_gains(0, leaf, leaf)
    with pytest.raises(NotImplementedError, match="actuator_biasprm"):
        check_velocity_gains(3, None, leaf)
    xml = open(os.path.join(ROOT, "tests", "golden", "compiler_pusher.xml")).read()
    assert "gravcomp" not in xml and "<body " in xml
    path = tmp_path / "gravcomp.xml"
    path.write_text(xml.replace("<body ", '<body gravcomp="1" ', 1))
    with pytest.raises(NotImplementedError, match="gravcomp"):
        mjcf.compile_mjcf(str(path))
    path.write_text(xml.replace("<body ", '<body gravcomp="0" ', 1))
    mjcf.compile_mjcf(str(path))


def test_malformed_blobs_are_refused(lib, cube_model):
    """rsr_model_create validates the blob's directory before reading through it: truncated blobs, entries pointing outside
    the blob, absurd entry counts and missing fields all return RSR_ERR_ARG (-1) with a message, never a crash."""
    import struct
    blob = make_blob(cube_model, episode_length=1200, auto_reset=True)
    h = C.c_void_p()
    ok = lambda b: lib.rsr_model_create(C.create_string_buffer(bytes(b), len(b)), len(b), C.byref(h))
    assert ok(blob) == 0
    lib.rsr_model_destroy(h)
    nent = struct.unpack_from("<i", blob, 8)[0]
    assert nent > 50
    # (1) cut in the middle of the entry table / of the data
    assert ok(blob[:16 + 56 * 3 + 10]) == -1
    assert ok(blob[:len(blob) // 2]) == -1
    # (2) entry count far larger than the blob
    b = bytearray(blob); struct.pack_into("<i", b, 8, 10 ** 8)
    assert ok(b) == -1 and b"entry table" in lib.rsr_last_error()
    # (3) one entry's offset / count pointing past the end
    for field_off, val in ((48, len(blob)), (44, 10 ** 8), (48, -4)):       # blob_entry: name[40], dtype, count, offset, reserved
        b = bytearray(blob); struct.pack_into("<i", b, 16 + 56 * 5 + field_off, val)
        assert ok(b) == -1, (field_off, val)
    # (4) a required field renamed away
    b = bytearray(blob)
    idx = bytes(b).find(b"opt_integrator\0")
    assert idx > 0
    b[idx:idx + 3] = b"xxx"
    assert ok(b) == -1 and b"opt_integrator" in lib.rsr_last_error()
    # (5) a name without terminator
    b = bytearray(blob); b[16:16 + 40] = b"a" * 40
    assert ok(b) == -1


def test_go2_model_create_checks_the_block_arrow_structure(lib):
    """The Go2 kernels factor M and H in block-arrow form (trunk of 6 dofs, legs of 3 that couple only through the trunk):
    rsr_model_create accepts the shipped model and refuses one whose body chains or contact pairs tie two legs together."""
    import numpy as np
    from rsr_mjx_amd.envs import config, go2
    from rsr_mjx_amd.model import model_fields, pack_blob
    env = go2.load("Go2JoystickFlatTerrain")
    f = model_fields(env.sys)
    f.update(config.go2_env_fields(env.sys, env._config, 1000, True))
    h = C.c_void_p()
    create = lambda fields: (lambda b: lib.rsr_model_create(C.create_string_buffer(b, len(b)), len(b), C.byref(h)))(pack_blob(fields))
    assert create(f) == 0
    lib.rsr_model_destroy(h)
    bad = dict(f); m1 = np.array(f["pair_mask1"]).copy()
    m1[0] = int(m1[0]) | (7 << 6) | (7 << 9)                     # a contact pair whose chain holds the dofs of two legs
    bad["pair_mask1"] = m1
    assert create(bad) == -2 and b"legs" in lib.rsr_last_error()
    bad = dict(f); bm = np.array(f["body_dofmask"]).copy()
    bm[-1] = int(bm[-1]) | (7 << 6)                               # the last calf's chain also runs through the first leg
    bad["body_dofmask"] = bm
    assert create(bad) == -2


def test_airbot_model_create_checks_the_tree_ranges(lib, cube_model):
    """The Airbot kernels factor one kinematic tree per DPP row (arm | target | cube over fixed dof ranges): a model whose body
    chain straddles two ranges is refused."""
    import numpy as np
    from rsr_mjx_amd.envs import config
    from rsr_mjx_amd.model import model_fields, pack_blob
    f = model_fields(cube_model); f.update(config.cube_env_fields(cube_model))
    h = C.c_void_p()
    create = lambda fields: (lambda b: lib.rsr_model_create(C.create_string_buffer(b, len(b)), len(b), C.byref(h)))(pack_blob(fields))
    assert create(f) == 0
    lib.rsr_model_destroy(h)
    bad = dict(f); bm = np.array(f["body_dofmask"]).copy()
    bm[-1] = int(bm[-1]) | 1                                      # the last body's chain also runs through the arm's first dof
    bad["body_dofmask"] = bm
    assert create(bad) == -2 and b"trees" in lib.rsr_last_error()


# ---------------------------------------------------------------- rsr_model_create: every refusal, and what it accepts
# rsr_dims of every shipped model (episode_length 1000), field for field: nq nv nu nbody njnt ngeom nsite neq npair obs_dim nmetrics
# n_frames episode_length env_kind rec_floats ncon_max nefc_max lds_bytes
SHIPPED_DIMS = {
    "cube": (22, 20, 5, 14, 10, 23, 1, 1, 45, 23, 3, 4, 1000, 0, 320, 24, 161, 16384),
    "sf": (22, 20, 5, 14, 10, 23, 1, 1, 45, 23, 3, 4, 1000, 2, 320, 24, 161, 16384),
    "tshape": (15, 14, 5, 14, 9, 25, 3, 1, 60, 16, 5, 4, 1000, 1, 288, 32, 209, 18944),
    "go2_flat": (19, 18, 12, 14, 13, 39, 6, 0, 4, 48, 22, 5, 1000, 3, 832, 4, 40, 10032),
    "go2_rough": (19, 18, 12, 14, 13, 39, 6, 0, 4, 48, 22, 5, 1000, 3, 832, 4, 40, 10032),
    "handstand": (19, 18, 12, 14, 13, 44, 6, 0, 30, 45, 11, 5, 1000, 4, 800, 12, 72, 13600),
}
PAIR_HFIELD_SPHERE = 3          # rsr_device.hpp


@pytest.fixture(scope="module")
def shipped(cube_model, sf_model, tshape_model):
    """The blob fields of every shipped model, as the env definitions pack them (config.*_env_fields)."""
    from rsr_mjx_amd.envs import config, go2
    from rsr_mjx_amd.model import model_fields
    out = {}
    for name, m, fn in (("cube", cube_model, config.cube_env_fields), ("sf", sf_model, config.sf_env_fields),
                        ("tshape", tshape_model, config.tshape_env_fields)):
        out[name] = dict(model_fields(m)); out[name].update(fn(m, 1000, True))
    for name, env_name in (("go2_flat", "Go2JoystickFlatTerrain"), ("go2_rough", "Go2JoystickRoughTerrain"), ("handstand", "Go2Handstand")):
        env = go2.load(env_name)
        out[name] = dict(model_fields(env.sys)); out[name].update(env._fields_fn(env.sys, 1000, True))
    return out


def _create(lib, fields):
    """(return code, message) of rsr_model_create on the packed fields; a created model is destroyed."""
    from rsr_mjx_amd.model import pack_blob
    blob, h = pack_blob(fields), C.c_void_p()
    rc = lib.rsr_model_create(C.create_string_buffer(blob, len(blob)), len(blob), C.byref(h))
    if rc == 0:
        lib.rsr_model_destroy(h)
        return 0, b""
    return rc, lib.rsr_last_error()


def _with(fields, **changes):
    """A copy of `fields` with the given entries replaced: name=array, or name=(index, value) for one element."""
    import numpy as np
    out = dict(fields)
    for name, v in changes.items():
        if isinstance(v, tuple):
            a = np.array(fields[name]).copy(); a.reshape(-1)[v[0]] = v[1]; v = a
        out[name] = v
    return out


@pytest.mark.parametrize("name", sorted(SHIPPED_DIMS))
def test_model_create_accepts_every_shipped_model_and_reports_its_dims(lib, shipped, name):
    from rsr_mjx_amd import _lib
    from rsr_mjx_amd.model import pack_blob
    blob, h = pack_blob(shipped[name]), C.c_void_p()
    _lib.check(lib.rsr_model_create(C.create_string_buffer(blob, len(blob)), len(blob), C.byref(h)))
    d = _lib.Dims()
    _lib.check(lib.rsr_model_dims(h, C.byref(d)))
    lib.rsr_model_destroy(h)
    got = tuple(getattr(d, n) for n, _ in _lib.Dims._fields_)
    print(name, got)
    assert got == SHIPPED_DIMS[name]


def _refusals(shipped):
    """(id, fields, return code, distinctive part of the message), one per refusal of rsr_model_create after the directory checks."""
    import numpy as np
    cube, tshape, flat, rough, hand = (shipped[k] for k in ("cube", "tshape", "go2_flat", "go2_rough", "handstand"))
    legs = lambda f, name, i: (i, int(np.asarray(f[name]).reshape(-1)[i]) | (7 << 6) | (7 << 9))       # the dofs of two legs
    rough_foot = int(np.asarray(rough["pair_geom2"])[0])
    wide = np.array(rough["geom_size"], dtype=np.float64).copy(); wide.reshape(-1, 3)[rough_foot, 0] = 0.2   # cell: 20 m / 255
    return [
        ("dims_short", _with(cube, dims=np.asarray(cube["dims"])[:8]), -1, b"lacks dims/env_int"),
        ("counts2_short", _with(cube, counts2=np.asarray(cube["counts2"])[:3]), -1, b"counts2 / opt_gravity too short"),
        ("no_kernel_nv", _with(cube, dims=(1, 19)), -2, b"no compiled kernel"),
        ("no_kernel_env_kind", _with(cube, env_int=(0, 9)), -2, b"no compiled kernel"),
        ("no_kernel_cube_dims_as_tshape", _with(cube, env_int=(0, 1)), -2, b"no compiled kernel"),
        ("no_kernel_nfric", _with(flat, counts2=(0, 11)), -2, b"no compiled kernel"),
        ("no_kernel_obs_dim", _with(hand, env_int=(4, 48)), -2, b"no compiled kernel"),
        ("two_joints_per_body", _with(cube, counts2=(3, 2)), -2, b"more than one joint"),
        ("slots_short", _with(cube, geom_slot_ids=np.asarray(cube["geom_slot_ids"])[:-1]), -2, b"geom_slot_ids"),
        ("slots_permuted", _with(cube, geom_slot_ids=np.asarray(cube["geom_slot_ids"])[::-1].copy()), -2, b"geom_slot_ids"),
        ("slots_out_of_range", _with(tshape, geom_slot_ids=(3, 25)), -2, b"geom_slot_ids"),
        ("slots_count_handstand", _with(hand, geom_slot_ids=np.asarray(hand["geom_slot_ids"])[:5]), -2, b"geom_slot_ids"),
        ("slots_miss_pair_geom", _with(flat, geom_slot_ids=(1, 13)), -2, b"miss a pair geom"),
        ("trees_body_cube", _with(cube, body_dofmask=(-1, int(np.asarray(cube["body_dofmask"])[-1]) | 1)), -2, b"separate kinematic trees"),
        ("trees_body_tshape", _with(tshape, body_dofmask=(-1, int(np.asarray(tshape["body_dofmask"])[-1]) | 1)), -2, b"separate kinematic trees"),
        ("arrow_pair_go2", _with(flat, pair_mask1=legs(flat, "pair_mask1", 0)), -2, b"legs of 3 dofs"),
        ("arrow_body_go2", _with(rough, body_dofmask=legs(rough, "body_dofmask", -1)), -2, b"legs of 3 dofs"),
        ("arrow_body_handstand", _with(hand, body_dofmask=legs(hand, "body_dofmask", -1)), -2, b"legs of 3 dofs"),
        ("condim_3_on_cube", _with(cube, pair_condim=(7, 3)), -2, b"condim the kernel is built for"),
        ("condim_3_on_tshape", _with(tshape, pair_condim=(0, 3)), -2, b"condim the kernel is built for"),
        ("condim_4_on_go2", _with(flat, pair_condim=(2, 4)), -2, b"condim the kernel is built for"),
        ("condim_4_on_handstand", _with(hand, pair_condim=(29, 4)), -2, b"condim the kernel is built for"),
        ("equality_inactive", _with(cube, eq_active0=(0, 0)), -2, b"inactive equality"),
        ("integrator", _with(cube, opt_integrator=(0, 7)), -2, b"rsr_model_create: integrator"),
        ("integrator_go2", _with(flat, opt_integrator=(0, 7)), -2, b"rsr_model_create: integrator"),
        ("iso_pair", _with(cube, pair_mask1=(0, 1 | (1 << 8))), -2, b"target body's dofs"),
        ("hfield_pair_on_cube", _with(cube, pair_kind=(0, PAIR_HFIELD_SPHERE)), -2, b"height-field pairs need the Go2 kernels"),
        ("hfield_pair_on_handstand", _with(hand, pair_kind=(8, PAIR_HFIELD_SPHERE)), -2, b"height-field pairs need the Go2 kernels"),
        ("hfield_without_field", _with(flat, pair_kind=(0, PAIR_HFIELD_SPHERE)), -2, b"height-field pairs need the Go2 kernels"),
        ("hfield_two_rows", _with(rough, hfield_nrow=(0, 2)), -2, b"height-field pairs need the Go2 kernels"),
        ("hfield_wide_sphere", _with(rough, geom_size=wide), -2, b"height-field pairs need the Go2 kernels"),
        # two defects at once: the checks run in a fixed order and the first one to fail speaks
        ("order_trees_before_condim", _with(cube, pair_condim=(0, 3), body_dofmask=(-1, int(np.asarray(cube["body_dofmask"])[-1]) | 1)), -2, b"separate kinematic trees"),
        ("order_slots_before_arrow", _with(flat, geom_slot_ids=(1, 13), pair_mask1=legs(flat, "pair_mask1", 0)), -2, b"miss a pair geom"),
        ("order_condim_before_integrator", _with(flat, pair_condim=(2, 4), opt_integrator=(0, 7)), -2, b"condim the kernel is built for"),
        ("order_equality_before_iso", _with(cube, eq_active0=(0, 0), pair_mask1=(0, 1 | (1 << 8))), -2, b"inactive equality"),
        ("order_iso_before_hfield", _with(cube, pair_mask1=(0, 1 | (1 << 8)), pair_kind=(0, PAIR_HFIELD_SPHERE)), -2, b"target body's dofs"),
    ]


REFUSAL_IDS = ["dims_short", "counts2_short", "no_kernel_nv", "no_kernel_env_kind", "no_kernel_cube_dims_as_tshape", "no_kernel_nfric",
               "no_kernel_obs_dim", "two_joints_per_body", "slots_short", "slots_permuted", "slots_out_of_range", "slots_count_handstand",
               "slots_miss_pair_geom", "trees_body_cube", "trees_body_tshape", "arrow_pair_go2", "arrow_body_go2", "arrow_body_handstand",
               "condim_3_on_cube", "condim_3_on_tshape", "condim_4_on_go2", "condim_4_on_handstand", "equality_inactive", "integrator",
               "integrator_go2", "iso_pair", "hfield_pair_on_cube", "hfield_pair_on_handstand", "hfield_without_field", "hfield_two_rows",
               "hfield_wide_sphere", "order_trees_before_condim", "order_slots_before_arrow", "order_condim_before_integrator",
               "order_equality_before_iso", "order_iso_before_hfield"]


@pytest.mark.parametrize("case", REFUSAL_IDS)
def test_model_create_refusals(lib, shipped, case):
    """Every refusal of rsr_model_create that a packed blob can reach on a host without a GPU: the return code and a distinctive
    part of the message.  The `order_*` cases carry two defects and pin which check speaks first."""
    table = {c[0]: c for c in _refusals(shipped)}
    assert sorted(table) == sorted(REFUSAL_IDS)
    _, fields, want_rc, want_msg = table[case]
    rc, msg = _create(lib, fields)
    print(case, rc, msg.decode())
    assert rc == want_rc and want_msg in msg, (rc, msg)
