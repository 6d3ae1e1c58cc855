"""Dynamics terms of the physics layer (rsr_physics_set_jac_sites / rsr_physics_dynamics / rsr_physics_dynamics_view,
Physics.set_jac_sites / Physics.dynamics), host side only: the ABI and the Python surface.  The kernel is covered by
tests/test_dynamics_gpu.py."""
import ctypes as C
import inspect
import os
import re

from api_support import ROOT, header, refused, standin


def test_header_declares_the_dynamics_api():
    h = header()
    for sig in ("int rsr_physics_set_jac_sites(rsr_physics* p, const int32_t* site_ids, int nsite);",
                "int rsr_physics_dynamics(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream);",
                "int rsr_physics_dynamics_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);"):
        assert sig in h, sig
    enum = re.search(r"enum rsr_dynamics_field \{([^}]*)\}", h).group(1)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    from rsr_mjx_amd import _lib
    assert names == ["RSR_D_" + f.upper() for f in _lib.DYNAMICS_FIELDS] + ["RSR_D_COUNT"]
    assert "RSR_D_QM = 0" in enum
    nmax = int(re.search(r"#define RSR_MAX_JAC_SITES (\d+)", h).group(1))
    assert nmax >= 5 and nmax == _lib.MAX_JAC_SITES          # the Go2's IMU and four feet fit
    # the call is documented as describing the state after the integration
    assert "after the" in h[h.index("RSR_D_QM") - 1500:h.index("RSR_D_QM")]
    # the other enums are unchanged
    assert _lib.PHYS_FIELDS[-1] == "sensordata" and len(_lib.PHYS_FIELDS) == 7 and len(_lib.APPLIED_FIELDS) == 2


def test_library_exports_and_argument_checks():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    for sym in ("rsr_physics_set_jac_sites", "rsr_physics_dynamics", "rsr_physics_dynamics_view"):
        assert sym in _lib.PHYS_SYMBOLS and getattr(L, sym) is not None
        assert getattr(L, sym).argtypes is not None
    # null handle, refused before any device work
    ids = (C.c_int32 * 2)(0, 1)
    for table, k in ((None, 0), (ids, 2), (ids, _lib.MAX_JAC_SITES + 1), (ids, -1)):
        assert L.rsr_physics_set_jac_sites(None, table, k) == -1
        assert b"null" in L.rsr_last_error()
    assert L.rsr_physics_dynamics(None, None, 0, None) == -1
    assert b"null" in L.rsr_last_error()
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    for fid in (0, len(_lib.DYNAMICS_FIELDS) - 1, len(_lib.DYNAMICS_FIELDS), -1):
        assert L.rsr_physics_dynamics_view(None, fid, C.byref(ptr), shape, stride) == -1
    assert not ptr.value


def test_argument_checks_come_before_device_work():
    """Bad site ids, nsite > RSR_MAX_JAC_SITES, env_ids with count < 1 and unknown view ids: RSR_ERR_ARG on a real handle, with
    the check ahead of every device call and of the table update (checked by source order, as the handle needs a device)."""
    src = open(os.path.join(ROOT, "rsr_mjx_amd", "csrc", "physics", "rsr_physics.hip")).read()

    def body(name):
        b = src[src.index(name + "("):]
        return b[:b.index("\n}\n")]
    dev = ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset", "hipMemcpy", "zeroed_once", "dyn_buffers", "launch(")
    first_dev = lambda b: min(b.index(k) for k in dev if k in b)
    sites = body("int rsr_physics_set_jac_sites")
    for check in ("!p)", "nsite > RSR_MAX_JAC_SITES", "site_ids[k] >= p->b->model->dims.nsite", "site_ids[k] < 0"):
        assert sites.index(check) < first_dev(sites), check
    assert sites.count("RSR_ERR_ARG") == 3 and first_dev(sites) < sites.index("p->njac = nsite")
    dyn = body("int rsr_physics_dynamics")
    assert dyn.index("!p)") < first_dev(dyn) and dyn.index("env_count(") < first_dev(dyn)
    assert "count < 1" in body("static int env_count") and not any(k in body("static int env_count") for k in dev)
    # the buffer and the site table come together, through the one allocation helper: a failure of the second undoes the first
    bufs = body("static int dyn_buffers")
    assert "zeroed_once(p, &p->dyn, " in bufs and "zeroed_once(p, &p->jac_sites, " in bufs
    assert "if (rc && !had) { (void)hipFree(p->dyn); p->dyn = nullptr; }" in bufs
    assert src.count("&p->dyn,") == 1 and src.count("&p->jac_sites,") == 1
    view = body("int rsr_physics_dynamics_view")
    assert view.index("default: return fail(RSR_ERR_ARG") < first_dev(view)
    for entry in (sites, dyn, view):
        assert "dyn_buffers(" in entry
    # the buffer goes with the handle
    destroy = body("void rsr_physics_destroy")
    assert "hipFree(p->dyn)" in destroy and "hipFree(p->jac_sites)" in destroy


def test_the_dynamics_op_is_an_ordinary_op():
    """The op is a member of the physics op enum and its arguments a field of the physics launch struct, like every other physics
    op's (all nine are checked here); nothing is carried through another op's arguments.  The enum, the struct, the kernel, its
    arguments' type and its buffer layout are in the physics layer: no source directly under csrc/ names a physics op."""
    import re
    csrc = os.path.join(ROOT, "rsr_mjx_amd", "csrc")
    for d in (csrc, os.path.join(csrc, "physics")):
        for f in os.listdir(d):
            if f.endswith((".hip", ".hpp")):
                text = open(os.path.join(d, f)).read()
                assert "pack_dyn" not in text and "reinterpret_cast<const int4" not in text, f
                if d == csrc:
                    assert "dynamics_kernel" not in text and "struct DynArgs" not in text, f
    launch = open(os.path.join(csrc, "rsr_launch.hpp")).read()
    phys = open(os.path.join(csrc, "physics", "rsr_physics.hpp")).read()
    kernels = open(os.path.join(csrc, "physics", "rsr_physics_kernels.hpp")).read()
    lp = kernels[kernels.index("int launch_physics("):]
    assert re.search(r"\bPhysLaunch ph;", re.search(r"struct Launch \{(.*?)\};", launch, re.S).group(1))
    enum = re.sub(r"//.*", "", re.search(r"enum PhysOp \{(.*?)\};", phys, re.S).group(1))
    fields = re.search(r"struct PhysLaunch \{(.*?)\};", phys, re.S).group(1)
    # op: the field it owns (forward and step share the one struct physics_kernel takes), and every field its case may read
    ops = {"FORWARD": ("PhysArgs p", "p ap"), "STEP": ("PhysArgs p", "p ap"), "ROLLOUT": ("RollArgs r", "p r ap"),
           "DYNAMICS": ("DynArgs d", "d"), "CONSTRAINT": ("ConArgs c", "c ap"), "TRANSITION": ("FdArgs fd", "p fd ap"),
           "INVERSE": ("InvArgs inv", "inv"), "SAMPLE": ("int K", "p r K ap"), "SWEEP": ("SweepArgs sw", "p r sw ap")}
    assert sorted(re.findall(r"\bOP_PHYS_(\w+)", enum)) == sorted(ops) and "switch (op)" in lp
    assert len(re.findall(r"\bcase \w+:", lp)) == len(ops)                   # one case per op, nothing else
    for op, (own, reads) in ops.items():
        assert re.search(rf"\b{own};", fields), op
        assert lp.count(f"case OP_PHYS_{op}:") == 1, op
        case = re.search(rf"case OP_PHYS_{op}:(.*?)\n\s*(?:case |default:)", lp, re.S).group(1)
        assert set(re.findall(r"\bph\.(\w+)", case)) == set(reads.split()), op
        assert not re.search(r"\bx\.", case.replace("x.ph", "")), op         # (and nothing of the Launch but through the lambda)
    # the two enums share the entries' int: the physics ops start above the env ops, stated next to both and checked
    env_ops = re.findall(r"\bOP_\w+", re.sub(r"//.*", "", re.search(r"enum Op \{(.*?)\};", launch, re.S).group(1)))
    assert env_ops == ["OP_RESET", "OP_STEP", "OP_STEP_OCCUPANCY"]
    assert int(re.search(r"OP_PHYS_FORWARD = (\d+),", enum).group(1)) > len(env_ops) and enum.count("=") == 1
    assert "static_assert((int)OP_STEP_OCCUPANCY < (int)OP_PHYS_FORWARD," in kernels
    # no source directly under csrc/ names an individual physics op; each unit sends what it does not handle itself to
    # launch_physics, which launches nothing for an op it does not know
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".hpp")):
            assert "OP_PHYS_" not in open(os.path.join(csrc, f)).read(), f
    for unit in ("rsr_cube.hip", "rsr_tshape.hip", "rsr_go2.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert text.count("default: return launch_physics<") == 1 and "default: return -1;" not in text, unit
    assert lp.rstrip().endswith("default: return -1;\n  }\n}\n\n}  // namespace rsr")
    assert "struct DynArgs" in phys and "struct DynLayout" in phys
    kern = open(os.path.join(csrc, "physics", "rsr_dynamics.hpp")).read()
    assert "void dynamics_kernel(" in kern
    for stage in ("kinematics<C>(", "com_crb_mass<C>(", "smooth_forces<C>("):
        assert stage in kern, stage
    for absent in ("collision<C>(", "make_constraint<C>(", "solve<C>(", "forward<C>("):
        assert absent not in kern, absent


def test_physics_module_surface(monkeypatch):
    from rsr_mjx_amd.physics import Physics
    for m in ("set_jac_sites", "dynamics"):
        assert callable(getattr(Physics, m))
    assert list(inspect.signature(Physics.dynamics).parameters) == ["self", "env_ids"]
    assert list(inspect.signature(Physics.set_jac_sites).parameters) == ["self", "sites"]
    for view in ("qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "jacp", "jacr", "jac_site_xpos"):
        assert isinstance(getattr(Physics, view), property), view
    refused(monkeypatch, standin().set_jac_sites, [(dict(sites=[0, 1, 2, 3] * 3), "set_jac_sites expects at most 8 sites, got 12"),
                                                   (dict(sites=["tip", "nose"]), "set_jac_sites: no site 'nose'"),
                                                   (dict(sites=[0, 4]), r"set_jac_sites: site ids must lie in \[0, 4\), got 4")])
