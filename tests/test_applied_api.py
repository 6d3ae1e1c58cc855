"""Applied forces of the physics layer (rsr_physics_set_applied / rsr_physics_applied_view, Physics.set_applied), host side only:
the ABI and the Python surface.  The kernels are covered by tests/test_applied_gpu.py."""
import ctypes as C
import os
import re

from api_support import ROOT, header


def test_header_declares_the_applied_api():
    h = header()
    for sig in ("int rsr_physics_set_applied(rsr_physics* p, int on);",
                "int rsr_physics_applied_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);"):
        assert sig in h, sig
    enum = re.search(r"enum rsr_applied_field \{([^}]*)\}", h).group(1)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    from rsr_mjx_amd import _lib
    assert names == ["RSR_A_" + f.upper() for f in _lib.APPLIED_FIELDS] + ["RSR_A_COUNT"]
    assert "RSR_A_XFRC_APPLIED = 0" in enum
    assert "data.xfrc_applied is zero" not in h
    # the physics field enum is unchanged: sensordata stays last
    assert _lib.PHYS_FIELDS[-1] == "sensordata" and len(_lib.PHYS_FIELDS) == 7


def test_library_exports_and_argument_checks():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", header())) == set(_lib.PHYS_SYMBOLS)
    for sym in ("rsr_physics_set_applied", "rsr_physics_applied_view"):
        assert sym in _lib.PHYS_SYMBOLS and getattr(L, sym) is not None
        assert getattr(L, sym).argtypes is not None
    # null handle, refused before any device work
    for on in (0, 1):
        assert L.rsr_physics_set_applied(None, on) == -1
        assert b"null" in L.rsr_last_error()
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    for fid in (0, 1, 2, -1):
        assert L.rsr_physics_applied_view(None, fid, C.byref(ptr), shape, stride) == -1
    assert not ptr.value


def test_set_applied_checks_on_and_field_before_device_work():
    """`on` outside {0, 1} and unknown view ids: RSR_ERR_ARG on a real handle, with the argument check ahead of device calls
    (checked by source order, as the handle needs a device)."""
    src = open(os.path.join(ROOT, "rsr_mjx_amd", "csrc", "physics", "rsr_physics.hip")).read()
    body = src[src.index("int rsr_physics_set_applied("):]
    body = body[:body.index("\n}\n")]
    first_dev = min(body.index(k) for k in ("hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipMemset"))
    assert body.index("on != 0 && on != 1") < first_dev
    assert body.index("!p)") < first_dev
    view = src[src.index("int rsr_physics_applied_view("):]
    view = view[:view.index("\n}\n")]
    assert "default: return fail(RSR_ERR_ARG" in view and "!p->applied" in view


def test_physics_module_surface():
    from rsr_mjx_amd.physics import Physics
    for m in ("set_applied", "clear_applied"):
        assert callable(getattr(Physics, m))
    import inspect
    assert list(inspect.signature(Physics.set_applied).parameters) == ["self", "xfrc", "qfrc", "env_ids"]
    src = inspect.getsource(Physics.__init__)
    assert "self.xfrc_applied = None" in src and "self.qfrc_applied = None" in src
