"""Physics-level C ABI and Python surface (include/rsr_physics.h, rsr_mjx_amd/physics.py), host side only: what can be
checked without a device.  The kernels themselves are covered by tests/test_physics_gpu.py."""
import ctypes as C
import re

from api_support import header


def test_header_declares_the_physics_api():
    h = header()
    assert '#include "rsr_mjx.h"' in h
    for sig in ("int rsr_physics_create(rsr_batch* b, rsr_physics** out);",
                "void rsr_physics_destroy(rsr_physics* p);",
                "int rsr_physics_step(rsr_physics* p, const float* ctrl, int nsteps, void* hip_stream);",
                "int rsr_physics_forward(rsr_physics* p, void* hip_stream);",
                "int rsr_physics_forward_envs(rsr_physics* p, const int32_t* env_ids, int count, void* hip_stream);",
                "int rsr_physics_view(rsr_physics* p, int field, void** dev_ptr, int64_t shape[2], int64_t stride[2]);"):
        assert sig in h, sig
    enum = re.search(r"enum rsr_physics_field \{([^}]*)\}", h).group(1)
    names = [t.strip().split("=")[0].strip() for t in enum.split(",") if t.strip()]
    from rsr_mjx_amd import _lib
    assert names[:-1] == ["RSR_P_" + f.upper() for f in _lib.PHYS_FIELDS] and names[-1] == "RSR_P_COUNT"
    assert len(_lib.FIELDS) == 38          # the record is unchanged: the physics outputs live in a side buffer


def test_library_exports_and_argument_checks():
    from rsr_mjx_amd import _lib
    L = _lib.lib()
    h = header()
    assert set(re.findall(r"\b(rsr_physics_[a-z_]+)\s*\(", h)) == set(_lib.PHYS_SYMBOLS)
    for sym in _lib.PHYS_SYMBOLS:
        assert getattr(L, sym) is not None
    # argument checks come before any device work
    h = C.c_void_p()
    assert L.rsr_physics_create(None, C.byref(h)) == -1 and not h.value
    L.rsr_physics_destroy(None)
    assert L.rsr_physics_step(None, None, 1, None) == -1
    assert L.rsr_physics_forward(None, None) == -1
    assert L.rsr_physics_forward_envs(None, None, 1, None) == -1
    ptr, shape, stride = C.c_void_p(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    assert L.rsr_physics_view(None, 0, C.byref(ptr), shape, stride) == -1
    assert b"null" in L.rsr_last_error()


def test_physics_module_surface():
    from rsr_mjx_amd.physics import Physics
    for m in ("set_state", "forward", "step", "contacts"):
        assert callable(getattr(Physics, m))
