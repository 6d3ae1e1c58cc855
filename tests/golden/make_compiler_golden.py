"""Compiles tests/golden/compiler_pusher.xml with rsr_mjx_amd.mjcf and writes tests/golden/compiler_pusher.npz (CompiledModel.save):
the stored output tests/test_mjcf.py::test_compiler_output_of_a_stored_model compares the compiler against.  Re-run only after
a deliberate change of the compiler, and check the new output against the analytic values that test also asserts."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rsr_mjx_amd.mjcf import compile_mjcf

golden = os.path.join(ROOT, "tests", "golden")
m = compile_mjcf(os.path.join(golden, "compiler_pusher.xml"))
m.save(os.path.join(golden, "compiler_pusher.npz"))
print(m.name, m.nq, m.nv, m.nu, m.nbody, m.ngeom, m.npair)
