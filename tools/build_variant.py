"""Builds a variant of the library next to the default one: python tools/build_variant.py <tag> [--rev GITREV] [-Dflags ...]
-> rsr_mjx_amd/csrc/librsrmjx_<tag>.so (for tools/ab_bench.py).  --rev builds the sources of another commit with that commit's own
rsr_mjx_amd/build.py (from a git archive of the revision)."""
import io, os, subprocess, sys, tarfile, tempfile, shutil
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
tag = sys.argv[1]
args = sys.argv[2:]
rev = None
if "--rev" in args:
    i = args.index("--rev"); rev = args[i + 1]; args = args[:i] + args[i + 2:]
from rsr_mjx_amd import build as B
out = os.path.join(B.CSRC, f"librsrmjx_{tag}.so")
if rev is None:
    B.compile_lib(out, extra_flags=args)
else:
    tmp = tempfile.mkdtemp()
    try:
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", rev, "rsr_mjx_amd", "include"])
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        lib = os.path.join(tmp, "rsr_mjx_amd", "csrc", "lib.so")
        code = ("import sys; sys.path.insert(0, sys.argv[1]); from rsr_mjx_amd import build as B; "
                "B.compile_lib(sys.argv[2], extra_flags=sys.argv[3:])")
        subprocess.check_call([sys.executable, "-c", code, tmp, lib] + args, cwd=tmp)
        shutil.copy(lib, out)
    finally:
        shutil.rmtree(tmp)
print(out)
