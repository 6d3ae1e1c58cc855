"""Compares the gfx950 device code of two builds of the library, kernel by kernel: python tools/kernel_diff.py A.so B.so [--rename REGEX=REPLACEMENT]...
Extracts the code objects of each (llvm-objdump --offloading), disassembles them and reads their kernel metadata notes
(VGPR / SGPR / scratch / LDS / kernarg sizes); per kernel symbol the instructions (addresses, symbol offsets and the zero padding
between kernels stripped; branch targets are relative) and the metadata must be equal.  Exit status 0: same symbols, every kernel identical.  No GPU needed.
With --rename the kernels are paired by their demangled names after every re.sub(REGEX, REPLACEMENT) in turn, on both sides: a kernel that
changed its name or its template arguments between the builds is compared with the one it replaces, and every such pair that is
identical is listed.  Two kernels of a build that come to the same name are an error."""
import argparse, glob, os, re, shutil, subprocess, tempfile

BIN = "/opt/rocm/llvm/bin"
tool = lambda n: shutil.which(n) or os.path.join(BIN, n)


def kernels(lib):
    """{kernel symbol: (instruction lines, metadata lines)} over every gfx950 code object in `lib`"""
    tmp = tempfile.mkdtemp()
    try:
        so = shutil.copy(lib, tmp)
        subprocess.check_call([tool("llvm-objdump"), "--offloading", os.path.basename(so)], cwd=tmp, stdout=subprocess.DEVNULL)
        out = {}
        for co in sorted(glob.glob(so + ".*gfx950*")):
            dis = subprocess.check_output([tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
            name, body = None, {}
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1); body[name] = []
                elif name and line.strip() and line.strip() != "...":             # ("...": zero padding up to the next kernel)
                    ins = re.sub(r"\s*//.*$", "", line)                               # the address comment
                    body[name].append(re.sub(r"<[^>]*>", "<>", ins).strip())      # symbol+offset of a branch target
            for ins in body.values():           # a single zero dword of padding disassembles as this instruction
                while ins and ins[-1] == "v_cndmask_b32_e32 v0, s0, v0, vcc":
                    ins.pop()
            notes = subprocess.check_output([tool("llvm-readelf"), "--notes", co], text=True)
            for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                sym = re.search(r"\.symbol:\s+'?([^\s']+?)\.kd'?\s", blk + "\n").group(1)
                meta = sorted(l.strip() for l in blk.splitlines() if re.match(r"\s*\.(sgpr|vgpr)_(count|spill_count)|\s*\.(group|private)_segment_fixed_size|\s*\.kernarg_segment_size|\s*\.wavefront_size|\s*\.max_flat_workgroup_size|\s*\.uses_dynamic_stack", l))
                out[sym] = (body[sym], meta)
        return out
    finally:
        shutil.rmtree(tmp)


def renamed(ks, renames):
    """`ks` keyed by demangled name, each `renames` pair applied in turn; and the names a pair changed"""
    syms = sorted(ks)
    names = subprocess.run([shutil.which("c++filt") or tool("llvm-cxxfilt")], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    out, moved = {}, set()
    for sym, was in zip(syms, names):
        name = was
        for pat, rep in renames:
            name = re.sub(pat, rep, name)
        if name in out:
            raise SystemExit(f"two kernels of one build are named {name}")
        out[name] = ks[sym]
        if name != was:
            moved.add(name)
    return out, moved


ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument("libs", nargs=2, metavar="LIB.so")
ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT", help="re.sub on the demangled kernel names of both builds before they are paired")
args = ap.parse_args()
a, b = kernels(args.libs[0]), kernels(args.libs[1])
moved = set()
if args.rename:
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    (a, ma), (b, mb) = renamed(a, renames), renamed(b, renames)
    moved = ma | mb
bad = sorted(set(a) ^ set(b))
for k in bad:
    print("only in", args.libs[0] if k in a else args.libs[1], ":", k)
for k in sorted(set(a) & set(b)):
    if a[k] != b[k]:
        bad.append(k)
        print("DIFFERS:", k, "instructions", len(a[k][0]), "vs", len(b[k][0]), "| metadata equal:", a[k][1] == b[k][1])
    elif k in moved:                            # the pairs the renames made, listed: the proof is about them
        print("same across the rename:", k, "|", len(a[k][0]), "instructions |", " ".join(" ".join(a[k][1]).split()))
print(f"{len(a)} vs {len(b)} kernels, {sum(len(v[0]) for v in a.values())} vs {sum(len(v[0]) for v in b.values())} instructions, {len(bad)} differ")
raise SystemExit(1 if bad else 0)
