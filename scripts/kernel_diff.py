"""Per-kernel comparison of the gfx950 code objects of two builds.

    python scripts/kernel_diff.py PARENT/libiqo_amd/build libiqo_amd/build

For every object file of the second build directory that holds device code: unbundle the gfx950 code object, and
compare each kernel's code bytes (.text, by symbol) and its kernel descriptor (.rodata, NAME.kd) with the first
build's by SHA-1.  A refactor of host code only must report every kernel identical.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "")
def code_object(obj, tmp):
    fat = os.path.join(tmp, "x.fatbin"); co = os.path.join(tmp, "x.co")
    subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "x.o")])
    subprocess.check_call([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    return co
def symbols(co):
    data = open(co, "rb").read()
    secs = {}
    for line in subprocess.check_output([LLVM + "llvm-readelf", "-SW", co], text=True).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
    out = {}
    for line in subprocess.check_output([LLVM + "llvm-readelf", "-sW", co], text=True).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, size, name = int(f[1], 16), int(f[2]), f[7]
            sname, saddr, soff = secs[int(f[6])]
            if sname in (".text", ".rodata"):
                out[name] = (f[3], size, hashlib.sha1(data[soff + addr - saddr: soff + addr - saddr + size]).hexdigest())
    return out
def demangle(names):
    out = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return dict(zip(names, out))
a, b = sys.argv[1:3]
tot = [0, 0, 0]
for obj in sorted(os.listdir(b)):
    if not obj.endswith(".o"):
        continue
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        try:
            sa, sb = symbols(code_object(os.path.join(a, obj), t1)), symbols(code_object(os.path.join(b, obj), t2))
        except subprocess.CalledProcessError:
            print("%-22s no device code" % obj); continue
    kern = [n for n in sb if sb[n][0] == "FUNC"]
    same = [n for n in kern if sa.get(n) == sb[n] and sa.get(n + ".kd") == sb.get(n + ".kd")]
    diff = sorted(set(kern) - set(same)); gone = sorted(n for n in sa if sa[n][0] == "FUNC" and n not in sb)
    print("%-22s %4d kernels, %4d identical (code bytes and kernel descriptor), %d differ, %d only in the parent" % (obj, len(kern), len(same), len(diff), len(gone)))
    d = demangle(diff + gone) if diff + gone else {}
    for n in diff: print("    differs: " + d[n])
    for n in gone: print("    parent only: " + d[n])
    tot[0] += len(kern); tot[1] += len(same); tot[2] += len(diff) + len(gone)
print("total: %d kernels, %d identical, %d not" % tuple(tot))
