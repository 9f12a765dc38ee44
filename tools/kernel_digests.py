"""Device code of two builds of the library compared kernel by kernel: for every object of both build/obj directories
the gfx950 code object is taken out of the host object (llvm-objcopy, clang-offload-bundler) and disassembled
(llvm-objdump -d, addresses and encodings dropped); per kernel the sha256 (first 16 hex digits) of its disassembly and its
instruction lines, parent then this build, `same` where both are equal; per object the digest of the whole disassembly.
Usage: python tools/kernel_digests.py PARENT_OBJDIR THIS_OBJDIR [object name prefix ...]  > profiles/<name>.txt"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def disassembly(obj):
    """{kernel symbol: [instruction lines]} of the object's gfx950 code, in order; {} for an object without device code."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj,
                            os.path.join(d, "copy.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
            return {}
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                            "--input=" + fat, "--output=" + co], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
            return {}
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co],
                              stdout=subprocess.PIPE, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].rstrip())
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main():
    parent, this = sys.argv[1], sys.argv[2]
    prefixes = tuple(sys.argv[3:])
    names = sorted({f for d in (parent, this) for f in os.listdir(d) if f.endswith(".o")})
    differing = []
    for f in names:
        if prefixes and not f.startswith(prefixes):
            continue
        sides = [disassembly(os.path.join(d, f)) if os.path.exists(os.path.join(d, f)) else None for d in (parent, this)]
        if not any(sides):
            continue
        a, b = [s or {} for s in sides]
        whole = [digest([k + ":" + l for k, v in s.items() for l in v]) if s else "-" for s in (a, b)]
        print("object %s: %d kernels parent, %d this; disassembly %s / %s %s" % (
            f[:-2], len(a), len(b), whole[0], whole[1], "same" if whole[0] == whole[1] else "DIFFERENT"))
        for k in sorted(set(a) | set(b)):
            da = "%s %d instr" % (digest(a[k]), len(a[k])) if k in a else "absent"
            db = "%s %d instr" % (digest(b[k]), len(b[k])) if k in b else "absent"
            same = da == db
            if not same:
                differing.append((f[:-2], k))
            print("  %s\n    parent %s\n    this   %s  %s" % (k, da, db, "same" if same else
                                                              "new" if k not in a else "gone" if k not in b else "DIFFERENT"))
    print("\nkernels that differ, are new or are gone: %d" % len(differing))
    for f, k in differing:
        print("  %s %s" % (f, k))


if __name__ == "__main__":
    main()
