#!/usr/bin/env python3
"""Per-kernel resources of two builds side by side, from hipcc's assembly: VGPRs, SGPRs, scratch
bytes, LDS bytes, instruction count and code bytes of every kernel, keyed by its demangled name, so
a kernel that moved to another file is compared with itself.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S -x hip csrc/mle.hip -o a/mle.s
    ... (one .s per source file, the parent's into one directory, the tree's into another)
    tools/kernel_table.py a b

The numbers are those of the "Kernel info" comment block after each kernel; instructions are the
mnemonic lines of its body (no directives, no comments).  x/y in a cell: parent/tree differ."""
import glob
import os
import re
import subprocess
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def kernels(path):
    """symbol -> (TotalNumVgprs, TotalNumSgprs, ScratchSize, LDSByteSize, instructions, codeLenInByte) from the
    'Kernel info' block hipcc prints after each kernel"""
    lines = open(path).read().split("\n")
    kern = {m.group(1) for l in lines for m in [re.match(r"\s+\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, cur, n, info = {}, None, 0, None
    for l in lines:
        m = LABEL.match(l)
        if m and m.group(1) in kern and cur is None:
            cur, n, info = m.group(1), 0, None
            continue
        if cur is None:
            continue
        if info is None:
            if l.startswith(".Lfunc_end"):
                info = {"insns": n}
            elif INSN.match(l.split(";", 1)[0].rstrip() + " "):
                n += 1
            continue
        m = re.match(r"; (\w+)\s*[:=] (\d+)", l)
        if m:
            info[m.group(1)] = m.group(2)
        if l.startswith("; COMPUTE_PGM_RSRC2:SCRATCH_EN"):
            out[cur] = (info["TotalNumVgprs"], info["TotalNumSgprs"], info["ScratchSize"], info["LDSByteSize"],
                        str(info["insns"]), info["codeLenInByte"])
            cur = None
    assert set(out) == kern, (path, kern - set(out))
    return out


def demangle(syms):
    r = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    return {s: re.sub(r"\(.*$", "", d).replace("void ", "").replace("tns::", "") for s, d in zip(syms, r)}


def collect(d):
    res = {}
    for p in sorted(glob.glob(os.path.join(d, "*.s"))):
        ks = kernels(p)
        dm = demangle(list(ks))
        for s, v in ks.items():
            res[dm[s]] = (os.path.basename(p)[:-2] + ".hip", v)
    return res


def main():
    a, b = collect(sys.argv[1]), collect(sys.argv[2])
    print(f"{'kernel':<44}{'parent file':<17}{'tree file':<17}{'vgpr':>10}{'sgpr':>10}{'scratch':>10}{'lds':>12}{'insns':>14}{'code bytes':>14}  same")
    for k in sorted(set(a) | set(b)):
        fa, va = a.get(k, ("-", ("-",) * 6))
        fb, vb = b.get(k, ("-", ("-",) * 6))
        cols = [f"{x}/{y}" if x != y else f"{x}" for x, y in zip(va, vb)]
        print(f"{k:<44}{fa:<17}{fb:<17}{cols[0]:>10}{cols[1]:>10}{cols[2]:>10}{cols[3]:>12}{cols[4]:>14}{cols[5]:>14}  {'yes' if va == vb else 'NO'}")


main()
