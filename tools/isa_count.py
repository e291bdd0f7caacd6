#!/usr/bin/env python3
"""Instruction histogram of a kernel's largest block, from hipcc's assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -x hip csrc/msm.hip -o msm.s
    tools/isa_count.py msm.s 'k_accumulate<false>'

The kernel name is matched as a substring of the mangled symbol or of its demangled form (c++filt,
where there is one).  A block is what the assembly lists under one label (.LBBn_m): it runs from
that label to the next, through conditional branches that fall through (the exec-mask skips of
if-converted code), so the mixed addition of the MSM accumulation, whose special cases are such
skips, counts as one block -- the loop body DESIGN.md 2.6 reasons about.  Only instructions are
counted (no directives, no comments).  The script only reports; what the counts have to satisfy
is stated where they are recorded (profiles/)."""
import collections
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
# listed first and in this order; every other mnemonic follows by count
HEAD = ["v_mad_u64_u32", "v_addc_co_u32", "v_mov_b32", "v_mov_b64", "v_pk_mov_b32", "s_nop", "v_mul_lo_u32"]


def demangle(sym):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return sym
    try:
        return subprocess.run([tool, sym], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return sym


def functions(lines):
    """(symbol, first line, one past the last line) of every function of the file"""
    types = {m.group(1) for l in lines for m in [re.match(r"\s+\.type\s+([^,\s]+),@function", l)] if m}
    start = {}
    for n, l in enumerate(lines):
        m = LABEL.match(l)
        if m and m.group(1) in types:
            start[m.group(1)] = n + 1
    out = []
    for sym, a in start.items():
        b = next((n for n in range(a, len(lines)) if lines[n].startswith(".Lfunc_end")), len(lines))
        out.append((sym, a, b))
    return out


def blocks(lines, a, b):
    """(label, [mnemonic, ...]) of every labelled block of lines[a:b]"""
    out = [("<entry>", [])]
    for n in range(a, b):
        l = lines[n].split(";", 1)[0].rstrip()
        m = LABEL.match(l)
        if m:
            out.append((m.group(1), []))
            continue
        m = INSN.match(l)
        if m:
            out[-1][1].append(m.group(1))
    return [blk for blk in out if blk[1]]


def resources(lines, sym):
    """the kernel's register counts and scratch size from the .set lines that follow its body"""
    res = {}
    for l in lines:
        m = re.match(r"\s+\.set\s+" + re.escape(sym) + r"\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size),\s*(\S+)", l)
        if m:
            res[m.group(1)] = m.group(2)
    return res


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    path, want = argv[1], argv[2]
    with open(path) as f:
        lines = f.read().split("\n")
    hits = [(sym, a, b) for sym, a, b in functions(lines) if want in sym or want in demangle(sym)]
    if len(hits) != 1:
        names = "\n  ".join(demangle(s) for s, _, _ in hits) or "(none)"
        sys.exit(f"{want!r} names {len(hits)} functions of {path}:\n  {names}")
    sym, a, b = hits[0]
    blks = blocks(lines, a, b)
    label, ops = max(blks, key=lambda blk: len(blk[1]))
    hist = collections.Counter(re.sub(r"_(e32|e64|sdwa|dpp)$", "", op) for op in ops)
    res = resources(lines, sym)
    print(f"kernel          {demangle(sym).split('(')[0]}")
    print(f"vgprs           {res.get('num_vgpr', '?')}  (agprs {res.get('num_agpr', '?')}, sgprs {res.get('numbered_sgpr', '?')})")
    print(f"scratch bytes   {res.get('private_seg_size', '?')}")
    print(f"blocks          {len(blks)}, {sum(len(o) for _, o in blks)} instructions in all")
    print(f"largest block   {label}: {len(ops)} instructions")
    rest = sorted((op for op in hist if op not in HEAD), key=lambda op: (-hist[op], op))
    for op in [h for h in HEAD if hist[h]] + rest:
        print(f"  {op:<24}{hist[op]:>6}")


if __name__ == "__main__":
    main(sys.argv)
