#!/usr/bin/env python3
"""Scratch (register spill) traffic of the kernels of one gfx950 assembly file, by where it sits.

usage: tools/loop_scratch.py FILE.s [name filter]        (FILE.s: tools/asm_diff.py --keep=DIR leaves old_*.s and new_*.s there)

Per kernel: the vector scratch loads / stores in all, those inside any loop (a label with a later branch back to it) by
nesting depth, and those inside the innermost loops that hold MFMAs -- the K loops of the conv and weight-gradient kernels,
where a spill costs a memory round trip per K-step.  Kernels without scratch instructions are left out.

The loop finder (find_loops, innermost_with, scratch_counts) is what tools/asm_diff.py classifies a changed kernel with."""
import re, subprocess, sys

_BRANCH = re.compile(r"s_c?branch\w*\s+(\.LBB\w+)")


def find_loops(body):
    """(label position, branch position) of every backward branch in a kernel's instruction lines (labels included)"""
    pos = {b[:-1]: i for i, b in enumerate(body) if b.endswith(":")}
    loops = []
    for i, b in enumerate(body):
        m = _BRANCH.match(b)
        if m and m.group(1) in pos and pos[m.group(1)] < i: loops.append((pos[m.group(1)], i))
    return loops


def innermost_with(body, loops, needle):
    """the loops that hold an instruction matching `needle` (a regex) and no other such loop"""
    rx = re.compile(needle)
    held = [(lo, hi) for lo, hi in loops if any(rx.match(b) for b in body[lo:hi])]
    return [(lo, hi) for lo, hi in held if not any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi for l2, h2 in held)]


def scratch_counts(body, loops, hot):
    """scratch instructions: in all, inside loops by nesting depth, inside the `hot` loops"""
    tot, inloop = 0, {}
    for i, b in enumerate(body):
        if b.startswith("scratch_"):
            tot += 1
            d = sum(1 for lo, hi in loops if lo <= i <= hi)
            if d: inloop[d] = inloop.get(d, 0) + 1
    in_hot = sum(1 for i, b in enumerate(body) if b.startswith("scratch_") and any(lo <= i <= hi for lo, hi in hot))
    return tot, inloop, in_hot


def main(path, flt):
    lines = open(path).read().splitlines()
    kern = {}
    cur = None
    for ln in lines:
        s = ln.split(";", 1)[0].rstrip()
        m = re.match(r"^(_Z\w+):", s)
        if m: cur = m.group(1); kern[cur] = []; continue
        if s.strip().startswith(".Lfunc_end"): cur = None; continue
        if cur is not None and s.strip(): kern[cur].append(s.strip())
    names = list(kern)
    dem = dict(zip(names, subprocess.run(["c++filt", *names], capture_output=True, text=True).stdout.splitlines()))
    for n in names:
        if "Kernel" in n or (flt and flt not in dem[n]): continue
        body = kern[n]
        if not any("s_endpgm" in b for b in body): continue
        loops = find_loops(body)
        tot, inloop, in_mfma = scratch_counts(body, loops, innermost_with(body, loops, r"v_mfma"))
        if tot:
            print(f"{dem[n][:64]:64s} scratch instr {tot:3d}  in loops by depth {inloop or '-'}  in the innermost loops that hold MFMAs (the K loops) {in_mfma}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
