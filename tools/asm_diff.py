#!/usr/bin/env python3
"""Device assembly of one csrc file in two source directories, compared kernel by kernel.

usage: tools/asm_diff.py FILE.hip OLD_CSRC NEW_CSRC [-DNAME ...] [--keep=DIR [--reuse-old]] [--rename=REGEX=REPL]

Each side is compiled with the flags of nasa-niswan_amd/build.py plus ``--cuda-device-only -S`` (its own directory on the
include path, so each side sees its own nint_common.h).  Per mangled kernel name two things are compared by plain equality:

* the instruction stream: the lines from the kernel's label to the end of the function, comments and assembler directives
  dropped, the function index taken out of ``.LBB<function>_<block>`` labels (it moves when a kernel is added above);
* the resource block: the ``.amdhsa_*`` lines of its ``.amdhsa_kernel`` descriptor.

A device function that a kernel calls out of line (a lambda the compiler did not inline) is compared in the same way, by its
instruction stream alone, and counted with the kernels.

``--rename=REGEX=REPL`` (re.sub on the OLD side's mangled names, before the two sides are matched) pairs kernels whose name
moved for a reason that cannot touch their code, such as a template parameter that only ever had one value being dropped.

A kernel that passes both is in class A (identical).  One that does not is in class B (same hot loop) where all of these hold:

* the resource block is identical (VGPRs, AGPRs, SGPRs, scratch, LDS);
* its hot loops -- the innermost loops that hold MFMAs, or, in a kernel without MFMAs, the innermost loops that hold FMAs (the
  stencil kernel's main loop), found by tools/loop_scratch.py -- are the same in number and order and hold the same instruction
  sequence once register numbers and local label numbers are masked: opcodes, modifiers, offsets, immediates and s_waitcnt
  counts are compared as they stand;
* it has no scratch instruction where the old side has none, and no more of them inside its hot loops.

Printed: the kernel count on each side, the names on one side only, and the kernels that differ (class, instruction counts, the
resource lines that changed, what kept a kernel out of class B).  Exit status 0 where both sides hold the same kernels and none
differs, 2 where some differ and all of those are in class B, 1 otherwise.  A refactor of host code is checked with this: it
must leave every kernel as it was (profiles/conv_dispatch_asm.txt); a refactor of device code may move instructions outside the
hot loops (profiles/conv_body_refactor_asm.txt).  ``--reuse-old`` (with ``--keep=DIR``) takes DIR's old_*.s as it is."""
from __future__ import annotations

import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loop_scratch import find_loops, innermost_with, scratch_counts  # noqa: E402


def _build_py():
    spec = importlib.util.spec_from_file_location("nint_build", os.path.join(ROOT, "nasa-niswan_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(B, name, csrc, out, defines):
    flags = [f for f in B.FLAGS if f != "-I" + B.CSRC] + ["-I" + csrc] + list(defines)
    cmd = [B.HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(csrc, name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return cmd


_LBB = re.compile(r"\.LBB\d+_(\d+)")


def kernels(path):
    """mangled name -> (instruction lines, resource lines) of every kernel, and of every device function a kernel calls out of
    line (no resource block of its own: an empty list)"""
    lines = open(path).read().splitlines()
    res, cur = {}, None
    for ln in lines:
        s = ln.split(";", 1)[0].strip()
        if s.startswith(".type") and s.endswith(",@function"):
            res.setdefault(s.split()[1].rsplit(",", 1)[0], [])
        elif s.startswith(".amdhsa_kernel "):
            cur = s.split()[1]
        elif s == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and s.startswith(".amdhsa_"):
            res[cur].append(" ".join(s.split()))
    out = {}
    labels = [ln.split(";", 1)[0].strip() for ln in lines]
    start = {s[:-1]: i for i, s in enumerate(labels) if s.endswith(":") and s[:-1] in res}
    for name, i in start.items():
        body = []
        for ln in lines[i + 1:]:
            s = ln.split(";", 1)[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue
            body.append(_LBB.sub(r".LBB_\1", " ".join(s.split())))
        out[name] = (body, res[name])
    missing = sorted(set(res) - set(out))
    if missing:
        raise SystemExit("no function body found for: " + ", ".join(missing))
    return out


_REG = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")


def _mask(line):
    """register numbers (a range keeps its width) and local label numbers taken out of one instruction line"""
    line = _REG.sub(lambda m: m.group(1) + ("#" if m.group(2) else f"[#+{int(m.group(4)) - int(m.group(3))}]"), line)
    line = re.sub(r"\bvcc_(lo|hi)\b", "s#", re.sub(r"\bvcc\b", "s[#+1]", line))   # vcc named as an operand is SGPRs 106:107
    return re.sub(r"\.LBB_\d+", ".LBB_#", line)


def hot_loops(body):
    """(the masked instruction sequences of the hot loops, scratch instructions in all, scratch instructions inside them)"""
    loops = find_loops(body)
    hot = innermost_with(body, loops, r"v_mfma") or innermost_with(body, loops, r"v_(pk_)?fma")
    tot, _, in_hot = scratch_counts(body, loops, hot)
    return [[_mask(b) for b in body[lo:hi + 1]] for lo, hi in sorted(hot)], tot, in_hot


def class_b(old, new):
    """why `new` is NOT in class B against `old` (both (instruction lines, resource lines)); an empty list: it is"""
    why = []
    if old[1] != new[1]:
        why.append("resource block differs")
    (ho, to, io), (hn, tn, in_) = hot_loops(old[0]), hot_loops(new[0])
    if len(ho) != len(hn):
        why.append(f"hot loops: old {len(ho)}, new {len(hn)}")
    else:
        for i, (a, b) in enumerate(zip(ho, hn)):
            if a != b:
                at = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                why.append(f"hot loop {i}: old {len(a)} lines, new {len(b)}, first difference at line {at}: "
                           f"{a[at] if at < len(a) else '(end)'}  |  {b[at] if at < len(b) else '(end)'}")
    if (tn and not to) or in_ > io:
        why.append(f"scratch instructions: old {to} ({io} in hot loops), new {tn} ({in_})")
    return why


def demangle(names):
    try:
        r = subprocess.run(["c++filt", *names], capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    args = [a for a in argv if not a.startswith("-D") and not a.startswith("--")]
    reuse_old = "--reuse-old" in argv
    defines = [a for a in argv if a.startswith("-D")]
    keep = [a.split("=", 1)[1] for a in argv if a.startswith("--keep=")]
    renames = [a.split("=", 1)[1].rsplit("=", 1) for a in argv if a.startswith("--rename=")]
    if len(args) != 3:
        raise SystemExit(__doc__)
    name, old, new = args[0], os.path.abspath(args[1]), os.path.abspath(args[2])
    B = _build_py()
    scratch = None if keep else tempfile.TemporaryDirectory(prefix="asm_diff_")      # --keep=DIR: the two .s files stay there
    tmp = keep[0] if keep else scratch.name
    os.makedirs(tmp, exist_ok=True)
    outs = [os.path.join(tmp, side + "_" + name.replace(".hip", ".s")) for side in ("old", "new")]
    sides = list(zip((old, new), outs))[1 if reuse_old and keep and os.path.exists(outs[0]) else 0:]
    with ThreadPoolExecutor(max_workers=2) as ex:
        cmds = list(ex.map(lambda p: compile_asm(B, name, p[0], p[1], defines), sides))
    ko, kn = kernels(outs[0]), kernels(outs[1])
    for rx, repl in renames:                  # names, and the symbols that instructions refer to (a call out of line)
        renamed = {re.sub(rx, repl, n): ([re.sub(rx.lstrip("^"), repl, ln) for ln in body], r) for n, (body, r) in ko.items()}
        if len(renamed) != len(ko):
            raise SystemExit(f"--rename={rx}={repl} maps two kernels of the old side onto one name")
        print(f"# old names through re.sub({rx!r}, {repl!r}): {sum(n not in ko for n in renamed)} renamed")
        ko = renamed
    if scratch:
        scratch.cleanup()
    flags = " ".join(a for a in cmds[0][1:-3] if not a.startswith("-I"))
    print(f"# csrc/{name}, device assembly for gfx950, old against new: hipcc {flags}")
    print("# per mangled kernel name: the instruction stream (comments and directives dropped, the function index taken out")
    print("# of .LBB labels) and the .amdhsa_* resource block, compared by equality")
    print(f"kernels: old {len(ko)}, new {len(kn)}")
    dm = demangle(sorted(set(ko) | set(kn)))
    only_old, only_new = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
    print(f"only in old ({len(only_old)}):" + "".join(f"\n  {n}  {dm[n]}" for n in only_old))
    print(f"only in new ({len(only_new)}):" + "".join(f"\n  {n}  {dm[n]}" for n in only_new))
    both = sorted(set(ko) & set(kn))
    differ = [n for n in both if ko[n] != kn[n]]
    why = {n: class_b(ko[n], kn[n]) for n in differ}
    neither = [n for n in differ if why[n]]
    print(f"in both: {len(both)}, class A (identical): {len(both) - len(differ)}, class B (same hot loop): "
          f"{len(differ) - len(neither)}, neither: {len(neither)}")
    for n in differ:
        (io, ro), (in_, rn) = ko[n], kn[n]
        print(f"  {'neither' if why[n] else 'B'}  {n}  {dm[n]}")
        print(f"    instructions: old {len(io)}, new {len(in_)}" + ("" if io != in_ else " (the same stream)")
              + f"; hot loops {len(hot_loops(in_)[0])}")
        for a, b in zip(ro, rn):
            if a != b:
                print(f"    {a}  ->  {b.split(None, 1)[-1]}")
        for w in why[n]:
            print(f"    not B: {w}")
    by_name = {}
    for n in both:
        if n not in differ:
            base = dm[n].split("<", 1)[0].replace("void ", "")
            by_name[base] = by_name.get(base, 0) + 1
    print("identical, by kernel:" + "".join(f"\n  {k:<34}{v:>3} instance(s)" for k, v in sorted(by_name.items())))
    if only_old or only_new or neither:
        return 1
    return 2 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
