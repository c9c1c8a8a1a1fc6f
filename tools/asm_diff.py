#!/usr/bin/env python3
"""Device assembly of one csrc file in two source directories, compared kernel by kernel.

usage: tools/asm_diff.py FILE.hip OLD_CSRC NEW_CSRC [-DNAME ...] [--keep=DIR] [--rename=REGEX=REPL]

Each side is compiled with the flags of nasa-niswan_amd/build.py plus ``--cuda-device-only -S`` (its own directory on the
include path, so each side sees its own nint_common.h).  Per mangled kernel name two things are compared by plain equality:

* the instruction stream: the lines from the kernel's label to the end of the function, comments and assembler directives
  dropped, the function index taken out of ``.LBB<function>_<block>`` labels (it moves when a kernel is added above);
* the resource block: the ``.amdhsa_*`` lines of its ``.amdhsa_kernel`` descriptor.

A device function that a kernel calls out of line (a lambda the compiler did not inline) is compared in the same way, by its
instruction stream alone, and counted with the kernels.

``--rename=REGEX=REPL`` (re.sub on the OLD side's mangled names, before the two sides are matched) pairs kernels whose name
moved for a reason that cannot touch their code, such as a template parameter that only ever had one value being dropped.

Printed: the kernel count on each side, the names on one side only, and the kernels that differ (instruction counts and the
resource lines that changed).  Exit status 0 where both sides hold the same kernels and none differs, 1 otherwise.  A refactor
of host code is checked with this: it must leave every kernel as it was (profiles/conv_dispatch_asm.txt)."""
from __future__ import annotations

import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def demangle(names):
    try:
        r = subprocess.run(["c++filt", *names], capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    args = [a for a in argv if not a.startswith("-D") and not a.startswith("--keep") and not a.startswith("--rename")]
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
    with ThreadPoolExecutor(max_workers=2) as ex:
        cmds = list(ex.map(lambda p: compile_asm(B, name, p[0], p[1], defines), zip((old, new), outs)))
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
    print(f"in both: {len(both)}, identical: {len(both) - len(differ)}, differing: {len(differ)}")
    for n in differ:
        (io, ro), (in_, rn) = ko[n], kn[n]
        print(f"  {n}  {dm[n]}")
        print(f"    instructions: old {len(io)}, new {len(in_)}" + ("" if io != in_ else " (the same stream)"))
        for a, b in zip(ro, rn):
            if a != b:
                print(f"    {a}  ->  {b.split(None, 1)[-1]}")
    by_name = {}
    for n in both:
        if n not in differ:
            base = dm[n].split("<", 1)[0].replace("void ", "")
            by_name[base] = by_name.get(base, 0) + 1
    print("identical, by kernel:" + "".join(f"\n  {k:<34}{v:>3} instance(s)" for k, v in sorted(by_name.items())))
    return 0 if not (only_old or only_new or differ) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
