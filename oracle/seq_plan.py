"""The whole-sequence plan (csrc/seq.hip: the check, the forward planner, BwdPlanner, add_wrap_steps) as plain records, and the
sweep that pins it.

The three ``nint_debug_seq_plan*`` entries run the check and the planner of a pass on the host (no GPU: the CU count falls
back to 256).  ``record`` flattens what one call returns -- the return value, then every field of every nint_launch_rec --
into a row; ``sweep`` lists the cases of tests/golden/seq_plan.npy.xz, which holds the rows the library gave BEFORE the open,
closed-loop and roll-out windows were folded into one pass description (made from the parent commit's library):

    python -m oracle.seq_plan LIBRARY.so OUT.npy.xz

tests/test_seq_plan_cpu.py holds the product library against that file, row for row.  A record's ``index`` is its step's
position in the enqueue list, so the steps without records (halo wraps, feedback launches and their adjoints) are pinned
through the gaps.
"""
from __future__ import annotations

import ctypes as C
import io
import lzma
import os
import sys
from typing import Dict, Iterator, List, Sequence, Tuple

import numpy as np

EXPLICIT = 0x40000000
# (C, hidden, ks): one to four layers, each with a thin layer-0 input (folded where nint_xfold_pays) and a plain one; the two
# k = 3, Ch = 8 stacks run the direct nint_cell_fwd call (tiny / stencil), WIDE_HEAD a head the feedback kernel does not hold
STACKS = ((4, (16,), (5,)), (64, (16,), (3,)), (4, (8,), (3,)), (16, (8,), (3,)),
          (5, (32, 16), (5, 3)), (64, (32, 16), (3, 3)),
          (5, (32, 16, 16), (5, 3, 3)), (64, (32, 16, 16), (5, 3, 3)),
          (5, (32, 32, 16, 16), (5, 3, 3, 3)), (64, (64, 32, 16, 16), (3, 3, 3, 3)),
          (5, (32, 160), (3, 3)))
WIDE_HEAD = len(STACKS) - 1
T = 4
# (B, H, W): the closed-loop tests' small grid, and both sides of the small-batch rule at 100 x 154 (wave = 5 below it, 4 above)
SHAPES = ((2, 13, 37), (1, 100, 154), (8, 100, 154))
FUSE = (0, 1, 2, EXPLICIT | 0b0110 | (0b0100 << 8), EXPLICIT | 0b1000 | (0b0010 << 16) | (0b1000 << 8))
CAP = 48                    # records a row has room for
REC = ("index", "bwd", "op", "layer", "t", "kernel", "dtype", "epi", "wn", "wk", "ntw", "mt", "strip", "gx", "gy", "nt_begin")
FIELDS = ["rc"] + [f"rec{i}.{f}" for i in range(CAP) for f in REC]
# entry: 0 nint_debug_seq_plan, 1 _closed, 2 _rollout.  fb: 0 = a NULL nint_feedback, 1 = (w set), 2 = (w NULL); O_kind: 0, 1,
# Cx, Cx + 1.  dh_seq / dx: 0 NULL, 1 set, 2 misaligned.  wave 7 is no mode.  rows: nint_layer.tile_rows of every layer (1: the
# stencil kernel where it holds the layer).
CASE = ("entry", "bwd", "stack", "bf16", "shape", "T", "rows", "wave", "cyclic", "has_init", "zero", "fuse", "need_dx", "parts", "train_from",
        "accumulate", "dh_seq", "dx", "fb", "O_kind", "from")
_BASE = dict(entry=(0,), bwd=(0,), stack=(6,), bf16=(0, 1), shape=(0,), T=(T,), rows=(0,), wave=(4,), cyclic=(0,), has_init=(0,), zero=(0,),
             fuse=(0,), need_dx=(0,), parts=(0,), train_from=(0,), accumulate=(0,), dh_seq=(0,), dx=(1,), fb=(1,), O_kind=(1,))
_BASE["from"] = (1,)
_ALL = tuple(range(len(STACKS) - 1))
_BWD = dict(bwd=(1,), zero=(0, 1), fuse=tuple(range(len(FUSE))), need_dx=(0, 1), accumulate=(0, 1), has_init=(0, 1))
# (dims that differ from _BASE, number of cases, stride through their product)
TIERS = (
    # plans that are mostly accepted: every stack, shape, mode
    (dict(entry=(0, 1), stack=_ALL, shape=(0, 1, 2), rows=(0, 1, 8), wave=range(6), cyclic=(0, 1), has_init=(0, 1)), 900, 7919),
    (dict(entry=(1,), stack=_ALL, shape=(0, 1, 2), rows=(0, 1, 8), wave=range(6), cyclic=(0, 1), has_init=(0, 1), O_kind=(1, 2),
          **{"from": (0, 1, T - 1, T)}), 1300, 7919),
    (dict(_BWD, entry=(0, 1, 2), stack=_ALL, shape=(0, 1, 2), wave=range(6), cyclic=(0, 1), parts=(0, 1, 2), train_from=range(5),
          dh_seq=(0, 1), O_kind=(0, 1), **{"from": (T, T + 1)}), 2200, 104729),
    (dict(_BWD, entry=(2,), stack=_ALL, shape=(0, 1, 2), wave=range(6), cyclic=(0, 1), dh_seq=(1,), O_kind=(1, 2),
          **{"from": (1, 2, T - 1)}), 1400, 104729),
    # what the checks refuse, and which code a doubly wrong call gets: every field at its invalid values too
    (dict(entry=(1,), stack=(0, 6), wave=(0, 4, 7), cyclic=(0, 1), has_init=(0, 1), fb=(0, 1, 2), O_kind=range(4),
          **{"from": (-1, 0, 1, T - 1, T, T + 1)}), 600, 7919),
    (dict(_BWD, entry=(0, 1, 2), stack=(0, 4, 6), wave=(0, 4, 7), cyclic=(0, 1), parts=(0, 1, 2), train_from=range(5),
          dh_seq=(0, 1, 2), dx=(0, 1, 2), fb=(0, 1, 2), O_kind=range(4), **{"from": (-1, 0, 1, T - 1, T, T + 1)}), 2400, 1299709),
    (dict(_BWD, entry=(2,), stack=(0, 6, 8), wave=(0, 5, 7), parts=(0, 1), train_from=(0, 1), dh_seq=(0, 1, 2), dx=(0, 1, 2),
          fb=(1, 1, 2), O_kind=(1, 1, 2, 3), **{"from": (0, 1, T - 1)}), 900, 15485863),
    # a head the staged kernels do not hold: refused by the planner (NINT_E_SHAPE)
    (dict(entry=(1, 2), bwd=(0, 1), stack=(WIDE_HEAD,), bf16=(0,), wave=(0,), dh_seq=(1,), **{"from": (1, T)}), 8, 1),
)


def sweep() -> Iterator[Tuple[int, ...]]:
    """cases as CASE tuples: each tier walks the product of its dimensions with a stride coprime to its size"""
    for dims, count, stride in TIERS:
        d: Dict[str, Sequence[int]] = {k: tuple(dims.get(k, _BASE[k])) for k in CASE}
        sizes = [len(d[k]) for k in CASE]
        n = int(np.prod(sizes))
        assert count <= n and np.gcd(stride, n) == 1, (count, n, stride)
        for i in range(count):
            idx, case = (i * stride) % n, []
            for k, size in zip(CASE, sizes):
                case.append(d[k][idx % size])
                idx //= size
            c = dict(zip(CASE, case))
            L = len(STACKS[c["stack"]][1])
            c["train_from"] %= L + 1
            if c["entry"] == 2:
                c["bwd"] = 1
            yield tuple(c[k] for k in CASE)


def _seq_of(**kw):
    try:
        import test_launch_plan_cpu as TLP
    except ImportError:      # (outside pytest)
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import test_launch_plan_cpu as TLP
    return TLP._seq_of(**kw)


def build(case):
    """(nint_seq, nint_feedback or None) of one case: the plan tests' nint_seq with the case's fields written over it"""
    from nasa_niswan_amd import _lib
    c = dict(zip(CASE, case))
    Cin, hidden, ks = STACKS[c["stack"]]
    B, H, W = SHAPES[c["shape"]]
    s = _seq_of(C_=Cin, hidden=list(hidden), ks=list(ks), B=B, T=c["T"], H=H, W=W, dtype="bf16" if c["bf16"] else "f32", wave=0, rows=c["rows"],
                fuse=FUSE[c["fuse"]], has_init=bool(c["has_init"]), zero=bool(c["zero"]), need_dx=bool(c["need_dx"]), train=True)
    s.wave, s.lon_cyclic, s.bwd_parts, s.train_from, s.accumulate = c["wave"], c["cyclic"], c["parts"], c["train_from"], c["accumulate"]
    s.dh_seq = (None, 1 << 30, (1 << 30) + 8)[c["dh_seq"]]
    s.dx = (None, s.dx, (s.dx or 0) + 8)[c["dx"]]
    fb = None
    if c["fb"]:
        fb = _lib.NintFeedback()
        fb.w, fb.b = (1 << 12 if c["fb"] == 1 else None), None
        fb.O, fb.from_step = (0, 1, Cin, Cin + 1)[c["O_kind"]], c["from"]
    return s, fb


def record(lib, case) -> np.ndarray:
    """one row of FIELDS: the entry's return value (the number of records, or the refusal) and the records"""
    from nasa_niswan_amd import _lib
    c = dict(zip(CASE, case))
    s, fb = build(case)
    recs = (_lib.NintLaunchRec * CAP)()
    pfb = None if fb is None else C.byref(fb)
    if c["entry"] == 0:
        rc = lib.nint_debug_seq_plan(C.byref(s), c["bwd"], recs, CAP)
    elif c["entry"] == 1:
        rc = lib.nint_debug_seq_plan_closed(C.byref(s), pfb, c["bwd"], recs, CAP)
    else:
        rc = lib.nint_debug_seq_plan_rollout(C.byref(s), pfb, recs, CAP)
    assert rc <= CAP, (case, rc)
    row = np.zeros(len(FIELDS), dtype=np.int64)
    row[0] = rc
    if rc > 0:
        row[1:1 + rc * len(REC)] = np.frombuffer(recs, dtype=np.int32, count=rc * len(REC))
    return row


def table(lib) -> Tuple[np.ndarray, np.ndarray]:
    cases = list(sweep())
    return np.array(cases, dtype=np.int64), np.stack([record(lib, c) for c in cases])


def load(path) -> Tuple[np.ndarray, np.ndarray]:
    """(cases, rows) of a fixture file"""
    with lzma.open(path) as f:
        a = np.load(io.BytesIO(f.read()))
    return a[:len(CASE)].T.astype(np.int64), a[len(CASE):].T.astype(np.int64)


def main(argv):
    from nasa_niswan_amd import _lib
    lib = _lib.load(argv[0])
    cases, rows = table(lib)
    # one .npy, column-major (a field changes slowly along the sweep, which is what the compression feeds on), xz-compressed
    buf = io.BytesIO()
    np.save(buf, np.ascontiguousarray(np.concatenate([cases, rows], axis=1).T.astype(np.int32)))
    with lzma.open(argv[1], "wb", preset=9) as f:
        f.write(buf.getvalue())
    print(f"{len(cases)} cases, {int((rows[:, 0] < 0).sum())} of them refused, {len(FIELDS)} fields -> {argv[1]}")


if __name__ == "__main__":
    main(sys.argv[1:])
