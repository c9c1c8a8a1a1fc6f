"""The weight-gradient plan (csrc/wgrad.hip: wg_plan, nint_internal_wgrad_plan) as plain records, and the sweep that pins it.

``nint_debug_wgrad_plan`` runs the planner of nint_conv_wgrad / nint_seq_bwd on the host.  ``record`` flattens what it returns
for one case into a row of FIELDS; ``sweep`` lists the cases of tests/golden/wgrad_plan.npy.xz, which holds the rows the planner
gave BEFORE the instance table replaced dispatch_wgrad (made from the parent commit's csrc plus this entry alone):

    python -m oracle.wgrad_plan LIBRARY.so OUT.npy.xz

tests/test_wgrad_plan_cpu.py holds the product library against that file, row for row.
"""
from __future__ import annotations

import ctypes as C
import io
import itertools
import lzma
import struct
import sys
from typing import Iterator, List, Tuple

import numpy as np

KS = (1, 3, 5, 7, 9)
WIDE = (0, 1, 2)
# (Cx, Ch): the KEYS, SHAPES and REAL shapes of tests/test_gpu_exact_reductions.py and tests/test_gpu_wgrad_families.py, the
# bench and cfg3 / cfg4 layers, and channel counts that are no multiple of 32 (or of 16)
PAIRS = ((62, 64), (64, 64), (64, 32), (16, 32), (5, 64), (5, 32), (2, 16), (48, 48), (48, 16), (16, 16), (3, 32), (5, 16),
         (6, 16), (10, 16), (4, 16), (62, 128), (128, 64), (64, 128), (32, 32), (126, 64), (32, 16), (128, 128), (40, 24),
         (7, 20), (62, 48), (64, 16))
GRIDS = ((37, 50), (100, 154), (7, 33))
IMAGES = ((1, 1), (7, 1), (96, 8))          # (N, B): the h source skips 0 or B images
N_CU = (256, 64)

SRC = ("CB", "JG", "TG", "nblk", "ntiles", "tiles_per_split", "want_db", "is_h", "off")
LAUNCH = ("family", "KS", "NTC", "JW", "KX", "nparts", "gx", "gy", "block", "lds")
FIELDS = (["rc", "workspace_bytes", "n_launch", "n_fold", "fold_grid", "fold_block"]
          + [f"launch{i}.{f}" for i in range(2) for f in LAUNCH + tuple(f"src{q}.{s}" for q in range(2) for s in SRC)]
          + [f"fold{i}.{f}" for i in range(2) for f in ("blk_begin", "splits", "waves")])
_REC = "@4i" + ("10i" + "8iq" * 2) * 2 + "6i"
CASE = ("k", "bf16", "xfold", "wide", "Cx", "Ch", "H", "W", "N", "h_skip", "n_cu")


def rup(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def layer_of(Cx: int, Ch: int, k: int, bf16: int, xfold: int, wide: int):
    """nint_layer as SeqEngine pads it (nint_kc: 32 channels in bf16, 16 in f32)"""
    from nasa_niswan_amd._lib import NintLayer
    kc = 32 if bf16 else 16
    ly = NintLayer()
    ly.Cx, ly.Ch, ly.k, ly.xfold, ly.wide = Cx, Ch, k, xfold, wide
    ly.Cxp, ly.Ch16, ly.Chp = rup(k * Cx if xfold else Cx, kc), rup(Ch, 16), rup(Ch, kc)
    return ly


def sweep() -> Iterator[Tuple[int, ...]]:
    """cases as CASE tuples"""
    for k, dt, xfold, wide, (Cx, Ch), (H, W), (N, B), skip, n_cu in itertools.product(
            KS, (1, 0), (0, 1), WIDE, PAIRS, GRIDS, IMAGES, (0, 1), N_CU):
        yield (k, dt, xfold, wide, Cx, Ch, H, W, N, skip * B, n_cu)


def record(lib, case) -> List[int]:
    """one row of FIELDS: the planner's return code, the workspace query, and -- where it plans -- every record"""
    from nasa_niswan_amd._lib import NintGeom, NintWgradPlanRec
    k, bf16, xfold, wide, Cx, Ch, H, W, N, h_skip, n_cu = case
    ly = layer_of(Cx, Ch, k, bf16, xfold, wide)
    g = NintGeom()
    assert lib.nint_geom_make(C.byref(g), H, W, max(k // 2, 1)) == 0
    out = NintWgradPlanRec()
    rc = lib.nint_debug_wgrad_plan(C.byref(ly), C.byref(g), bf16, N, h_skip, n_cu, C.byref(out))
    row = [rc, lib.nint_wgrad_workspace_bytes(C.byref(ly), bf16, n_cu)]
    if rc != 0:
        return row + [0] * (len(FIELDS) - 2)
    return row + list(struct.unpack_from(_REC, out))      # nint_wgrad_plan_rec is FIELDS[2:] in this order


def table(lib) -> Tuple[np.ndarray, np.ndarray]:
    cases = list(sweep())
    return np.array(cases, dtype=np.int32), np.array([record(lib, c) for c in cases], dtype=np.int64)


def load(path) -> Tuple[np.ndarray, np.ndarray]:
    """(cases, rows) of a fixture file"""
    with lzma.open(path) as f:
        a = np.load(io.BytesIO(f.read()))
    return a[:len(CASE)].T.astype(np.int32), a[len(CASE):].T


def main(argv):
    from nasa_niswan_amd import _lib
    lib = _lib.load(argv[0])
    cases, rows = table(lib)
    # one .npy, column-major (a field changes slowly along the sweep, which is what the compression feeds on), xz-compressed
    buf = io.BytesIO()
    np.save(buf, np.ascontiguousarray(np.concatenate([cases.astype(np.int64), rows], axis=1).T))
    with lzma.open(argv[1], "wb", preset=9) as f:
        f.write(buf.getvalue())
    print(f"{len(cases)} cases, {int((rows[:, 0] != 0).sum())} of them refused, {len(FIELDS)} fields -> {argv[1]}")


if __name__ == "__main__":
    main(sys.argv[1:])
