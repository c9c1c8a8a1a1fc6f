"""The cases and data of tests/test_gpu_skill_exact.py (no test here; CPU only).  tests/test_small_audit_cpu.py proves on these
same data sets, in Python integers, that every sum of the reference is exact -- so the reference is free of any summation
order and the GPU test may ask for equal bits.

Geometry of the skill kernels (csrc/head.hip): grid = (ceil(Hc*Wc / 256) pixel blocks, ceil(O / 4) output groups), one
partial row per (sample, output, wave), NP = 4 * blocks rows folded by skill_fold_kernel in trips of 8; calls of more than
NINT_SKILL_MAX_N = 64 samples run in pieces."""
import collections

import numpy as np

from oracle import small_audit as SM

MAX_N = 64                 # include/nint.h NINT_SKILL_MAX_N
SENTINEL = np.array([0x7FF80000DEADBEEF], np.uint64).view(np.float64)[0]     # a NaN with a payload: must come back bit for bit

Plain = collections.namedtuple("Plain", "N O H W oy ox Hc Wc slots row_w")
# slots: "mod13" = SM.skill_slots (12 slots, non-monotone, -1 among them), "none" = every sample -1, None = NULL (all slot 0);
# row_w: False = NULL.  The call gets nslots = 13: slot 12 is named by no sample and holds SENTINEL.
NSLOTS = 13

PLAIN_CASES = {
    # crop                                  what it reaches
    "1x1-N1-O1-null-slot-null-roww":   Plain(1, 1, 4, 5, 2, 3, 1, 1, None, False),          # one live lane; waves 1..3 dead
    "8x8-N63-O4":                      Plain(63, 4, 11, 13, 1, 4, 8, 8, "mod13", True),      # 64 px: waves 1..3 dead
    "15x17-N64-O5":                    Plain(64, 5, 20, 23, 2, 5, 15, 17, "mod13", True),    # 255 px; one full piece; group 1 has 1 output
    "16x16-N65-O6":                    Plain(65, 6, 19, 24, 3, 1, 16, 16, "mod13", True),    # 256 px; a second piece of one sample; group 1 has 2
    "1x257-N5-O7":                     Plain(5, 7, 3, 260, 1, 2, 1, 257, "mod13", True),     # second block with ONE live lane; group 1 has 3
    "17x31-N129-O9":                   Plain(129, 9, 21, 40, 1, 6, 17, 31, "mod13", True),   # 3 blocks (NP = 12: 2nd fold trip), 3 pieces, 3 groups
    "5x461-N3-O1":                     Plain(3, 1, 7, 470, 2, 4, 5, 461, "mod13", True),     # 10 blocks, NP = 40: five fold trips
    "corner-6x10-N14-O5":              Plain(14, 5, 9, 14, 3, 0, 6, 10, "mod13", True),      # oy + Hc == H, ox == 0; every slot named
    "whole-grid-7x9-N2-O4":            Plain(2, 4, 7, 9, 0, 0, 7, 9, "mod13", True),
    "product-90x144-N2-O1":            Plain(2, 1, 100, 154, 5, 5, 90, 144, "mod13", True),  # 51 blocks, the last one ragged; NP = 204
    "17x31-N5-O5-every-slot-minus-1":  Plain(5, 5, 21, 40, 1, 6, 17, 31, "none", True),
    "17x31-N3-O6-null-slot-null-roww": Plain(3, 6, 21, 40, 1, 6, 17, 31, None, False),
}
SPLIT_CASE, SPLIT = "17x31-N129-O9", (40, 89)      # the same samples as two calls into the same pix: the same bits


def plain_slots(c):
    return {"mod13": SM.skill_slots(c.N), "none": [-1] * c.N, None: None}[c.slots]


def plain_data(name):
    """(pred, y, row_w or None, pix_before with the sentinel slot, slot list or None) of a plain case"""
    c = PLAIN_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    pred, y, row_w, before = SM.skill_int_data(rng, c.N, c.O, c.H, c.W, c.oy, c.ox, c.Hc, c.Wc, NSLOTS)
    before[NSLOTS - 1] = SENTINEL
    return pred, y, (row_w if c.row_w else None), before, plain_slots(c)


Fused = collections.namedtuple("Fused", "dt Ch O N n0 H W P oy ox Hc Wc bias")
# dt: 0 = f32 (channels padded to 16), 1 = bf16 (to 32); CHV = 32 / 64 / 128 by the padded count
FUSED_CASES = {
    "f32-chv32-Ch16-O6-17x31-n0=1":        Fused(0, 16, 6, 3, 1, 21, 40, 2, 1, 6, 17, 31, True),
    "bf16-chv32-Ch16-O5":                  Fused(1, 16, 5, 2, 0, 9, 13, 2, 2, 3, 4, 5, True),
    "f32-chv64-Ch40-Chp48-O6-17x31-no-bias": Fused(0, 40, 6, 2, 2, 21, 40, 1, 1, 6, 17, 31, False),
    "bf16-chv64-Ch64-O7-corner":           Fused(1, 64, 7, 3, 0, 9, 14, 2, 3, 0, 6, 10, True),
    "f32-chv128-Ch100-Chp112-O9":          Fused(0, 100, 9, 2, 1, 9, 13, 2, 2, 1, 5, 11, True),
    "bf16-chv128-Ch128-O4-whole-grid":     Fused(1, 128, 4, 2, 0, 7, 9, 1, 0, 0, 7, 9, True),
    "f32-chv32-Ch16-O5-N65-two-pieces-n0=1": Fused(0, 16, 5, 65, 1, 11, 13, 1, 1, 4, 8, 8, True),
    # the window in which the fused head passes hold the shape while its [O][CHV] weight image is beyond 64 KiB
    "window-bf16-Ch128-O200":              Fused(1, 128, 200, 2, 1, 9, 13, 2, 2, 1, 5, 9, True),
    "window-f32-Ch48-O300":                Fused(0, 48, 300, 2, 0, 9, 13, 2, 2, 1, 5, 9, True),
    "window-f32-Ch16-O600":                Fused(0, 16, 600, 2, 0, 9, 13, 2, 2, 1, 5, 9, True),
}


def chp_of(dt, Ch):
    kc = 32 if dt else 16
    return (Ch + kc - 1) // kc * kc


def fused_data(name):
    """(slab values (n0 + N, Hh, Wh, Chp) f32, crop h, w, b or None, y, row_w, pix_before, slots, geometry)"""
    c = FUSED_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    gt = SM.make_geom(c.H, c.W, c.P)
    slab, h, w, b = SM.skill_head_int_data(rng, c.n0, c.N, c.Ch, chp_of(c.dt, c.Ch), c.O, gt, c.oy, c.ox, c.Hc, c.Wc, c.bias)
    _, y, row_w, before = SM.skill_int_data(rng, c.N, c.O, c.Hc, c.Wc, 0, 0, c.Hc, c.Wc, NSLOTS)
    before[NSLOTS - 1] = SENTINEL
    return slab, h, w, b, y, row_w, before, SM.skill_slots(c.N), gt
