"""The evaluation skill kernels (skill_accum_kernel, head_skill_accum_kernel, skill_fold_kernel of csrc/head.hip) beyond one
pixel block: several blocks and a ragged last one, dead waves, ragged output groups, the 64-sample piece boundary, many
slots in non-monotone order, accumulation onto non-zero maps -- and the fused entry against a reference that shares no
code with the head kernels.

Part 1: integer data (tests/skill_exact_cases.py) on which every f32 and f64 partial sum is exact in any order, with or
without FMA -- tests/test_small_audit_cpu.py proves it in Python integers -- so the kernels must return the bits of the numpy
model oracle.small_audit.skill_sums: no tolerance.  Everything that must not be read is NaN (pred outside the crop window;
the halo ring, the slack, the images below n0 and the interior outside the crop window of the h slab), everything that must
be overwritten is NaN (sample, scratch, pred_out), the maps start from non-zero values and one slot that no sample names
holds a NaN with a payload that must come back bit for bit.

Part 2: standard-normal data.  The maps must still have the bits of the model (a cell grows in the documented order, one f64
operation per product and per sum); a sample row is reduced by a tree, so its error against the exact sum of its addends
(math.fsum) is held to gamma(n - 1) * sum |addends|, u = 2^-53, the bound of ANY summation order: nothing here is measured."""
import ctypes as C

import numpy as np
import pytest
import torch

import skill_exact_cases as SX
from oracle import small_audit as SM

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as pkg
    return pkg.load_library()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def i32(v):
    return None if v is None else (C.c_int32 * len(v))(*[int(a) for a in v])


def nan_scratch(lib, N, O, Hc, Wc):
    nb = lib.nint_skill_scratch_bytes(N, O, Hc, Wc)
    blocks = (Hc * Wc + 255) // 256
    assert nb == min(N, SX.MAX_N) * O * blocks * 4 * SM.SKILL_SAMPLE * 8
    return torch.full((nb // 8,), NAN, dtype=torch.float64, device="cuda"), nb


def plain_call(lib, pred, y, slots, row_w, pix, H, W, oy, ox):
    """one nint_skill_accum call on device tensors, `pix` accumulated in place; returns the sample rows (pre-filled with NaN)"""
    N, O, Hc, Wc = y.shape
    sample = torch.full((N, O, SM.SKILL_SAMPLE), NAN, dtype=torch.float64, device="cuda")
    scratch, nb = nan_scratch(lib, N, O, Hc, Wc)
    assert lib.nint_skill_accum(P(pred), P(y), i32(slots), SX.NSLOTS, P(row_w), P(pix), P(sample), P(scratch), nb, N, O, H, W,
                                oy, ox, Hc, Wc, None) == 0
    return sample


# =========================================================================== 1: integer data, equal bits
@pytest.mark.parametrize("name", list(SX.PLAIN_CASES))
def test_plain_entry_bits_on_integer_data(lib, name):
    c = SX.PLAIN_CASES[name]
    pred, y, row_w, before, slots = SX.plain_data(name)
    ref = SM.skill_sums(pred, y, c.oy, c.ox, slots, SX.NSLOTS, row_w, before)
    blocks = (c.Hc * c.Wc + 255) // 256
    print(f"  {name}: {blocks} pixel blocks (NP = {4 * blocks}), {(c.O + 3) // 4} output groups, {(c.N + SX.MAX_N - 1) // SX.MAX_N} pieces")
    pd, yd, rw, pix = dev(pred), dev(y), dev(row_w), dev(before)
    sample = plain_call(lib, pd, yd, slots, rw, pix, c.H, c.W, c.oy, c.ox)
    got_pix, got_smp = host(pix), host(sample)
    SM.check_equal(got_smp, ref["sample"], "sample")
    SM.check_equal(got_pix, ref["pix"], "pix")                     # the sentinel slot and every slot without a sample included
    if c.slots == "none":
        SM.check_equal(got_pix, before, "pix under slots of -1 only")
    if name == SX.SPLIT_CASE:                                      # the same samples as two calls into the same maps
        pix2, k = dev(before), SX.SPLIT[0]
        assert sum(SX.SPLIT) == c.N and k < SX.MAX_N < SX.SPLIT[1]
        a = plain_call(lib, pd[:k], yd[:k], slots[:k], rw, pix2, c.H, c.W, c.oy, c.ox)
        b = plain_call(lib, pd[k:], yd[k:], slots[k:], rw, pix2, c.H, c.W, c.oy, c.ox)
        SM.check_equal(host(pix2), got_pix, "pix of the split call")
        SM.check_equal(host(torch.cat([a, b])), got_smp, "sample of the split call")


def head_dispatch_is_wide(dt, Ch, O):
    chv = 32 if SX.chp_of(dt, Ch) <= 32 else (64 if SX.chp_of(dt, Ch) <= 64 else 128)
    return O * chv * 4 > 64 * 1024, (O * chv + min(O, 64) * 64) * 4 + 8192 <= 160 * 1024


@pytest.mark.parametrize("name", list(SX.FUSED_CASES))
def test_fused_entry_bits_on_integer_data_against_the_numpy_model(lib, name):
    """pred_out, pix and sample of nint_head_skill_accum against numpy (skill_head_pred + skill_sums), not against
    nint_head_fwd; with pred_out and without it."""
    from nasa_niswan_amd._lib import NintGeom
    c = SX.FUSED_CASES[name]
    slab, h, w, b, y, row_w, before, slots, gt = SX.fused_data(name)
    Chp = SX.chp_of(c.dt, c.Ch)
    assert Chp == (c.Ch + lib.nint_kc(c.dt) - 1) // lib.nint_kc(c.dt) * lib.nint_kc(c.dt)
    beyond_64k, fused_holds = head_dispatch_is_wide(c.dt, c.Ch, c.O)
    assert fused_holds and beyond_64k == name.startswith("window")
    g = NintGeom()
    assert lib.nint_geom_make(C.byref(g), c.H, c.W, c.P) == 0 and (g.H, g.W, g.P, g.Hh, g.Wh) == gt
    pred = SM.skill_head_pred(h, w, b)
    ref = SM.skill_sums(pred, y, 0, 0, slots, SX.NSLOTS, row_w, before)
    hsl = dev(slab).to(torch.bfloat16 if c.dt else torch.float32)
    assert hsl.data_ptr() % 16 == 0
    wd, bd, yd, rw = dev(w), dev(b), dev(y), dev(row_w)
    for with_pred in (True, False):
        pix = dev(before)
        sample = torch.full((c.N, c.O, SM.SKILL_SAMPLE), NAN, dtype=torch.float64, device="cuda")
        pout = torch.full((c.N, c.O, c.Hc, c.Wc), NAN, device="cuda") if with_pred else None
        scratch, nb = nan_scratch(lib, c.N, c.O, c.Hc, c.Wc)
        assert lib.nint_head_skill_accum(P(hsl), c.n0, c.N, c.Ch, Chp, c.O, P(wd), P(bd), P(yd), i32(slots), SX.NSLOTS, P(rw), P(pix),
                                         P(sample), P(pout), P(scratch), nb, C.byref(g), c.oy, c.ox, c.Hc, c.Wc, c.dt, None) == 0
        if with_pred:
            SM.check_equal(host(pout), pred, "pred_out")
        SM.check_equal(host(sample), ref["sample"], f"sample (pred_out {'given' if with_pred else 'NULL'})")
        SM.check_equal(host(pix), ref["pix"], f"pix (pred_out {'given' if with_pred else 'NULL'})")


# =========================================================================== 2: random data, the any-order bound
RANDOM_CASES = {"17x31-N65-O5": SX.Plain(65, 5, 21, 40, 1, 6, 17, 31, "mod13", True),
                "product-90x144-N2-O1": SX.Plain(2, 1, 100, 154, 5, 5, 90, 144, None, True)}


@pytest.mark.parametrize("name", list(RANDOM_CASES))
def test_plain_entry_on_random_data_within_the_any_order_bound(lib, name):
    c = RANDOM_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    pred = np.full((c.N, c.O, c.H, c.W), np.nan, np.float32)
    pred[:, :, c.oy:c.oy + c.Hc, c.ox:c.ox + c.Wc] = rng.standard_normal((c.N, c.O, c.Hc, c.Wc))
    y = rng.standard_normal((c.N, c.O, c.Hc, c.Wc)).astype(np.float32)
    row_w = 0.25 + rng.random(c.Hc)
    before = np.zeros((SX.NSLOTS, SM.SKILL_PIX, c.O, c.Hc, c.Wc))
    before[SX.NSLOTS - 1] = SX.SENTINEL
    slots = SX.plain_slots(c)
    pix = dev(before)
    sample = plain_call(lib, dev(pred), dev(y), slots, dev(row_w), pix, c.H, c.W, c.oy, c.ox)
    got_pix, got_smp = host(pix), host(sample)
    r = SM.skill_audit(pred, y, c.oy, c.ox, slots, SX.NSLOTS, row_w, before, got_pix, got_smp, name)
    print(f"  {name}: largest err / (gamma(n-1) sum|terms|): maps {r[0]:.3e} (n <= {c.N}), sample rows {r[1]:.3e} (n = {c.Hc * c.Wc}, "
          f"gamma = {SM.gamma(c.Hc * c.Wc - 1, SM.U64):.3e})")
    assert r[0] <= 1.0 and r[1] <= 1.0
    # a map cell grows in sample order, one f64 operation per product and per sum: the model's bits
    SM.check_equal(got_pix, SM.skill_sums(pred, y, c.oy, c.ox, slots, SX.NSLOTS, row_w, before)["pix"], "pix in sample order")
