"""GPU tests of the per-cell weighted training loss (cos-latitude weights and masks): the three ``_weighted`` entry points at
the C ABI against the f64 host model of tests/weighted_loss_model.py, against their unweighted twins (unit weights: bit for
bit) and against each other (fused pass = the three separate launches, bit for bit); ``FusedTrainer(loss_weights=...)``
against the oracle fit loop; ``CropMSEL1Loss`` on the autograd path; ``train.py --lat-weighted-loss --loss-weights``.

Every case uses the map ``weighted_loss_model.wmap(Hc, Wc)``: cos(latitude) rows times a column profile, the first row, the
last column and (from 8 x 8 up) an interior block masked, at least half of the cells live.  The shapes, cases and helpers of
the existing suites are reused as they are: the dispatch branches of tests/test_gpu_small_branches.py (FUSED_CASES) and
the models, targets and tolerances of tests/test_gpu_seq_train.py (S1, S3o, HeadCase, check_grad)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_seq_train as ST
import test_gpu_small_branches as SB
import weighted_loss_model as WM
from oracle import small_audit as SM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
P, dev, host = SB.P, SB.dev, SB.host
E_SHAPE = -2
BEFORE = np.array([1.0, 2.0, -3.0, 4.0, 5.0, 6.0, -7.0, 8.0])


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as pkg
    return pkg.load_library()


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


def bits(t):
    """the bytes of a device tensor, for bit-for-bit comparisons (NaN-safe, -0 != +0)"""
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def stats_close(a, b, mags, what):
    """two accumulations of the same terms in different orders: each within 1e-14 of the magnitude its roundings are relative
    to -- the value itself for the sums of non-negative terms, the count, the loss and R2; the sum of |w y| for the signed
    sum [2] (as oracle.small_audit.check_stats does)."""
    a, b = host(a), host(b)
    ref = np.maximum(np.abs(a), np.abs(b))
    ref[2] = max(ref[2], mags)
    err = np.abs(a - b)
    print(f"  {what}: stats relative differences {err / np.where(ref > 0, ref, 1.0)}")
    assert np.isfinite(a).all() and np.isfinite(b).all() and (err <= 1e-14 * ref).all(), (what, a, b)


def outside_mask(H, W, oy, ox, w):
    """(H, W) bool: outside the crop or under a zero weight"""
    m = np.ones((H, W), bool)
    m[oy:oy + w.shape[0], ox:ox + w.shape[1]] = (w == 0)
    return m


# =========================================================================== 1: the stand-alone kernel against the f64 model
LOSS_SHAPES = [pytest.param(2, 3, 12, 20, 1, 2, 10, 16, id="asymmetric-crop"),
               pytest.param(2, 3, 9, 11, 0, 0, 9, 11, id="full-image"),
               pytest.param(6, 3, 100, 154, 5, 5, 90, 144, id="grid-stride-twice[277200>256*1024]")]


def crop_weighted(lib, pd, yd, wd, wsum, dp, sc, st, shape):
    N, O, H, W, oy, ox, Hc, Wc = shape
    assert lib.nint_loss_mse_l1_crop_weighted(P(pd), P(yd), P(wd), wsum, P(dp), P(sc), P(st), N, O, H, W, oy, ox, Hc, Wc, None) == 0


def loss_case(shape, seed=60):
    N, O, H, W, oy, ox, Hc, Wc = shape
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((N, O, H, W)).astype(f32)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(f32)
    w = WM.wmap(Hc, Wc)
    assert w[1, 0] > 0
    pred[0, 0, oy + 1, ox] = y[0, 0, 1, 0]                           # sign(0) = 0 on a live cell
    return pred, y, w, WM.wsum_of(w)


@pytest.mark.parametrize("N,O,H,W,oy,ox,Hc,Wc", LOSS_SHAPES)
def test_weighted_loss_kernel_against_the_f64_model(lib, N, O, H, W, oy, ox, Hc, Wc):
    """dpred within 2^-22 |ref| elementwise (one f32 rounding of d, |2d| <= |2d + sgn d|, plus the final rounding: 2^-24
    relative each; the f64 operations between them are far below), exactly +0 outside the crop and under a zero weight; the
    loss and the eight stats, accumulated onto non-zero stats, within oracle.small_audit's tolerances for the unweighted
    kernel; two runs bit-equal; dpred = NULL and stats = NULL."""
    shape = (N, O, H, W, oy, ox, Hc, Wc)
    if N * O * H * W > 256 * 1024:
        assert N * O * H * W <= 2 * 256 * 1024                       # LOSS_BLOCKS x 1024 threads: the grid-stride loop runs twice
    pred, y, w, wsum = loss_case(shape)
    ref = WM.loss(pred, y, w, oy, ox)
    pd, yd, wd = dev(pred), dev(y), dev(w)
    runs = []
    for _ in range(2):
        dp, sc, st = torch.full((N, O, H, W), 7.0, device="cuda"), torch.zeros(8194, device="cuda"), dev(BEFORE)
        crop_weighted(lib, pd, yd, wd, wsum, dp, sc, st, shape)
        runs.append((dp, sc[:1].clone(), st))
    dp, loss, st = runs[0]
    got = host(dp)
    err = np.abs(got.astype(np.float64) - ref["dpred"].astype(np.float64))
    bound = 2.0 ** -22 * np.abs(ref["dpred"].astype(np.float64))
    print(f"  dpred: max err / bound {float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))):.3f}, "
          f"{int((got != ref['dpred']).sum())} of {got.size} differ from the model's f32 value")
    assert np.isfinite(got).all() and (err <= bound).all()
    zero = outside_mask(H, W, oy, ox, w)
    assert not got.view(np.uint32)[:, :, zero].any()                # +0: no bit set
    assert (got[:, :, ~zero] != 0).sum() >= got[:, :, ~zero].size - 1   # every live cell carries a gradient (but the one d = 0)
    r1 = SM.check_loss_scalar(host(loss)[0], ref["loss"], what="weighted loss")
    r2 = SM.check_stats(BEFORE, host(st), [ref], what="weighted stats")
    print(f"  loss {float(host(loss)[0])!r} model {ref['loss']!r}; worst ratio loss {r1:.3f}, stats {r2:.3f}")
    assert all(same_bits(a, b) for a, b in zip(runs[0], runs[1]))
    sc = torch.zeros(8194, device="cuda")
    crop_weighted(lib, pd, yd, wd, wsum, None, sc, None, shape)
    assert same_bits(sc[:1], loss)


# =========================================================================== the fused entry points' inputs
def fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc):
    """SB.head_inputs' slab (random halo and slack, images below n0 included) plus targets and the map"""
    g, Chp, hsl, h, w, b, rng = SB.head_inputs(lib, dt, Ch, O, N, n0, H, W, 2, 40 + Ch + O)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(f32)
    wm = WM.wmap(Hc, Wc)
    return g, Chp, hsl, h, w, b, y, wm


def run_fused(lib, weighted, hsl, n0, N, Ch, Chp, O, wd, bd, yd, wgt, wsum, g, oy, ox, Hc, Wc, dt, H, W, st0=None):
    dp = torch.full((N, O, H, W), 7.0, device="cuda")
    dh = torch.full((N, H, W, Chp), 7.0, device="cuda").to(SB.et(dt))
    sc, st = torch.zeros(8194, device="cuda"), dev(np.zeros(8) if st0 is None else st0)
    if weighted:
        rc = lib.nint_head_loss_fused_weighted(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(yd), P(wgt), wsum, P(dp), P(dh), P(sc),
                                               P(st), C.byref(g), oy, ox, Hc, Wc, dt, None)
    else:
        rc = lib.nint_head_loss_fused(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(yd), P(dp), P(dh), P(sc), P(st), C.byref(g),
                                      oy, ox, Hc, Wc, dt, None)
    assert rc == 0
    return dp, dh, sc[:1].clone(), st


def grad_check(got, ref, what, bf16=False):
    """the project's standing gradient tolerances (tests/test_gpu_parity.py header): f32 max-abs error <= 1e-3 max|ref| + 1e-6;
    values stored in bf16: rel-L2 <= 2e-2"""
    ST.check_grad(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(ref)), what, "bf16" if bf16 else "f32")


# =========================================================================== 4: fused = the three launches; the f64 model
@pytest.mark.parametrize("dt,Ch,O,N,n0,H,W,oy,ox,Hc,Wc,want_chv,tags", SB.FUSED_CASES)
def test_fused_weighted_equals_the_three_launches_bit_for_bit(lib, dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, want_chv, tags):
    """nint_head_loss_fused_weighted against nint_head_fwd -> nint_loss_mse_l1_crop_weighted -> nint_head_bwd at every
    dispatch branch of the fused pass (test_gpu_small_branches.FUSED_CASES asserts that each shape reaches its branch): dpred,
    dh and the f32 loss bit for bit, the stats to 1e-14 (the f64 partial sums are folded in another order).  Then dpred and dh
    against the f64 model from the stored slab, with the standing gradient tolerances."""
    Chp, chv, _, _, _ = SB.head_dispatch(dt, Ch, O)
    assert chv == want_chv and Chp <= 128
    g, Chp, hsl, h, w, b, y, wm = fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc)
    wsum = WM.wsum_of(wm)
    wd, bd, yd, wgt = dev(w), dev(b), dev(y), dev(wm)
    dp2, dh2, loss2, st2 = run_fused(lib, True, hsl, n0, N, Ch, Chp, O, wd, bd, yd, wgt, wsum, g, oy, ox, Hc, Wc, dt, H, W)
    pred = torch.full((N, O, H, W), 7.0, device="cuda")
    assert lib.nint_head_fwd(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(pred), C.byref(g), dt, None) == 0
    dp1, sc1, st1 = torch.full((N, O, H, W), 7.0, device="cuda"), torch.zeros(8194, device="cuda"), dev(np.zeros(8))
    crop_weighted(lib, pred, yd, wgt, wsum, dp1, sc1, st1, (N, O, H, W, oy, ox, Hc, Wc))
    dh1 = torch.full((N, H, W, Chp), 7.0, device="cuda").to(SB.et(dt))
    assert lib.nint_head_bwd(P(hsl), n0, N, Ch, Chp, O, P(wd), P(dp1), P(dh1), None, None, C.byref(g), dt, None, 0, None) == 0
    torch.cuda.synchronize()
    print(f"  loss fused {float(loss2[0])!r} three launches {float(sc1[0])!r}")
    assert same_bits(dp1, dp2) and same_bits(dh1, dh2) and same_bits(sc1[:1], loss2)
    stats_close(st1, st2, float(np.sum(np.abs(y.astype(np.float64)) * wm)), "fused against three launches")
    assert host(st2)[4] == N * O * wsum and host(st2)[7] == 1.0
    # the f64 model
    rdp, rdh, rloss = WM.head_loss_fused(h, w, b, y, wm, oy, ox)
    got_dp, got_dh = host(dp2), SB.decode(dh2, dt)
    assert not got_dp.view(np.uint32)[:, :, outside_mask(H, W, oy, ox, wm)].any()
    assert not got_dh[..., Ch:].any()                               # the channel padding
    grad_check(got_dp, rdp, "fused weighted dpred")
    grad_check(got_dh[..., :Ch], rdh, "fused weighted dh", bool(dt))
    assert abs(float(loss2[0]) - rloss) <= 1e-4 * abs(rloss) + 1e-5  # (the output tolerance; the bit-level statement is above)


def seq_case(pkg, Ch, O, dtype):
    hc = ST.HeadCase(pkg, Ch, O, dtype)
    gen = torch.Generator().manual_seed(77 + Ch + O)
    y = torch.randn(hc.B, hc.T, O, *ST.CROP, generator=gen).cuda()
    wm = WM.wmap(*ST.CROP)
    return hc, y, wm, dev(wm), WM.wsum_of(wm)


def run_seq_fused(hc, weighted, y, wgt, wsum, st0=None):
    (oy, ox), (Hc, Wc) = ST.HALO, ST.CROP
    dp = torch.full((hc.T * hc.B, hc.O, hc.H, hc.W), 7.0, device="cuda")
    dh = torch.full((hc.T * hc.B * hc.H * hc.W * hc.Chp * hc.es,), 0xAB, dtype=torch.uint8, device="cuda")
    sc, st = torch.zeros(8194, device="cuda"), dev(np.zeros(8) if st0 is None else st0)
    a = (P(hc.slab), hc.B, hc.T, hc.Ch, hc.Chp, hc.O, P(hc.w), P(hc.b), P(y))
    z = (P(dp), P(dh), P(sc), P(st), C.byref(hc.g), oy, ox, Hc, Wc, hc.dt, None)
    rc = hc.lib.nint_head_loss_seq_fused_weighted(*a, P(wgt), wsum, *z) if weighted else hc.lib.nint_head_loss_seq_fused(*a, *z)
    return rc, dp, dh, sc[:1].clone(), st


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Ch,O", [(Ch, O) for Ch in (8, 40, 72) for O in (1, 3)] + [(72, 200)] +
                         [(32, 3), (64, 3), (128, 3)])    # (Ch = CHV: data in the 12 staged channels the dot product leaves unfused)
def test_seq_fused_weighted_equals_the_three_launches_bit_for_bit(pkg, Ch, O, dtype):
    """The sequence form (B = 2, T = 3, 12 x 20; the 32-, 64- and 128-channel bodies; 200 outputs at 72 channels: a weight image
    beyond 64 KiB that the fused pass still holds): nint_head_loss_seq_fused_weighted against
    nint_head_fwd_seq -> nint_loss_mse_l1_crop_weighted (N = B, O' = T*O) -> nint_head_bwd_seq; dpred is in image order t*B + b
    there and (B, T*O, H, W) here.  dpred also against the f64 model from the stored slab."""
    hc, y, wm, wgt, wsum = seq_case(pkg, Ch, O, dtype)
    (oy, ox), (Hc, Wc) = ST.HALO, ST.CROP
    B, T, H, W = hc.B, hc.T, hc.H, hc.W
    rc, dp2, dh2, loss2, st2 = run_seq_fused(hc, True, y, wgt, wsum)
    assert rc == 0
    seq = hc.fwd_seq()
    dseq, sc1, st1 = torch.full_like(seq, 7.0), torch.zeros(8194, device="cuda"), dev(np.zeros(8))
    crop_weighted(hc.lib, seq, y, wgt, wsum, dseq, sc1, st1, (B, T * O, H, W, oy, ox, Hc, Wc))
    dh1, _, _ = hc.bwd_seq(dseq, None)
    torch.cuda.synchronize()
    print(f"  loss fused {float(loss2[0])!r} three launches {float(sc1[0])!r}")
    assert same_bits(dp2.view(T, B, O, H, W).permute(1, 0, 2, 3, 4).contiguous(), dseq.view(B, T, O, H, W))
    assert same_bits(dh1, dh2) and same_bits(sc1[:1], loss2)
    stats_close(st1, st2, float(np.sum(np.abs(y.double().cpu().numpy()) * wm)), "seq fused against three launches")
    assert host(st2)[4] == T * B * O * wsum
    # f64 model: pred (B, T, O, H, W) from the stored slab
    pred = torch.einsum("oc,tbcyx->btoyx", hc.w.double().cpu(), hc.h) + hc.b.double().cpu().view(1, 1, O, 1, 1)
    d = pred[..., oy:oy + Hc, ox:ox + Wc].numpy() - y.double().cpu().numpy()
    want = np.zeros((B, T, O, H, W))
    want[..., oy:oy + Hc, ox:ox + Wc] = (2 * d + np.sign(d)) * wm.astype(np.float64) / (T * B * O * wsum)
    got = host(dseq).reshape(B, T, O, H, W)
    assert not got.view(np.uint32)[..., outside_mask(H, W, oy, ox, wm)].any()
    grad_check(got, want, f"seq fused weighted dpred Ch={Ch} O={O} {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_weighted_entries_refuse_more_than_128_padded_channels(pkg, dtype):
    hc, y, wm, wgt, wsum = seq_case(pkg, 136, 1, dtype)
    assert hc.Chp > 128
    rc, _, _, _, _ = run_seq_fused(hc, True, y, wgt, wsum)
    assert rc == E_SHAPE
    (oy, ox), (Hc, Wc) = ST.HALO, ST.CROP
    a = P(hc.slab)
    assert hc.lib.nint_head_loss_fused_weighted(a, hc.B, hc.B, hc.Ch, hc.Chp, hc.O, P(hc.w), P(hc.b), P(y), P(wgt), wsum, a, a, a, None,
                                                C.byref(hc.g), oy, ox, Hc, Wc, hc.dt, None) == E_SHAPE


# =========================================================================== 2: NaN targets under the mask
def test_nan_targets_under_the_mask_change_nothing(lib, pkg):
    """y = NaN wherever w == 0: loss, dpred, dh and stats stay finite and keep the bits of the run with finite targets, for the
    stand-alone, the fused and the sequence entry."""
    shape = (2, 3, 12, 20, 1, 2, 10, 16)
    N, O, H, W, oy, ox, Hc, Wc = shape
    pred, y, w, wsum = loss_case(shape, 61)
    y_nan = y.copy()
    y_nan[:, :, w == 0] = np.nan
    assert np.isnan(y_nan).sum() == N * O * 40
    pd, wd = dev(pred), dev(w)
    out = []
    for yy in (y, y_nan):
        dp, sc, st = torch.full((N, O, H, W), 7.0, device="cuda"), torch.zeros(8194, device="cuda"), dev(BEFORE)
        crop_weighted(lib, pd, dev(yy), wd, wsum, dp, sc, st, shape)
        out.append((dp, sc[:1].clone(), st))
    assert all(torch.isfinite(t).all() for t in out[1]) and all(same_bits(a, b) for a, b in zip(*out))
    # fused: two branches of FUSED_CASES (f32 CHV 32 with n0 = 1, bf16 CHV 64 with two output chunks)
    for case in (SB.FUSED_CASES[0], SB.FUSED_CASES[3]):
        dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, _, _ = case.values
        g, Chp, hsl, h, wh, b, y, wm = fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc)
        y_nan = y.copy()
        y_nan[:, :, wm == 0] = np.nan
        assert np.isnan(y_nan).any()
        wd, bd, wgt = dev(wh), dev(b), dev(wm)
        out = [run_fused(lib, True, hsl, n0, N, Ch, Chp, O, wd, bd, dev(yy), wgt, WM.wsum_of(wm), g, oy, ox, Hc, Wc, dt, H, W, BEFORE)
               for yy in (y, y_nan)]
        assert all(torch.isfinite(t.float()).all() for t in out[1]) and all(same_bits(a, b) for a, b in zip(*out)), case.id
    # sequence
    hc, y, wm, wgt, wsum = seq_case(pkg, 40, 3, "bf16")
    y_nan = y.clone()
    y_nan[..., torch.from_numpy(wm == 0).cuda()] = float("nan")
    assert torch.isnan(y_nan).any()
    out = [run_seq_fused(hc, True, yy, wgt, wsum, BEFORE)[1:] for yy in (y, y_nan)]
    vals = hc.dh_values(out[1][1])
    assert torch.isfinite(vals).all() and all(torch.isfinite(t).all() for t in (out[1][0], out[1][2], out[1][3]))
    assert all(same_bits(a, b) for a, b in zip(*out))


# =========================================================================== 3: unit weights = the unweighted twin
@pytest.mark.parametrize("N,O,H,W,oy,ox,Hc,Wc", LOSS_SHAPES)
def test_unit_weights_are_the_unweighted_loss_bit_for_bit(lib, N, O, H, W, oy, ox, Hc, Wc):
    shape = (N, O, H, W, oy, ox, Hc, Wc)
    pred, y, _, _ = loss_case(shape, 62)
    pd, yd, ones = dev(pred), dev(y), torch.ones(Hc, Wc, device="cuda")
    dp1, sc1, st1 = torch.full((N, O, H, W), 7.0, device="cuda"), torch.zeros(8194, device="cuda"), dev(BEFORE)
    assert lib.nint_loss_mse_l1_crop(P(pd), P(yd), P(dp1), P(sc1), P(st1), N, O, H, W, oy, ox, Hc, Wc, None) == 0
    dp2, sc2, st2 = torch.full((N, O, H, W), 7.0, device="cuda"), torch.zeros(8194, device="cuda"), dev(BEFORE)
    crop_weighted(lib, pd, yd, ones, float(Hc * Wc), dp2, sc2, st2, shape)
    torch.cuda.synchronize()
    assert torch.equal(dp1, dp2) and torch.equal(sc1[:1], sc2[:1]) and torch.equal(st1, st2)
    assert same_bits(dp1, dp2) and same_bits(st1, st2)


@pytest.mark.parametrize("dt,Ch,O,N,n0,H,W,oy,ox,Hc,Wc,want_chv,tags", SB.FUSED_CASES)
def test_unit_weights_are_the_unweighted_fused_pass_bit_for_bit(lib, dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, want_chv, tags):
    g, Chp, hsl, h, w, b, y, _ = fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc)
    wd, bd, yd, ones = dev(w), dev(b), dev(y), torch.ones(Hc, Wc, device="cuda")
    a = run_fused(lib, False, hsl, n0, N, Ch, Chp, O, wd, bd, yd, None, 0.0, g, oy, ox, Hc, Wc, dt, H, W, BEFORE)
    b2 = run_fused(lib, True, hsl, n0, N, Ch, Chp, O, wd, bd, yd, ones, float(Hc * Wc), g, oy, ox, Hc, Wc, dt, H, W, BEFORE)
    for x, z, name in zip(a, b2, ("dpred", "dh", "loss", "stats")):
        assert torch.equal(x, z) and same_bits(x, z), name


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Ch,O", [(8, 1), (40, 3), (72, 3)])
def test_unit_weights_are_the_unweighted_sequence_pass_bit_for_bit(pkg, Ch, O, dtype):
    hc, y, _, _, _ = seq_case(pkg, Ch, O, dtype)
    ones = torch.ones(*ST.CROP, device="cuda")
    a = run_seq_fused(hc, False, y, None, 0.0, BEFORE)
    b = run_seq_fused(hc, True, y, ones, float(ST.CROP[0] * ST.CROP[1]), BEFORE)
    assert a[0] == 0 and b[0] == 0
    for x, z, name in zip(a[1:], b[1:], ("dpred", "dh_seq", "loss", "stats")):
        assert torch.equal(x, z), name


# =========================================================================== 5: the trainer against the oracle fit loop
B, T, H, W = ST.B, ST.T, ST.H, ST.W
HALO, CROP, LR, BETAS = ST.HALO, ST.CROP, ST.LR, ST.BETAS


def targets(shape, sq):
    y = ST.trainer_targets(shape)
    return y if sq else y[:, -1].contiguous()


@functools.lru_cache(maxsize=None)
def oracle_steps(shape, sq, nsteps=3):
    """test_gpu_seq_train.oracle_seq_steps with the weighted loss (and the last step's output alone without `sq`): CPU autograd
    of weighted_loss_model.loss_torch on convlstm_oracle.convlstm_forward, then adam_step_numpy.  Per step: loss, gradients,
    parameters after the step, the cropped output before it."""
    from oracle import convlstm_oracle as O
    params, X, _, _ = ST.case_data(shape)
    yv = targets(shape, sq).reshape(B, -1, *CROP)
    w = WM.wmap(*CROP)
    p = params
    st = {"m": {k: torch.zeros_like(v) for k, v in p.items()}, "v": {k: torch.zeros_like(v) for k, v in p.items()}}
    out = []
    for step in range(1, nsteps + 1):
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
        pred, seq = O.convlstm_forward(X, leaf, return_sequence=True)
        full = seq if sq else pred
        loss = WM.loss_torch(full, yv, w, HALO[0], HALO[1])
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in leaf.items()}
        newp, m, v = {}, {}, {}
        for k in p:
            a, b_, c = O.adam_step_numpy(p[k].numpy(), grads[k].numpy(), st["m"][k].numpy(), st["v"][k].numpy(), step, LR, BETAS)
            newp[k], m[k], v[k] = torch.from_numpy(a), torch.from_numpy(b_), torch.from_numpy(c)
        p, st = newp, {"m": m, "v": v}
        out.append(dict(loss=float(loss.detach()), grads=grads, params=p, crop=O.crop_pred(full, HALO, CROP).detach()))
    return out


def make_trainer(pkg, shape, dtype, sq, fallback, weights):
    from nasa_niswan_amd.trainer import FusedTrainer
    params, X, _, _ = ST.case_data(shape)
    cin, hidden, ks, out = ST.SHAPES[shape]
    net = pkg.ConvLSTM(cin, hidden, ks, len(hidden), out_channels=out, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, sequence_loss=sq, loss_weights=weights)
    eng = net._engine(torch.device("cuda", 0))
    name = "head_loss_seq_fused" if sq else "head_loss_fused"
    calls, real = [], getattr(eng, name)

    def spy(*a, **k):
        calls.append(False if fallback else real(*a, **k))
        return calls[-1]
    setattr(eng, name, spy)
    return net, tr, calls


@pytest.mark.parametrize("fallback", [False, True], ids=["fused", "three-launch"])
@pytest.mark.parametrize("sq", [False, True], ids=["last-step", "sequence-loss"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ["S1", "S3o"])
def test_weighted_step_matches_the_oracle_fit_loop(pkg, shape, dtype, sq, fallback):
    """Three steps at lr 1e-4, betas (0.5, 0.999) with the weighted loss, through the fused head / loss pass and through the
    three-launch fallback, on the last step's output and on every step's.  The tolerances are those of
    test_gpu_seq_train.test_fused_sequence_step_matches_the_oracle_fit_loop (derived there): loss 1e-4 rel + 1e-5 (f32) / 2e-2
    (bf16); bucket gradients the standing ones; parameters max |dp| <= k * 2.2 * lr, mean 2e-6 (f32) / 0.1 * lr * k (bf16).  In
    f32 epoch_stats() is the mean of the per-step losses and of the per-step weighted r2_score."""
    params, X, _, _ = ST.case_data(shape)
    y = targets(shape, sq)
    want = oracle_steps(shape, sq)
    wm = WM.wmap(*CROP)
    net, tr, calls = make_trainer(pkg, shape, dtype, sq, fallback, wm)
    Xd, yd = X.cuda(), y.cuda()
    names = [k for k, _ in net.named_parameters()]
    for step in (1, 2, 3):
        loss = float(tr.step(Xd, yd))
        o = want[step - 1]
        print(f"  {shape} {dtype} step {step}: loss {loss:.7f} oracle {o['loss']:.7f}")
        if dtype == "f32":
            assert abs(loss - o["loss"]) <= 1e-4 * abs(o["loss"]) + 1e-5
        else:
            assert abs(loss - o["loss"]) <= 2e-2 * abs(o["loss"])
        if step == 1:
            for i, k in enumerate(names):
                ST.check_grad(tr.flat.grad_view(i).view(o["grads"][k].shape), o["grads"][k], f"{shape} {dtype} bucket d{k}", dtype)
        if step in (1, 3):
            for k, v in net.state_dict().items():
                d = (v.cpu() - o["params"][k]).abs()
                print(f"    after {step}: {k}: max |dp| {float(d.max()):.2e}, mean {float(d.mean()):.2e}")
                assert float(d.max()) <= step * 2.2 * LR, (k, step)
                assert float(d.mean()) <= (2e-6 if dtype == "f32" else 0.1 * LR * step), (k, step)
    assert calls == [not fallback] * 3                        # the path the case is about did run
    if dtype == "f32":
        loss_e, r2_e = tr.epoch_stats()
        yv = y.reshape(B, -1, *CROP).numpy()
        want_r2 = np.mean([WM.r2_weighted(yv, o["crop"].numpy(), wm) for o in want])
        want_loss = np.mean([o["loss"] for o in want])
        print(f"  epoch stats: loss {loss_e:.7f} (oracle {want_loss:.7f}), R2 {r2_e:.7f} (oracle {want_r2:.7f})")
        assert abs(loss_e - want_loss) <= 1e-4 * abs(want_loss) + 1e-5 and abs(r2_e - want_r2) <= 1e-4 * abs(want_r2) + 1e-5
    # evaluate() uses the map too: its statistics are the host model's on the prediction it returns (f64 sums of some 1e3
    # terms from f32 inputs: 1e-9 relative is far above their roundings and far below the unweighted figures)
    tr.reset_stats()
    full = tr.evaluate(Xd, yd)
    ref = WM.loss(host(full), y.reshape(B, -1, *CROP).numpy(), wm, HALO[0], HALO[1])
    le, r2e = tr.epoch_stats()
    print(f"  evaluate: loss {le!r} (model {ref['loss']!r}), R2 {r2e!r} (model {ref['r2']!r})")
    assert abs(le - ref["loss"]) <= 1e-9 * abs(ref["loss"]) and abs(r2e - ref["r2"]) <= 1e-9 * (1.0 + abs(ref["r2"]))


def one_step(pkg, weights, sq=False, dtype="f32", shape="S3o", switch=()):
    params, X, _, _ = ST.case_data(shape)
    net, tr, _ = make_trainer(pkg, shape, dtype, sq, False, weights)
    for w in switch:
        tr.set_loss_weights(w)
    loss = tr.step(X.cuda(), targets(shape, sq).cuda()).clone()
    return net, tr, loss


@pytest.mark.parametrize("sq", [False, True], ids=["last-step", "sequence-loss"])
def test_row_weight_vector_gives_the_bits_of_its_broadcast_map(pkg, sq):
    rows = np.cos(np.deg2rad(-90.0 + (np.arange(CROP[0]) + 0.5) * (180.0 / CROP[0]))).astype(f32)
    rows[0] = 0
    na, ta, la = one_step(pkg, rows, sq)
    nb, tb, lb = one_step(pkg, np.repeat(rows[:, None], CROP[1], axis=1), sq)
    assert same_bits(la, lb) and same_bits(ta.flat.grad, tb.flat.grad) and same_bits(ta.flat.data, tb.flat.data)
    assert same_bits(ta.stats, tb.stats) and torch.isfinite(ta.flat.data).all()
    with pytest.raises(ValueError):
        one_step(pkg, np.ones(CROP[0] + 1, f32), sq)              # the shape is checked against the target's crop at the first step
    with pytest.raises(ValueError):
        one_step(pkg, np.ones((CROP[1], CROP[0]), f32), sq)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("sq", [False, True], ids=["last-step", "sequence-loss"])
def test_set_loss_weights_none_returns_to_the_unweighted_bits(pkg, sq, dtype):
    wm = WM.wmap(*CROP)
    na, ta, la = one_step(pkg, wm, sq, dtype, switch=(None,))
    nb, tb, lb = one_step(pkg, None, sq, dtype)
    assert same_bits(la, lb) and same_bits(ta.flat.grad, tb.flat.grad) and same_bits(ta.flat.data, tb.flat.data) and same_bits(ta.stats, tb.stats)
    # ... and switching the map on between steps is the trainer that had it from the start
    nc, tc, lc = one_step(pkg, None, sq, dtype, switch=(wm,))
    nd, td, ld = one_step(pkg, wm, sq, dtype)
    assert same_bits(lc, ld) and same_bits(tc.flat.grad, td.flat.grad) and same_bits(tc.flat.data, td.flat.data)
    assert not same_bits(lc, lb)                                  # (the weighted loss is another number)


@pytest.mark.parametrize("sq", [False, True], ids=["last-step", "sequence-loss"])
def test_a_masked_region_gets_exactly_zero_dpred_while_the_parameters_move(pkg, sq):
    mask = np.ones(CROP, f32)
    mask[2:7, 3:11] = 0
    params, _, _, _ = ST.case_data("S3o")
    net, tr, loss = one_step(pkg, mask, sq)
    dp = tr._dpred.view(-1, H, W)
    region = dp[:, HALO[0] + 2:HALO[0] + 7, HALO[1] + 3:HALO[1] + 11]
    assert not bits(region).any()                                 # +0 in every image and output
    live = dp[:, HALO[0] + 7:HALO[0] + CROP[0], HALO[1]:HALO[1] + CROP[1]]
    assert (live != 0).all() and torch.isfinite(loss)
    moved = [k for k, v in net.state_dict().items() if not torch.equal(v.cpu(), params[k])]
    assert len(moved) == len(params), moved


# =========================================================================== 6: CropMSEL1Loss on the autograd path
def test_crop_mse_l1_loss_module_against_the_oracle_and_torch(pkg):
    """criterion(y, net(X)).backward() with the map: the oracle's weighted gradients (step 1 of oracle_steps, S1, f32) with
    the standing tolerances.  Without a map: torch's MSELoss + L1Loss on the crop.  An upstream factor is honoured."""
    from nasa_niswan_amd.loss import CropMSEL1Loss
    params, X, _, _ = ST.case_data("S1")
    y = targets("S1", False)
    cin, hidden, ks, out = ST.SHAPES["S1"]
    wm = WM.wmap(*CROP)
    o = oracle_steps("S1", False)[0]

    def grads(criterion, factor=1.0):
        net = pkg.ConvLSTM(cin, hidden, ks, len(hidden), out_channels=out, compute_dtype="f32").cuda()
        net.load_state_dict(params)
        loss = criterion(y.cuda(), net(X.cuda()))
        (factor * loss).backward()
        return float(loss.detach()), {k: p.grad.detach().cpu() for k, p in net.named_parameters()}

    loss, g = grads(CropMSEL1Loss(HALO, weights=wm))
    assert abs(loss - o["loss"]) <= 1e-4 * abs(o["loss"]) + 1e-5
    for k in sorted(g):
        ST.check_grad(g[k], o["grads"][k], f"CropMSEL1Loss weighted d{k}")
    loss3, g3 = grads(CropMSEL1Loss(HALO, weights=wm), 3.0)
    assert loss3 == loss
    for k in sorted(g):
        ST.check_grad(g3[k], 3.0 * o["grads"][k], f"CropMSEL1Loss weighted, upstream 3, d{k}")
    # the gradient handed to pred is dpred * upstream, exactly; y gets none
    pl = torch.randn(B, out, H, W, device="cuda").requires_grad_(True)
    yl = y.cuda().requires_grad_(True)
    crit = CropMSEL1Loss(HALO, weights=wm)
    crit(yl, pl).backward()
    g1 = pl.grad.clone()
    pl.grad = None
    (3.0 * crit(yl, pl)).backward()
    assert torch.equal(pl.grad, g1 * 3.0) and yl.grad is None
    assert not bits(g1[:, :, torch.from_numpy(outside_mask(H, W, HALO[0], HALO[1], wm)).cuda()]).any()
    # weights=None: torch's own criteria on the crop (reference train.py:74-75,102,105)
    def torch_criterion(yy, pred):
        pc = pred[:, :, HALO[0]:HALO[0] + CROP[0], HALO[1]:HALO[1] + CROP[1]].squeeze(1)
        return torch.nn.MSELoss()(yy, pc) + torch.nn.L1Loss()(yy, pc)
    l0, g0 = grads(CropMSEL1Loss(HALO))
    lt, gt = grads(torch_criterion)
    assert abs(l0 - lt) <= 1e-4 * abs(lt) + 1e-5
    for k in sorted(g0):
        ST.check_grad(g0[k], gt[k], f"CropMSEL1Loss unweighted against torch d{k}")


# =========================================================================== 7: train.py
def test_train_py_weighted_loss_end_to_end(pkg, tmp_path):
    """train.py --lat-weighted-loss --loss-weights m.npy on the command line of the existing end-to-end tests, two epochs in a
    child process: exit 0, finite Loss / R2T / R2V, both flags in configurations.json."""
    snap = tmp_path / "snap"
    m = WM.wmap(32, 32)
    np.save(tmp_path / "m.npy", m)
    argv = [sys.executable, os.path.join(ROOT, "nasa-niswan_amd", "train.py"), "--in-channels", "4", "--hidden-channels", "8",
            "--kernel-size", "3", "--num-layers", "1", "--sequence-length", "4", "--input-size", "32", "32", "--grid", "32", "32",
            "--batch-size", "2", "--num-epochs", "2", "--synthetic-steps", "24", "--lat-weighted-loss", "--loss-weights",
            str(tmp_path / "m.npy"), "--snapshot-dir", str(snap)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Epoch: ")]
    assert len(lines) == 2 and all("Loss:" in ln and "R2T:" in ln and "R2V:" in ln for ln in lines), out.stdout
    with open(snap / "logger.npy", "rb") as f:
        a, b_, c = np.load(f), np.load(f), np.load(f)
    assert a.shape == b_.shape == c.shape == (2,) and np.isfinite(a).all() and np.isfinite(b_).all() and np.isfinite(c).all()
    cfg = json.load(open(snap / "configurations.json"))
    assert cfg["lat_weighted_loss"] is True and cfg["loss_weights"] == str(tmp_path / "m.npy")
