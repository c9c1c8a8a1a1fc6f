"""GPU tests of the configurable loss (MSE / L1 / Huber mix with output and step weights): the three ``_spec`` entry points at
the C ABI against their twins (spec (1, 1, 0): bit for bit), against the f64 host model of tests/loss_spec_model.py (dpred bit
for bit), against each other (fused pass = the three separate launches, bit for bit) and at the edges (|d| == delta, NaN, inf,
NaN targets under a zero weight); ``FusedTrainer(loss=LossSpec(...))`` against the oracle fit loop; ``CropLoss`` on the
autograd path; ``train.py --loss-mix ...``.

The shapes, cases and helpers of the existing suites are reused as they are: the dispatch branches of
tests/test_gpu_small_branches.py (FUSED_CASES: f32 and bf16, O = 70 / 128 / 200 in two and more output chunks, Chp = 128), the
sequence slabs, models, targets and tolerances of tests/test_gpu_seq_train.py (HeadCase with B = 2, T = 3; S1, S3o; check_grad)
and the weight map of tests/weighted_loss_model.py."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_spec_model as LM
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
NSC = 10242                                                          # NINT_LOSS_SPEC_SCRATCH_FLOATS


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
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class DSpec:
    """an LM.Spec on the device: the nint_loss_spec struct and the tensor its ow points to"""

    def __init__(self, sp: LM.Spec):
        from nasa_niswan_amd import _lib
        self.t = None if sp.ow is None else dev(sp.ow)
        c = self.c = _lib.NintLossSpec()
        c.mse, c.l1, c.huber, c.delta = sp.a, sp.b, sp.c, sp.delta
        c.ow, c.now, c.osum = (None, 0, 0.0) if sp.ow is None else (self.t.data_ptr(), sp.ow.shape[0], sp.osum)

    @property
    def ref(self):
        return C.byref(self.c)


def crop_spec(lib, pd, yd, wd, wsum, ds, dp, sc, st, shape):
    N, O, H, W, oy, ox, Hc, Wc = shape
    rc = lib.nint_loss_crop_spec(P(pd), P(yd), P(wd), wsum, ds.ref, P(dp), P(sc), P(st), N, O, H, W, oy, ox, Hc, Wc, None)
    assert rc == 0, rc


def run_plain(lib, pred, y, w, sp, shape, st0=BEFORE, entry="spec"):
    """one call of the plain entry (or of its twin: entry = 'old') on fresh outputs; returns (dpred, loss, stats)"""
    N, O, H, W, oy, ox, Hc, Wc = shape
    pd, yd, wd = dev(pred), dev(y), (None if w is None else dev(w))
    wsum = 0.0 if w is None else WM.wsum_of(w)
    dp, sc, st = torch.full((N, O, H, W), 7.0, device="cuda"), torch.zeros(NSC, device="cuda"), dev(st0)
    if entry == "spec":
        crop_spec(lib, pd, yd, wd, wsum, DSpec(sp), dp, sc, st, shape)
    elif w is None:
        assert lib.nint_loss_mse_l1_crop(P(pd), P(yd), P(dp), P(sc), P(st), N, O, H, W, oy, ox, Hc, Wc, None) == 0
    else:
        assert lib.nint_loss_mse_l1_crop_weighted(P(pd), P(yd), P(wd), wsum, P(dp), P(sc), P(st), N, O, H, W, oy, ox, Hc, Wc, None) == 0
    torch.cuda.synchronize()
    return dp, sc[:1].clone(), st


def dead_mask(sp, w, O, H, W, oy, ox, Hc, Wc):
    """(O, H, W) bool: outside the crop or under a zero weight"""
    m = np.ones((O, H, W), bool)
    m[:, oy:oy + Hc, ox:ox + Wc] = LM.weights_of(sp, w, O, Hc, Wc) == 0
    return m


ONE_ONE = LM.Spec(1.0, 1.0, 0.0)


def ones_spec(n):
    return LM.Spec(1.0, 1.0, 0.0, ow=np.ones(n, f32))


# =========================================================================== 1: the general body reproduces today's bits
@pytest.mark.parametrize("shape", LM.PLAIN_SHAPES, ids=["asymmetric-crop", "one-plane-full-image", "grid-stride[>256*1024]"])
def test_spec_110_is_the_plain_entries_bit_for_bit(lib, shape):
    """spec (1, 1, 0) without output weights against nint_loss_mse_l1_crop (no map) and nint_loss_mse_l1_crop_weighted (map):
    loss_out[0], dpred and all eight stats accumulated onto non-zero stats; an all-ones ow with osum = O gives the same bits."""
    N, O, H, W, oy, ox, Hc, Wc = shape
    if N * O * H * W > 256 * 1024:
        assert shape == LM.PLAIN_SHAPES[2]                          # LOSS_BLOCKS x 1024 threads: the grid-stride loop runs
    else:
        assert shape != LM.PLAIN_SHAPES[2]
    case = LM.build_case(shape, LM.SEED + 1, True, False, "default")
    pred, y = case["pred"], case["y"]
    for w in (None, case["w"]):
        old = run_plain(lib, pred, y, w, None, shape, entry="old")
        for sp in (ONE_ONE, ones_spec(O)):
            new = run_plain(lib, pred, y, w, sp, shape)
            for a, b, name in zip(old, new, ("dpred", "loss", "stats")):
                assert same_bits(a, b), (name, w is not None, sp)


def fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc):
    g, Chp, hsl, h, w, b, rng = SB.head_inputs(lib, dt, Ch, O, N, n0, H, W, 2, 40 + Ch + O)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(f32)
    return g, Chp, hsl, h, w, b, y, WM.wmap(Hc, Wc)


def run_fused(lib, entry, hsl, n0, N, Ch, Chp, O, wd, bd, yd, wm, sp, g, oy, ox, Hc, Wc, dt, H, W, st0=BEFORE):
    """entry 'spec': nint_head_loss_fused_spec; 'old': its twin (weighted with a map).  Returns (dpred, dh, loss, stats)."""
    dp = torch.full((N, O, H, W), 7.0, device="cuda")
    dh = torch.full((N, H, W, Chp), 7.0, device="cuda").to(SB.et(dt))
    sc, st = torch.zeros(NSC, device="cuda"), dev(st0)
    wgt, wsum = (None, 0.0) if wm is None else (dev(wm), WM.wsum_of(wm))
    if entry == "spec":
        rc = lib.nint_head_loss_fused_spec(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(yd), P(wgt), wsum, DSpec(sp).ref, P(dp), P(dh),
                                           P(sc), P(st), C.byref(g), oy, ox, Hc, Wc, dt, None)
    elif wm is None:
        rc = lib.nint_head_loss_fused(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(yd), P(dp), P(dh), P(sc), P(st), C.byref(g),
                                      oy, ox, Hc, Wc, dt, None)
    else:
        rc = lib.nint_head_loss_fused_weighted(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(yd), P(wgt), wsum, P(dp), P(dh), P(sc),
                                               P(st), C.byref(g), oy, ox, Hc, Wc, dt, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dp, dh, sc[:1].clone(), st


def test_the_fused_table_holds_what_the_issue_asks_of_it():
    vals = [c.values for c in SB.FUSED_CASES]
    assert {v[0] for v in vals} == {0, 1}                          # f32 and bf16
    assert any(v[2] > 64 for v in vals)                             # an O above HEAD_OCH = 64: two output chunks
    assert any(SB.head_dispatch(v[0], v[1], v[2])[0] == 128 for v in vals)   # Chp = 128


@pytest.mark.parametrize("dt,Ch,O,N,n0,H,W,oy,ox,Hc,Wc,want_chv,tags", SB.FUSED_CASES)
def test_spec_110_is_the_fused_entries_bit_for_bit(lib, dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, want_chv, tags):
    g, Chp, hsl, h, w, b, y, wm = fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc)
    wd, bd, yd = dev(w), dev(b), dev(y)
    a = (hsl, n0, N, Ch, Chp, O, wd, bd, yd)
    z = (g, oy, ox, Hc, Wc, dt, H, W)
    for m in (None, wm):
        old = run_fused(lib, "old", *a, m, None, *z)
        for sp in (ONE_ONE, ones_spec(O)):
            new = run_fused(lib, "spec", *a, m, sp, *z)
            for x, v, name in zip(old, new, ("dpred", "dh", "loss", "stats")):
                assert same_bits(x, v), (name, m is not None, sp.ow is not None)


def seq_case(pkg, Ch, O, dtype):
    hc = ST.HeadCase(pkg, Ch, O, dtype)
    gen = torch.Generator().manual_seed(77 + Ch + O)
    y = torch.randn(hc.B, hc.T, O, *ST.CROP, generator=gen).cuda()
    assert (hc.B, hc.T) == (2, 3)
    return hc, y, WM.wmap(*ST.CROP)


def run_seq(hc, entry, y, wm, sp, st0=BEFORE):
    (oy, ox), (Hc, Wc) = ST.HALO, ST.CROP
    dp = torch.full((hc.T * hc.B, hc.O, hc.H, hc.W), 7.0, device="cuda")
    dh = torch.full((hc.T * hc.B * hc.H * hc.W * hc.Chp * hc.es,), 0xAB, dtype=torch.uint8, device="cuda")
    sc, st = torch.zeros(NSC, device="cuda"), dev(st0)
    wgt, wsum = (None, 0.0) if wm is None else (dev(wm), WM.wsum_of(wm))
    a = (P(hc.slab), hc.B, hc.T, hc.Ch, hc.Chp, hc.O, P(hc.w), P(hc.b), P(y))
    z = (P(dp), P(dh), P(sc), P(st), C.byref(hc.g), oy, ox, Hc, Wc, hc.dt, None)
    if entry == "spec":
        rc = hc.lib.nint_head_loss_seq_fused_spec(*a, P(wgt), wsum, DSpec(sp).ref, *z)
    elif wm is None:
        rc = hc.lib.nint_head_loss_seq_fused(*a, *z)
    else:
        rc = hc.lib.nint_head_loss_seq_fused_weighted(*a, P(wgt), wsum, *z)
    torch.cuda.synchronize()
    return rc, dp, dh, sc[:1].clone(), st


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Ch,O", [(8, 1), (40, 3), (72, 3), (32, 3), (64, 3), (128, 3)])    # (the last three: Ch = CHV, data in the unfused tail)
def test_spec_110_is_the_sequence_entries_bit_for_bit(pkg, Ch, O, dtype):
    hc, y, wm = seq_case(pkg, Ch, O, dtype)
    for m in (None, wm):
        old = run_seq(hc, "old", y, m, None)
        for sp in (ONE_ONE, ones_spec(hc.T * O)):
            new = run_seq(hc, "spec", y, m, sp)
            assert old[0] == 0 and new[0] == 0
            for x, v, name in zip(old[1:], new[1:], ("dpred", "dh_seq", "loss", "stats")):
                assert same_bits(x, v), (name, m is not None, sp.ow is not None)


# =========================================================================== 2: against the f64 model
@pytest.mark.parametrize("shape,mix,with_map,with_ow,steps", LM.plain_cases())
def test_spec_loss_kernel_against_the_f64_model(lib, shape, mix, with_map, with_ow, steps):
    """dpred bit-equal to the model's (float) of the same left-to-right f64 expression, exactly +0 outside the crop and under a
    zero weight; the loss and the eight stats, accumulated onto non-zero stats, within oracle.small_audit's tolerances for two
    f64 accumulations of the same terms in different orders; two runs bit-equal; dpred = NULL and stats = NULL."""
    N, O, H, W, oy, ox, Hc, Wc = shape
    case = LM.build_case(shape, LM.SEED, with_map, with_ow, mix, steps=steps)
    pred, y, w, sp = case["pred"], case["y"], case["w"], case["spec"]
    ref = LM.loss(pred, y, w, sp, oy, ox)
    runs = [run_plain(lib, pred, y, w, sp, shape) for _ in range(2)]
    dp, loss, st = runs[0]
    got = host(dp)
    ndiff = int((got.view(np.uint32) != ref["dpred"].view(np.uint32)).sum())
    print(f"  {sp}: dpred differs from the model's f32 value in {ndiff} of {got.size} elements")
    SM.check_equal(got, ref["dpred"], "spec dpred")
    dead = dead_mask(sp, w, O, H, W, oy, ox, Hc, Wc)
    assert not got.view(np.uint32)[:, dead].any()                   # +0: no bit set
    assert (got[:, ~dead] != 0).sum() >= got[:, ~dead].size - 1     # every live element carries a gradient (but the one d = 0)
    r1 = SM.check_loss_scalar(host(loss)[0], ref["loss"], what="spec loss")
    r2 = SM.check_stats(BEFORE, host(st), [ref], what="spec stats")
    print(f"  loss {float(host(loss)[0])!r} model {ref['loss']!r}; worst ratio loss {r1:.3f}, stats {r2:.3f}")
    assert all(same_bits(a, b) for a, b in zip(runs[0], runs[1]))
    sc = torch.zeros(NSC, device="cuda")
    crop_spec(lib, dev(pred), dev(y), None if w is None else dev(w), 0.0 if w is None else WM.wsum_of(w), DSpec(sp), None, sc, None, shape)
    assert same_bits(sc[:1], loss)


# =========================================================================== 3: fused = the three launches; the f64 model
def fused_spec(O, mix="mix"):
    return LM.Spec(*LM.MIXES[mix], delta=LM.DELTA, ow=LM.output_weights(O))


def stats_close(a, b, mags, what):
    """two accumulations of the same terms in different orders (tests/test_gpu_weighted_loss.py)"""
    a, b = host(a), host(b)
    ref = np.maximum(np.abs(a), np.abs(b))
    ref[2] = max(ref[2], mags)
    err = np.abs(a - b)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (err <= 1e-14 * ref).all(), (what, a, b)


def grad_check(got, ref, what, bf16=False):
    """the standing gradient tolerances (tests/test_gpu_parity.py header): f32 max-abs error <= 1e-3 max|ref| + 1e-6; values
    stored in bf16: rel-L2 <= 2e-2"""
    ST.check_grad(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(ref)), what, "bf16" if bf16 else "f32")


@pytest.mark.parametrize("dt,Ch,O,N,n0,H,W,oy,ox,Hc,Wc,want_chv,tags", SB.FUSED_CASES)
def test_fused_spec_equals_the_three_launches_bit_for_bit(lib, dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, want_chv, tags):
    """nint_head_loss_fused_spec (all three terms, map, output weights) against nint_head_fwd -> nint_loss_crop_spec ->
    nint_head_bwd at every dispatch branch of the fused pass: dpred, dh and the f32 loss bit for bit, the stats to 1e-14 (the f64
    partial sums are folded in another order).  Then dpred and dh against the f64 model from the stored slab."""
    Chp, chv, _, _, _ = SB.head_dispatch(dt, Ch, O)
    assert chv == want_chv and Chp <= 128
    g, Chp, hsl, h, w, b, y, wm = fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc)
    sp = fused_spec(O)
    wd, bd, yd = dev(w), dev(b), dev(y)
    dp2, dh2, loss2, st2 = run_fused(lib, "spec", hsl, n0, N, Ch, Chp, O, wd, bd, yd, wm, sp, g, oy, ox, Hc, Wc, dt, H, W, np.zeros(8))
    pred = torch.full((N, O, H, W), 7.0, device="cuda")
    assert lib.nint_head_fwd(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(pred), C.byref(g), dt, None) == 0
    dp1, sc1, st1 = torch.full((N, O, H, W), 7.0, device="cuda"), torch.zeros(NSC, device="cuda"), dev(np.zeros(8))
    crop_spec(lib, pred, yd, dev(wm), WM.wsum_of(wm), DSpec(sp), dp1, sc1, st1, (N, O, H, W, oy, ox, Hc, Wc))
    dh1 = torch.full((N, H, W, Chp), 7.0, device="cuda").to(SB.et(dt))
    assert lib.nint_head_bwd(P(hsl), n0, N, Ch, Chp, O, P(wd), P(dp1), P(dh1), None, None, C.byref(g), dt, None, 0, None) == 0
    torch.cuda.synchronize()
    print(f"  loss fused {float(loss2[0])!r} three launches {float(sc1[0])!r}")
    assert same_bits(dp1, dp2) and same_bits(dh1, dh2) and same_bits(sc1[:1], loss2)
    Wd = LM.weights_of(sp, wm, O, Hc, Wc)
    stats_close(st1, st2, float(np.sum(np.abs(y.astype(np.float64)) * Wd[None])), "fused against three launches")
    assert host(st2)[4] == LM.cnt_of(N, O, sp, wm, Hc, Wc) and host(st2)[7] == 1.0
    rdp, rdh, rloss = LM.head_loss_fused(h, w, b, y, wm, sp, oy, ox)
    got_dp, got_dh = host(dp2), SB.decode(dh2, dt)
    assert not got_dp.view(np.uint32)[:, dead_mask(sp, wm, O, H, W, oy, ox, Hc, Wc)].any()
    assert not got_dh[..., Ch:].any()                               # the channel padding
    grad_check(got_dp, rdp, "fused spec dpred")
    grad_check(got_dh[..., :Ch], rdh, "fused spec dh", bool(dt))
    assert abs(float(loss2[0]) - rloss) <= 1e-4 * abs(rloss) + 1e-5  # (the output tolerance; the bit-level statement is above)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Ch,O", [(Ch, O) for Ch in (8, 40, 72) for O in (1, 3)] + [(72, 200)] +
                         [(32, 3), (64, 3), (128, 3)])    # (Ch = CHV: data in the 12 staged channels the dot product leaves unfused)
def test_seq_fused_spec_equals_the_three_launches_bit_for_bit(pkg, Ch, O, dtype):
    """The sequence form with step weights (B = 2, T = 3; the first step dropped, the second discounted) times output weights:
    nint_head_loss_seq_fused_spec against nint_head_fwd_seq -> nint_loss_crop_spec (N = B, O' = T*O, the same ow) ->
    nint_head_bwd_seq; dpred is in image order t*B + b there and (B, T*O, H, W) here.  dpred also against the f64 model."""
    hc, y, wm = seq_case(pkg, Ch, O, dtype)
    (oy, ox), (Hc, Wc) = ST.HALO, ST.CROP
    B, T, H, W = hc.B, hc.T, hc.H, hc.W
    sp = LM.Spec(*LM.MIXES["mix"], delta=LM.DELTA, ow=LM.seq_weights(LM.STEP_W, LM.output_weights(O)))
    rc, dp2, dh2, loss2, st2 = run_seq(hc, "spec", y, wm, sp, np.zeros(8))
    assert rc == 0
    seq = hc.fwd_seq()
    dseq, sc1, st1 = torch.full_like(seq, 7.0), torch.zeros(NSC, device="cuda"), dev(np.zeros(8))
    crop_spec(hc.lib, seq, y, dev(wm), WM.wsum_of(wm), DSpec(sp), dseq, sc1, st1, (B, T * O, H, W, oy, ox, Hc, Wc))
    dh1, _, _ = hc.bwd_seq(dseq, None)
    torch.cuda.synchronize()
    print(f"  loss fused {float(loss2[0])!r} three launches {float(sc1[0])!r}")
    assert same_bits(dp2.view(T, B, O, H, W).permute(1, 0, 2, 3, 4).contiguous(), dseq.view(B, T, O, H, W))
    assert same_bits(dh1, dh2) and same_bits(sc1[:1], loss2)
    Wd = LM.weights_of(sp, wm, T * O, Hc, Wc)
    yh = y.double().cpu().numpy().reshape(B, T * O, Hc, Wc)
    stats_close(st1, st2, float(np.sum(np.abs(yh) * Wd[None])), "seq fused against three launches")
    assert host(st2)[4] == LM.cnt_of(B, T * O, sp, wm, Hc, Wc)
    assert not bits(dp2.view(T, B, O, H, W)[0]).any()               # the dropped step: +0 everywhere
    pred = torch.einsum("oc,tbcyx->btoyx", hc.w.double().cpu(), hc.h) + hc.b.double().cpu().view(1, 1, O, 1, 1)
    d = pred[..., oy:oy + Hc, ox:ox + Wc].numpy().reshape(B, T * O, Hc, Wc) - yh
    want = np.zeros((B, T * O, H, W))
    want[..., oy:oy + Hc, ox:ox + Wc] = np.where(Wd[None] > 0, LM.grad64(sp, d, 1.0 / LM.cnt_of(B, T * O, sp, wm, Hc, Wc), Wd[None]), 0.0)
    got = host(dseq)
    assert not got.view(np.uint32)[:, dead_mask(sp, wm, T * O, H, W, oy, ox, Hc, Wc)].any()
    grad_check(got, want, f"seq fused spec dpred Ch={Ch} O={O} {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_spec_entries_refuse_more_than_128_padded_channels(pkg, dtype):
    hc, y, wm = seq_case(pkg, 136, 1, dtype)
    assert hc.Chp > 128
    rc, _, _, _, _ = run_seq(hc, "spec", y, wm, ONE_ONE)
    assert rc == E_SHAPE
    (oy, ox), (Hc, Wc) = ST.HALO, ST.CROP
    a = P(hc.slab)
    assert hc.lib.nint_head_loss_fused_spec(a, hc.B, hc.B, hc.Ch, hc.Chp, hc.O, P(hc.w), P(hc.b), P(y), None, 0.0, DSpec(ONE_ONE).ref,
                                            a, a, a, None, C.byref(hc.g), oy, ox, Hc, Wc, hc.dt, None) == E_SHAPE


# =========================================================================== 4: edges
EDGE_SHAPE = LM.PLAIN_SHAPES[0]


def edge_case(with_ow=True):
    case = LM.build_case(EDGE_SHAPE, LM.SEED + 2, True, with_ow, "huber")
    return case["pred"], case["y"], case["w"], case["spec"], case["where"]


def at(where, shape):
    """index of a planted crop element in the (N, O, H, W) tensors"""
    n, o, cy, cx = where
    return (n, o, shape[4] + cy, shape[5] + cx)


def test_huber_threshold_elements_take_the_quadratic_branch(lib):
    """|d| == delta exactly: the gradient is c * d (the quadratic branch, `<=`); one ulp above: c * delta.  Both expressions give
    c * delta for d == delta itself, so the branch is pinned where it shows: H(d) in the loss is continuous, the gradient of the
    element one ulp above is the clamp's; the planted elements' dpred are the model's bits."""
    pred, y, w, sp, where = edge_case()
    N, O, H, W, oy, ox, Hc, Wc = EDGE_SHAPE
    sp = LM.Spec(0.0, 0.0, 2.5, delta=LM.DELTA, ow=sp.ow)
    dp, loss, st = run_plain(lib, pred, y, w, sp, EDGE_SHAPE)
    got, ref = host(dp), LM.loss(pred, y, w, sp, oy, ox)
    SM.check_equal(got, ref["dpred"], "huber dpred")
    cnt = LM.cnt_of(N, O, sp, w, Hc, Wc)
    Wd = LM.weights_of(sp, w, O, Hc, Wc)
    for name, dval in (("plus", LM.DELTA), ("minus", -LM.DELTA), ("zero", 0.0), ("above", LM.DELTA)):
        n, o, cy, cx = where[name]
        want = f32(((sp.c * dval) * (1.0 / cnt)) * Wd[o, cy, cx])
        assert got[at(where[name], EDGE_SHAPE)] == want, name
    assert not np.signbit(got[at(where["zero"], EDGE_SHAPE)])
    SM.check_loss_scalar(host(loss)[0], ref["loss"], what="huber loss")


def test_nan_and_inf_predictions(lib):
    pred, y, w, sp, where = edge_case()
    N, O, H, W, oy, ox, Hc, Wc = EDGE_SHAPE
    hub = LM.Spec(0.0, 0.0, 1.0, delta=LM.DELTA, ow=sp.ow)
    spot = at(where["plus"], EDGE_SHAPE)
    n, o, cy, cx = where["plus"]
    # one NaN in pred, Huber alone: the loss is NaN, dpred is NaN at that element only (fmin / fmax would give delta there)
    p = pred.copy(); p[spot] = np.nan
    dp, loss, st = run_plain(lib, p, y, w, hub, EDGE_SHAPE)
    got, ref = host(dp), LM.loss(p, y, w, hub, oy, ox)
    assert np.isnan(host(loss)[0]) and np.isnan(got[spot]) and int(np.isnan(got).sum()) == 1
    assert np.isnan(ref["dpred"][spot])
    got[spot] = ref["dpred"][spot] = 0.0                            # (a NaN's payload is nobody's contract: every OTHER element by its bytes)
    SM.check_equal(got, ref["dpred"], "dpred around one NaN")
    # one inf in pred, Huber alone: the loss is +inf, dpred there the finite c * delta * Wd / cnt; nothing is NaN
    p = pred.copy(); p[spot] = np.inf
    dp, loss, st = run_plain(lib, p, y, w, hub, EDGE_SHAPE)
    got = host(dp)
    cnt, Wd = LM.cnt_of(N, O, hub, w, Hc, Wc), LM.weights_of(hub, w, O, Hc, Wc)
    assert host(loss)[0] == np.inf and not np.isnan(got).any() and np.isfinite(got).all()
    assert got[spot] == f32(((hub.c * hub.delta) * (1.0 / cnt)) * Wd[o, cy, cx]) and got[spot] > 0
    SM.check_equal(got, LM.loss(p, y, w, hub, oy, ox)["dpred"], "dpred around one inf")
    assert not np.isnan(host(st)[[1, 2, 3, 4, 7]]).any()
    # one inf in pred with a = 0, b = 1, c = 0: +inf, not 0 * inf = NaN (the omitted-term rule)
    l1 = LM.Spec(0.0, 1.0, 0.0, ow=sp.ow)
    dp, loss, st = run_plain(lib, p, y, w, l1, EDGE_SHAPE)
    assert host(loss)[0] == np.inf and not np.isnan(host(dp)).any()
    SM.check_equal(host(dp), LM.loss(p, y, w, l1, oy, ox)["dpred"], "l1 dpred around one inf")


def test_nan_targets_under_zero_output_and_step_weights_change_nothing(lib, pkg):
    """y = NaN wherever the output's (or the step's) weight is 0: loss, dpred, dh and stats keep the bits of the run with finite
    targets, for the plain, the fused and the sequence entry."""
    pred, y, w, sp, _ = edge_case()
    sp = LM.Spec(*LM.MIXES["mix"], delta=LM.DELTA, ow=sp.ow)
    off = sp.ow == 0
    assert off.any()
    y_nan = y.copy(); y_nan[:, off] = np.nan
    out = [run_plain(lib, pred, yy, w, sp, EDGE_SHAPE) for yy in (y, y_nan)]
    assert all(torch.isfinite(t).all() for t in out[1]) and all(same_bits(a, b) for a, b in zip(*out))
    for case in (SB.FUSED_CASES[0], SB.FUSED_CASES[3]):              # f32 CHV 32 with n0 = 1, bf16 CHV 64 with two output chunks
        dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, _, _ = case.values
        g, Chp, hsl, h, wh, b, y2, wm = fused_inputs(lib, dt, Ch, O, N, n0, H, W, Hc, Wc)
        fs = fused_spec(O)
        y_nan = y2.copy(); y_nan[:, fs.ow == 0] = np.nan
        assert np.isnan(y_nan).any()
        wd, bd = dev(wh), dev(b)
        out = [run_fused(lib, "spec", hsl, n0, N, Ch, Chp, O, wd, bd, dev(yy), wm, fs, g, oy, ox, Hc, Wc, dt, H, W) for yy in (y2, y_nan)]
        assert all(torch.isfinite(t.float()).all() for t in out[1]) and all(same_bits(a, b) for a, b in zip(*out)), case.id
    hc, ys, wm = seq_case(pkg, 40, 3, "bf16")
    ss = LM.Spec(*LM.MIXES["mix"], delta=LM.DELTA, ow=LM.seq_weights(LM.STEP_W, np.array([1.5, 0.75, 1.0], f32)))
    y_nan = ys.clone(); y_nan[:, 0] = float("nan")                   # the whole dropped step
    out = [run_seq(hc, "spec", yy, wm, ss)[1:] for yy in (ys, y_nan)]
    assert torch.isfinite(hc.dh_values(out[1][1])).all() and all(torch.isfinite(t).all() for t in (out[1][0], out[1][2], out[1][3]))
    assert all(same_bits(a, b) for a, b in zip(*out))


# =========================================================================== 5: the trainer against the oracle fit loop
B, T, H, W = ST.B, ST.T, ST.H, ST.W
HALO, CROP, LR, BETAS = ST.HALO, ST.CROP, ST.LR, ST.BETAS
STEP4 = np.array([0.0, 0.5, 1.0, 1.0], f32)                          # T = 4: the first step dropped, the second discounted
TRAIN_MIX = (0.5, 2.0, 1.5)


def out_w(shape):
    O = ST.SHAPES[shape][3]
    return None if O == 1 else np.array([1.0, 0.0, 2.0], f32)[:O]


def model_spec(shape, sq):
    ow = out_w(shape)
    if sq:
        ow = LM.seq_weights(STEP4, np.ones(1, f32) if ow is None else ow)
    return LM.Spec(*TRAIN_MIX, delta=LM.DELTA, ow=ow)


def lib_spec(shape, sq):
    from nasa_niswan_amd.loss import LossSpec
    return LossSpec(*TRAIN_MIX, delta=LM.DELTA, output_weights=out_w(shape), step_weights=STEP4 if sq else None)


def targets(shape, sq):
    y = ST.trainer_targets(shape)
    return y if sq else y[:, -1].contiguous()


@functools.lru_cache(maxsize=None)
def oracle_steps(shape, sq, with_map, nsteps=3):
    """tests/test_gpu_weighted_loss.py's oracle_steps with loss_spec_model.loss_torch: CPU autograd on
    convlstm_oracle.convlstm_forward, then adam_step_numpy.  Per step: loss, gradients, parameters after the step."""
    from oracle import convlstm_oracle as O
    params, X, _, _ = ST.case_data(shape)
    yv = targets(shape, sq).reshape(B, -1, *CROP)
    w = WM.wmap(*CROP) if with_map else None
    sp = model_spec(shape, sq)
    p = params
    st = {"m": {k: torch.zeros_like(v) for k, v in p.items()}, "v": {k: torch.zeros_like(v) for k, v in p.items()}}
    out = []
    for step in range(1, nsteps + 1):
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
        pred, seq = O.convlstm_forward(X, leaf, return_sequence=True)
        loss = LM.loss_torch(seq if sq else pred, yv, w, sp, HALO[0], HALO[1])
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in leaf.items()}
        newp, m, v = {}, {}, {}
        for k in p:
            a, b_, c = O.adam_step_numpy(p[k].numpy(), grads[k].numpy(), st["m"][k].numpy(), st["v"][k].numpy(), step, LR, BETAS)
            newp[k], m[k], v[k] = torch.from_numpy(a), torch.from_numpy(b_), torch.from_numpy(c)
        p, st = newp, {"m": m, "v": v}
        out.append(dict(loss=float(loss.detach()), grads=grads, params=p))
    return out


def make_trainer(pkg, shape, dtype, sq, fallback, with_map, spec, **kw):
    from nasa_niswan_amd.trainer import FusedTrainer
    params, X, _, _ = ST.case_data(shape)
    cin, hidden, ks, out = ST.SHAPES[shape]
    net = pkg.ConvLSTM(cin, hidden, ks, len(hidden), out_channels=out, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, sequence_loss=sq, loss_weights=WM.wmap(*CROP) if with_map else None,
                      loss=spec, **kw)
    eng = net._engine(torch.device("cuda", 0))
    name = "head_loss_seq_fused" if sq else "head_loss_fused"
    calls, real = [], getattr(eng, name)

    def spy(*a, **k):
        assert ("spec" in k) == (tr._spec is not None)
        calls.append(False if fallback else real(*a, **k))
        return calls[-1]
    setattr(eng, name, spy)
    return net, tr, calls


TRAINER_CASES = [pytest.param("S3o", "f32", False, False, True, id="S3o-f32-last-step-fused-map"),
                 pytest.param("S3o", "bf16", True, False, True, id="S3o-bf16-sequence-step-weights-fused-map"),
                 pytest.param("S3o", "f32", True, True, True, id="S3o-f32-sequence-step-weights-three-launch-map"),
                 pytest.param("S1", "f32", True, False, False, id="S1-f32-sequence-step-weights-fused"),
                 pytest.param("S3o", "f32", False, True, False, id="S3o-f32-last-step-three-launch")]


@pytest.mark.parametrize("shape,dtype,sq,fallback,with_map", TRAINER_CASES)
def test_spec_step_matches_the_oracle_fit_loop(pkg, shape, dtype, sq, fallback, with_map):
    """Three steps at lr 1e-4, betas (0.5, 0.999) with the mix (0.5, 2, 1.5), delta 0.75, output weights (1, 0, 2) and step
    weights (0, 0.5, 1, 1), through the fused head / loss pass and through the three-launch fallback.  The tolerances are those
    of test_gpu_weighted_loss.test_weighted_step_matches_the_oracle_fit_loop (derived in test_gpu_seq_train): loss 1e-4 rel +
    1e-5 (f32) / 2e-2 (bf16); bucket gradients the standing ones; parameters max |dp| <= k * 2.2 * lr, mean 2e-6 (f32) /
    0.1 * lr * k (bf16).  Then evaluate(): its statistics are the host model's on the prediction it returns."""
    params, X, _, _ = ST.case_data(shape)
    y = targets(shape, sq)
    want = oracle_steps(shape, sq, with_map)
    net, tr, calls = make_trainer(pkg, shape, dtype, sq, fallback, with_map, lib_spec(shape, sq))
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
                assert float(d.max()) <= step * 2.2 * LR, (k, step)
                assert float(d.mean()) <= (2e-6 if dtype == "f32" else 0.1 * LR * step), (k, step)
    assert calls == [not fallback] * 3                            # the path the case is about did run
    if dtype == "f32":
        loss_e, _ = tr.epoch_stats()
        want_loss = np.mean([o["loss"] for o in want])
        assert abs(loss_e - want_loss) <= 1e-4 * abs(want_loss) + 1e-5   # the mean of the CONFIGURED loss
    tr.reset_stats()
    full = tr.evaluate(Xd, yd)
    ref = LM.loss(host(full), y.reshape(B, -1, *CROP).numpy(), WM.wmap(*CROP) if with_map else None, model_spec(shape, sq), HALO[0], HALO[1])
    le, r2e = tr.epoch_stats()
    print(f"  evaluate: loss {le!r} (model {ref['loss']!r}), R2 {r2e!r} (model {ref['r2']!r})")
    assert abs(le - ref["loss"]) <= 1e-9 * abs(ref["loss"]) and abs(r2e - ref["r2"]) <= 1e-9 * (1.0 + abs(ref["r2"]))


def test_spec_step_in_two_segments_and_two_micro_batches(pkg):
    """bptt_segments = 2 with accumulate_steps = 2 on the last-step loss: two calls with the same batch put the mean of two
    equal gradients under ONE Adam step -- the oracle's first step, with the tolerances of the test above."""
    shape, dtype = "S3o", "f32"
    params, X, _, _ = ST.case_data(shape)
    y = targets(shape, False)
    o = oracle_steps(shape, False, True)[0]
    net, tr, calls = make_trainer(pkg, shape, dtype, False, False, True, lib_spec(shape, False), bptt_segments=2, accumulate_steps=2)
    Xd, yd = X.cuda(), y.cuda()
    l1 = float(tr.step(Xd, yd))
    assert all(torch.equal(v.cpu(), params[k]) for k, v in net.state_dict().items())      # no optimizer step yet
    l2 = float(tr.step(Xd, yd))
    assert l1 == l2 and abs(l1 - o["loss"]) <= 1e-4 * abs(o["loss"]) + 1e-5 and calls == [True, True]
    for i, (k, _) in enumerate(net.named_parameters()):
        ST.check_grad(tr.flat.grad_view(i).view(o["grads"][k].shape), 2.0 * o["grads"][k], f"segments + accumulate bucket d{k}")
    for k, v in net.state_dict().items():
        d = (v.cpu() - o["params"][k]).abs()
        assert float(d.max()) <= 2.2 * LR and float(d.mean()) <= 2e-6, k


def one_step(pkg, spec, sq=False, dtype="f32", shape="S3o", switch=(), with_map=False):
    params, X, _, _ = ST.case_data(shape)
    net, tr, _ = make_trainer(pkg, shape, dtype, sq, False, with_map, spec)
    for s in switch:
        tr.set_loss(s)
    loss = tr.step(X.cuda(), targets(shape, sq).cuda()).clone()
    return net, tr, loss


@pytest.mark.parametrize("sq", [False, True], ids=["last-step", "sequence-loss"])
def test_set_loss_none_returns_to_todays_bits(pkg, sq):
    from nasa_niswan_amd.loss import LossSpec
    na, ta, la = one_step(pkg, lib_spec("S3o", sq), sq, switch=(None,))
    nb, tb, lb = one_step(pkg, None, sq)
    assert same_bits(la, lb) and same_bits(ta.flat.grad, tb.flat.grad) and same_bits(ta.flat.data, tb.flat.data) and same_bits(ta.stats, tb.stats)
    # the default spec is the same loss through the general body: the same bits again
    nc, tc, lc = one_step(pkg, LossSpec(), sq)
    assert same_bits(lc, lb) and same_bits(tc.flat.grad, tb.flat.grad) and same_bits(tc.flat.data, tb.flat.data) and same_bits(tc.stats, tb.stats)
    # ... and switching a spec on between steps is the trainer that had it from the start: another number
    nd, td, ld = one_step(pkg, None, sq, switch=(lib_spec("S3o", sq),))
    ne, te, le = one_step(pkg, lib_spec("S3o", sq), sq)
    assert same_bits(ld, le) and same_bits(td.flat.grad, te.flat.grad) and same_bits(td.flat.data, te.flat.data)
    assert not same_bits(ld, lb)
    with pytest.raises(ValueError):
        one_step(pkg, LossSpec(output_weights=[1.0, 2.0]), sq)       # the length is checked against O at the first step


@pytest.mark.parametrize("sq", [False, True], ids=["last-step", "sequence-loss"])
def test_default_spec_under_carried_state_and_the_guarded_adam_keeps_todays_bits(pkg, sq):
    """stateful + max_grad_norm + skip_nonfinite: two consecutive chunks with LossSpec() are the trainer without a spec bit for
    bit (loss, bucket, parameters, stats, guard counters); with the Huber mix the same options run, stay finite and apply both
    steps."""
    from nasa_niswan_amd.loss import LossSpec
    params, X, _, _ = ST.case_data("S3o")
    Xd, yd = X.cuda(), targets("S3o", sq).cuda()
    out = []
    for spec in (None, LossSpec(), lib_spec("S3o", sq)):
        net, tr, _ = make_trainer(pkg, "S3o", "bf16", sq, False, True, spec, stateful=True, max_grad_norm=0.5, skip_nonfinite=True)
        losses = [tr.step(Xd, yd).clone() for _ in range(2)]
        out.append((losses[0], losses[1], tr.flat.grad.clone(), tr.flat.data.clone(), tr.stats.clone(), tr.grad_stats()))
    for a, b in zip(out[0][:5], out[1][:5]):
        assert same_bits(a, b)
    assert out[0][5] == out[1][5] and out[0][5]["applied"] == 2
    assert all(torch.isfinite(t).all() for t in out[2][:5]) and out[2][5]["applied"] == 2 and out[2][5]["skipped"] == 0
    assert not same_bits(out[2][0], out[0][0])


@pytest.mark.parametrize("sq", [False, True], ids=["last-step", "sequence-loss"])
def test_a_zero_weighted_output_gets_no_head_gradient_while_the_rest_moves(pkg, sq):
    params, _, _, _ = ST.case_data("S3o")
    net, tr, loss = one_step(pkg, lib_spec("S3o", sq), sq)
    L = net.num_layers
    dw, db = tr.flat.grad_view(2 * L).view(3, -1), tr.flat.grad_view(2 * L + 1)
    assert not dw[1].any() and not db[1].any() and dw[0].any() and dw[2].any() and db[0] != 0 and db[2] != 0
    dp = tr._dpred.view(-1, 3, H, W)
    assert not bits(dp[:, 1]).any() and torch.isfinite(loss)
    if sq:
        assert not bits(dp[:B]).any()                                # the dropped first step (images t*B + b)
    state = net.state_dict()
    assert torch.equal(state["conv.weight"].cpu()[1], params["conv.weight"][1]) and torch.equal(state["conv.bias"].cpu()[1], params["conv.bias"][1])
    moved = [k for k, v in state.items() if not torch.equal(v.cpu(), params[k])]
    assert len(moved) == len(params), moved


def test_crop_loss_module_against_torch_on_the_crop(pkg):
    """criterion(y, pred) with a Huber mix, map and output weights: torch's MSELoss / L1Loss / HuberLoss on the crop with the
    weights applied by hand (loss_spec_model.loss_torch), value and gradient; an upstream factor is honoured exactly; y gets no
    gradient."""
    from nasa_niswan_amd.loss import CropLoss, LossSpec
    O = 3
    wm = WM.wmap(*CROP)
    ow = np.array([1.0, 0.0, 2.0], f32)
    sp = LM.Spec(*TRAIN_MIX, delta=LM.DELTA, ow=ow)
    gen = torch.Generator().manual_seed(9)
    pred, y = torch.randn(B, O, H, W, generator=gen), torch.randn(B, O, *CROP, generator=gen)
    pt = pred.double().requires_grad_(True)
    lt = LM.loss_torch(pt, y.double(), wm, sp, HALO[0], HALO[1])
    lt.backward()
    crit = CropLoss(HALO, LossSpec(*TRAIN_MIX, delta=LM.DELTA, output_weights=ow), weights=wm)
    pl, yl = pred.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    loss = crit(yl, pl)
    loss.backward()
    g1 = pl.grad.clone()
    assert abs(float(loss.detach()) - float(lt.detach())) <= 1e-6 * abs(float(lt.detach())) and yl.grad is None
    ST.check_grad(g1, pt.grad, "CropLoss dpred")
    SM.check_equal(host(g1), LM.loss(pred.numpy(), y.numpy(), wm, sp, HALO[0], HALO[1])["dpred"], "CropLoss dpred bits")
    pl.grad = None
    (3.0 * crit(yl, pl)).backward()
    assert torch.equal(pl.grad, g1 * 3.0)
    with pytest.raises(ValueError):
        CropLoss(HALO, LossSpec(step_weights=[0.0, 1.0]))(yl, pl)    # one prediction has no steps
    # the default spec is CropMSEL1Loss
    from nasa_niswan_amd.loss import CropMSEL1Loss
    a, b = CropLoss(HALO)(yl, pl), CropMSEL1Loss(HALO)(yl, pl)
    assert same_bits(a.detach(), b.detach())


def test_train_py_loss_mix_end_to_end(pkg, tmp_path):
    """train.py --loss-mix 0 0 1 --huber-delta 0.5 --sequence-loss --spinup-steps 1 on the synthetic dataset, two epochs in a
    child process: exit 0, finite Loss / R2T / R2V, the flags in configurations.json."""
    snap = tmp_path / "snap"
    argv = [sys.executable, os.path.join(ROOT, "nasa-niswan_amd", "train.py"), "--in-channels", "4", "--hidden-channels", "8",
            "--kernel-size", "3", "--num-layers", "1", "--sequence-length", "4", "--input-size", "32", "32", "--grid", "32", "32",
            "--batch-size", "2", "--num-epochs", "2", "--synthetic-steps", "24", "--loss-mix", "0", "0", "1", "--huber-delta", "0.5",
            "--sequence-loss", "--spinup-steps", "1", "--snapshot-dir", str(snap)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Epoch: ")]
    assert len(lines) == 2 and all("Loss:" in ln and "R2T:" in ln and "R2V:" in ln for ln in lines), out.stdout
    with open(snap / "logger.npy", "rb") as f:
        a, b_, c = np.load(f), np.load(f), np.load(f)
    assert a.shape == b_.shape == c.shape == (2,) and np.isfinite(a).all() and np.isfinite(b_).all() and np.isfinite(c).all()
    cfg = json.load(open(snap / "configurations.json"))
    assert cfg["loss_mix"] == [0.0, 0.0, 1.0] and cfg["huber_delta"] == 0.5 and cfg["spinup_steps"] == 1 and cfg["sequence_loss"] is True
