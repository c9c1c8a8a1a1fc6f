"""nint_ens_loss (csrc/ensemble.hip) against tests/ens_loss_model.py at the smallest shapes at which the kernel
can go wrong: grid 15 x 41 = 615 pixels (three 256-pixel workgroups, the last partial, a partial wave), crop 13 x 37 at (1, 2),
O = 5 (a group of four outputs and a remainder), M = 2, 3, 8 and the largest, 64; N = 1, 3 and 70 (beyond one launch piece).

Integer data with dyadic weights: SA, SD, SV, Sy, Syy are exact in any order, so loss_out, every dpred, ens_out and the stats
made of them must have the model's bits; S2 and S1 come from the mean m = S / M and are exact where M is a power of two (2, 8,
64) -- for M = 3 they are sums of rounded terms and are held to the any-order bound (check_all).  Normal data: dpred is elementwise, so it has the model's bits whatever the reduction order; every sum is held to
the bound of ANY summation order against the exact value (python fractions, ens_loss_model.total_bounds) -- nothing here is
measured."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import ensemble_model as EM
import ens_loss_model as LM
from oracle import small_audit as SM
from oracle.guarded_alloc import GuardedTorch, same_bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
H, W, OY, OX, HC, WC, O = 15, 41, 1, 2, 13, 37, 5


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


def dyadic_map():
    """(Hc, Wc) powers of two times small integers, with zero cells"""
    w = np.broadcast_to(EM.dyadic_rows(HC)[:, None], (HC, WC)).astype(np.float32).copy()
    w[3, 5] = 0.0
    w[12, 36] = 0.0
    w[:, 7] *= 0.5
    return w


def dyadic_table(rows):
    """(rows, O) dyadic output weights with a zero entry in every row"""
    t = np.array([[1.0, 0.5, 0.0, 2.0, 0.25], [0.0, 1.0, 4.0, 0.5, 1.0], [0.5, 0.0, 1.0, 1.0, 2.0]], np.float32)
    return t[:rows]


def call(lib, pred, poff, pstride, dpred, doff, dstride, M, y, alpha, cnt, wgt=None, ow=None, ow_row=None, stats=None, ens=None,
         grid=(H, W), at=(OY, OX), alloc=torch, nan_fill=True):
    """one nint_ens_loss call on device tensors; dpred, stats and ens grow / are written in place; returns (loss_out, stats, ens).
    The scratch has exactly the queried size and starts as NaN."""
    N, Oo, Hc, Wc = y.shape
    nb = lib.nint_ens_loss_scratch_bytes(N, M, Oo, grid[0], grid[1])
    assert nb == (min(N, 64) * Oo * ((grid[0] * grid[1] + 255) // 256) + N * Oo) * 8 * 8
    scratch = alloc.empty(nb // 8, dtype=torch.float64, device="cuda")
    loss = alloc.empty(1, dtype=torch.float32, device="cuda")
    if nan_fill:
        scratch.fill_(NAN)
        loss.fill_(NAN)
    stats = alloc.zeros(8, dtype=torch.float64, device="cuda") if stats is None else stats
    ens = alloc.zeros(4, dtype=torch.float64, device="cuda") if ens is None else ens
    from nasa_niswan_amd import _lib
    sp = _lib.NintEnsLossSpec()
    rows = None if ow_row is None else (C.c_int32 * N)(*[int(v) for v in ow_row])
    sp.alpha, sp.cnt, sp.ow, sp.ow_row, sp.nrows = float(alpha), float(cnt), None if ow is None else ow.data_ptr(), rows, 0 if ow is None else ow.shape[0]
    wsum = 0.0 if wgt is None else float(host(wgt).astype(np.float64).sum())
    rc = lib.nint_ens_loss(P(pred), (C.c_int64 * N)(*[int(v) for v in poff]), int(pstride), P(dpred),
                           (C.c_int64 * N)(*[int(v) for v in doff]), int(dstride), M, P(y), P(wgt), wsum, C.byref(sp), P(loss), P(stats),
                           P(ens), P(scratch), nb, N, Oo, grid[0], grid[1], at[0], at[1], Hc, Wc, None)
    assert rc == 0, rc
    return loss, stats, ens


def contiguous(N, M):
    img = O * H * W
    return [n * M * img for n in range(N)], img


def run_contiguous(lib, pred, y, M, alpha, wgt=None, ow=None, ow_row=None, stats0=None, ens0=None, **kw):
    """members contiguous (N, M, O, H, W), gradients in the same layout; dpred starts as NaN"""
    N = y.shape[0]
    off, img = contiguous(N, M)
    q, w, cnt = LM.weights(N, O, HC, WC, wgt, ow, ow_row)
    dp = torch.full((N, M, O, H, W), NAN, device="cuda")
    loss, stats, ens = call(lib, dev(pred), off, img, dp, off, img, M, dev(y), alpha, cnt, dev(wgt), dev(ow), ow_row,
                            dev(stats0), dev(ens0), **kw)
    return host(dp), host(loss), host(stats), host(ens)


def check_all(got, ref, what, M, alpha, stats0=None, ens0=None):
    """Integer data.  SA, SD, SV, Sy, Syy are sums of integers times dyadic weights: exact in any order, so the loss, ens_out and
    those stats have the model's bits.  S2 and S1 come from m = S / M: exact too where M is a power of two (2, 8, 64).  For M = 3
    the terms Wd*(m-t)^2, Wd*|m-t| are rounded numbers -- the model's and the kernel's terms have the same bits, their sums
    depend on the order: each is held to gamma(n) * sum |term| against math.fsum of the model's terms (n terms: n - 1 additions
    in any order, one rounding for fsum's own), and stats[0], [1], [6] to the closing expressions on the device's own sums."""
    import math
    dp, loss, stats, ens = got
    SM.check_equal(dp, LM.full_images(ref["dpred"], H, W, OY, OX), f"{what}: dpred")
    SM.check_equal(loss, np.array([ref["loss_f32"]], np.float32), f"{what}: loss_out")
    SM.check_equal(ens, ref["ens"], f"{what}: ens_out")
    if M & (M - 1) == 0:
        SM.check_equal(stats, ref["stats"], f"{what}: stats")
        return
    s0 = np.zeros(8) if stats0 is None else np.asarray(stats0, np.float64)
    n = int(ref["live"].sum())
    for k in (3, 4):                                     # S2, S1
        terms = ref["terms"][k].reshape(-1)
        exact, mag = math.fsum(terms), math.fsum(np.abs(terms))
        got_k = stats[k - 3] - s0[k - 3]                 # (stats0 holds small numbers: one rounding for its addition, below)
        bound = float(EM.gamma(n)) * mag + 2.0 ** -52 * abs(stats[k - 3])
        assert abs(got_k - exact) <= bound, f"{what}: {LM.TERMS[k]}: got {got_k!r}, fsum {exact!r}, bound {bound:.3e}"
    keep = [2, 3, 4, 5, 7]
    SM.check_equal(stats[keep], ref["stats"][keep], f"{what}: stats[2, 3, 4, 5, 7]")
    # R2 = 1 - S2 / ss_tot with ss_tot exact: S2's relative error (below n * 2^-53) carries over, times S2 / ss_tot
    r2 = ref["stats"][6] - s0[6]
    assert abs((stats[6] - s0[6]) - r2) <= (n + 8) * 2.0 ** -52 * (1.0 + abs(1.0 - r2)), f"{what}: stats[6]"


# =========================================================================== integer data: equal bits
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("M", [2, 3, 8, 64])
def test_bits_on_integer_data(lib, M, N, weighted):
    rng = np.random.default_rng(1000 * M + 10 * N + weighted)
    pred, x, y = EM.int_data(rng, N, M, O, H, W, OY, OX, HC, WC)
    wgt = dyadic_map() if weighted else None
    ow = dyadic_table(3) if weighted else None
    ow_row = [(2 * n + 1) % 3 for n in range(N)] if weighted else None
    if weighted:
        y[:, :, 3, 5] = np.nan                                       # a NaN target under a zero cell weight
        y[np.asarray(ow_row) == 0, 2] = np.nan                       # ... and under a zero output weight
    pre = LM.pairs_int(x, y) if M == 64 else LM.pairs(x, y)
    stats0 = np.array([3.0, 5.0, -2.0, 7.0, 11.0, 0.5, 0.25, 2.0])
    ens0 = np.array([4.0, 1.0, 9.0, 11.0])
    for alpha in (0.0, 0.5, 1.0):
        ref = LM.run(x, y, alpha, wgt, ow, ow_row, stats0, ens0, pre=pre)
        assert np.isfinite(ref["stats"]).all() and np.isfinite(ref["loss"])
        got = run_contiguous(lib, pred, y, M, alpha, wgt, ow, ow_row, stats0, ens0)
        check_all(got, ref, f"M={M} N={N} alpha={alpha} weighted={weighted}", M, alpha, stats0, ens0)
    live = ref["live"]
    assert (x[:, 0] == y)[live].any() and (x[:, 0] == x[:, 1])[live].any()       # ties with the target and among members
    assert weighted == (not live.all())


# =========================================================================== normal data: dpred bits, sums within the any-order bound
@pytest.mark.parametrize("M,alpha", [(2, 1.0), (3, 0.5), (8, 0.0)])
def test_normal_data_dpred_bits_sums_within_the_any_order_bound_and_reproducible(lib, M, alpha):
    N = 3
    rng = np.random.default_rng(300 + M)
    x = rng.standard_normal((N, M, O, HC, WC)).astype(np.float32)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    pred = np.full((N, M, O, H, W), np.nan, np.float32)
    pred[:, :, :, OY:OY + HC, OX:OX + WC] = x
    wgt = (0.25 + rng.random((HC, WC))).astype(np.float32)
    wgt[2, 2] = 0.0
    ow = (0.5 + rng.random((2, O))).astype(np.float32)
    ow[1, 4] = 0.0
    ow_row = [1, 0, 1]
    q, w, cnt = LM.weights(N, O, HC, WC, wgt, ow, ow_row)
    ref = LM.cells(x, y, alpha, q, w, cnt)
    a = run_contiguous(lib, pred, y, M, alpha, wgt, ow, ow_row)
    b = run_contiguous(lib, pred, y, M, alpha, wgt, ow, ow_row)
    for u, v, what in zip(a, b, ("dpred", "loss_out", "stats", "ens_out")):
        SM.check_equal(u, v, f"{what}: second run")
    dp, loss, stats, ens = a
    SM.check_equal(dp, LM.full_images(ref["dpred"], H, W, OY, OX), "dpred")
    bounds = LM.total_bounds(x, y, q, w)
    got = {"SA": ens[0], "SD": ens[1], "SV": ens[2], "S2": stats[0], "S1": stats[1], "Sy": stats[2], "Syy": stats[3]}
    worst = 0.0
    for k, name in enumerate(LM.TERMS):
        exact, bound = bounds[k]
        err = abs(Fraction(float(got[name])) - exact)
        print(f"  M = {M} {name}: got {got[name]!r}, exact {float(exact)!r}, |error| {float(err):.3e}, bound {float(bound):.3e}")
        assert np.isfinite(got[name]) and err <= bound, name
        worst = max(worst, float(err / bound))
    assert stats[4] == cnt and ens[3] == cnt and stats[7] == 1.0
    # the closing expressions, from the device's own sums: the bits of the documented order
    want_loss, want_stats, _ = LM.finish([got[n] for n in LM.TERMS], M, alpha, cnt)
    SM.check_equal(loss, np.array([want_loss], np.float32), "loss_out from the device's sums")
    SM.check_equal(stats, want_stats, "stats from the device's sums")
    print(f"  M = {M}: largest |error| / bound {worst:.3e}")


# =========================================================================== ties, placed on purpose, on non-integer data
def test_ties_between_members_and_with_the_target(lib):
    N, M, alpha = 2, 3, 1.0
    rng = np.random.default_rng(41)
    x = rng.standard_normal((N, M, O, HC, WC)).astype(np.float32)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    x[:, 1, :, 0, :] = x[:, 0, :, 0, :]                  # x_0 == x_1 along crop row 0
    y[:, :, 1, :] = x[:, 2, :, 1, :]                     # x_2 == t along crop row 1
    x[:, :, :, 12, 30:] = x[:, :1, :, 12, 30:]           # all members equal, in the last (partial) wave
    y[:, :, 12, 33:] = x[:, 0, :, 12, 33:]               # ... and on the target: every gradient +0
    pred = np.full((N, M, O, H, W), np.nan, np.float32)
    pred[:, :, :, OY:OY + HC, OX:OX + WC] = x
    q, w, cnt = LM.weights(N, O, HC, WC)
    ref = LM.cells(x, y, alpha, q, w, cnt)
    g = ref["dpred"]
    assert (g[:, :, :, 12, 33:] == 0).all() and not np.signbit(g[:, :, :, 12, 33:]).any()
    R2 = LM.pairs(x, y)["R"][:, 2, :, 1, :]
    assert (g[:, 2, :, 1, :] == (((0.0 / M - LM.kp_of(M, alpha) * R2) * (1.0 / cnt)) * 1.0).astype(np.float32)).all()      # sgn(x_2 - t) = 0 there
    dp, _, _, _ = run_contiguous(lib, pred, y, M, alpha)
    SM.check_equal(dp, LM.full_images(g, H, W, OY, OX), "dpred")


# =========================================================================== NaN and zero weights
def test_nan_target_under_zero_weight_is_harmless_and_a_nan_member_stays_in_its_cell(lib):
    N, M, alpha = 2, 4, 0.5
    rng = np.random.default_rng(61)
    pred, x, y = EM.int_data(rng, N, M, O, H, W, OY, OX, HC, WC)
    wgt = dyadic_map()
    y[:, :, 3, 5] = np.nan
    y[:, :, 12, 36] = np.nan
    ref = LM.run(x, y, alpha, wgt)
    got = run_contiguous(lib, pred, y, M, alpha, wgt)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all() and np.isfinite(got[3]).all()
    check_all(got, ref, "NaN targets under zero weights", M, alpha)
    # one NaN member under a live weight: its cell's M gradients and the loss are NaN, and no other dpred
    x[1, 2, 4, 6, 9] = np.nan
    pred[1, 2, 4, OY + 6, OX + 9] = np.nan
    ref = LM.run(x, y, alpha, wgt)
    dp, loss, stats, ens = run_contiguous(lib, pred, y, M, alpha, wgt)
    nan = np.zeros(dp.shape, bool)
    nan[1, :, 4, OY + 6, OX + 9] = True
    assert np.array_equal(np.isnan(dp), nan) and np.isnan(loss[0]) and np.isnan(ens[0]) and np.isnan(ens[1]) and np.isnan(ens[2])
    want = LM.full_images(ref["dpred"], H, W, OY, OX)
    assert np.array_equal(np.isnan(want), nan)
    SM.check_equal(np.where(nan, 0.0, dp).astype(np.float32), np.where(nan, 0.0, want).astype(np.float32), "dpred off the NaN cell")
    assert np.isfinite(stats[[2, 3, 4, 7]]).all() and stats[4] == ref["cnt"]


# =========================================================================== outside the crop: +0, sign bit included
def test_outside_the_crop_is_plus_zero(lib):
    N, M = 2, 3
    rng = np.random.default_rng(71)
    pred = rng.standard_normal((N, M, O, H, W)).astype(np.float32)          # finite data outside the crop too: it must not be used
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    dp, _, _, _ = run_contiguous(lib, pred, y, M, 1.0)
    out = np.ones((H, W), bool)
    out[OY:OY + HC, OX:OX + WC] = False
    assert (dp[..., out].view(np.uint32) == 0).all()
    other = pred.copy()
    other[..., out] = np.nan
    dp2, _, _, _ = run_contiguous(lib, other, y, M, 1.0)
    SM.check_equal(dp2, dp, "dpred does not depend on what lies outside the crop")


# =========================================================================== addressing: the roll-out layouts, in place
def test_rollout_layouts_equal_contiguous_copies(lib):
    """reads head_forward_seq's (lanes, T, O, H, W), lanes n*M + m: sample (n, t) at ((n*M)*T + t) images, member stride T images;
    writes the roll-out slab (T*B, O, H, W): sample (n, t) at (t*B + n*M) images, member stride one image.  Samples (n, t) in y's
    order for the steps t >= 1; the slab's images of step 0 are not listed and must keep what they held."""
    Ns, M, T, alpha = 2, 3, 3, 0.5
    B, img = Ns * M, O * H * W
    rng = np.random.default_rng(31)
    seq = rng.standard_normal((B, T, O, H, W)).astype(np.float32)
    pairs = [(n, t) for n in range(Ns) for t in range(1, T)]
    N = len(pairs)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    ow = (0.5 + rng.random((T, O))).astype(np.float32)
    ow_row = [t for _, t in pairs]
    q, w, cnt = LM.weights(N, O, HC, WC, None, ow, ow_row)
    slab = torch.full((T * B, O, H, W), 7.0, device="cuda")
    poff = [((n * M) * T + t) * img for n, t in pairs]
    doff = [(t * B + n * M) * img for n, t in pairs]
    a = call(lib, dev(seq), poff, T * img, slab, doff, img, M, dev(y), alpha, cnt, None, dev(ow), ow_row)
    copy = np.stack([np.stack([seq[n * M + m, t] for m in range(M)]) for n, t in pairs])          # (N, M, O, H, W)
    off, _ = contiguous(N, M)
    dp = torch.full((N, M, O, H, W), NAN, device="cuda")
    b = call(lib, dev(copy), off, img, dp, off, img, M, dev(y), alpha, cnt, None, dev(ow), ow_row)
    for u, v, what in zip(a, b, ("loss_out", "stats", "ens_out")):
        SM.check_equal(host(u), host(v), what)
    got, flat = host(slab).reshape(T, Ns, M, O, H, W), host(dp)
    for i, (n, t) in enumerate(pairs):
        SM.check_equal(got[t, n], flat[i], f"slab images of sample {(n, t)}")
    assert (got[0] == 7.0).all()
    ref = LM.cells(copy[:, :, :, OY:OY + HC, OX:OX + WC], y, alpha, q, w, cnt)
    SM.check_equal(flat, LM.full_images(ref["dpred"], H, W, OY, OX), "dpred against the model")


# =========================================================================== cuts: N beyond one piece, and two calls
def test_seventy_samples_in_one_call_and_as_six_plus_sixty_four(lib):
    N, M, alpha, k = 70, 2, 1.0, 6
    rng = np.random.default_rng(51)
    x = rng.standard_normal((N, M, O, HC, WC)).astype(np.float32)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    pred = np.full((N, M, O, H, W), np.nan, np.float32)
    pred[:, :, :, OY:OY + HC, OX:OX + WC] = x
    q, w, cnt = LM.weights(N, O, HC, WC)
    off, img = contiguous(N, M)
    pd, yd = dev(pred), dev(y)
    dp1 = torch.full((N, M, O, H, W), NAN, device="cuda")
    _, s1, e1 = call(lib, pd, off, img, dp1, off, img, M, yd, alpha, cnt)
    dp2 = torch.full((N, M, O, H, W), NAN, device="cuda")
    stats, ens = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    call(lib, pd, off[:k], img, dp2, off[:k], img, M, yd[:k], alpha, cnt, stats=stats, ens=ens)       # the same cnt: the same gradients
    call(lib, pd, off[k:], img, dp2, off[k:], img, M, yd[k:], alpha, cnt, stats=stats, ens=ens)
    SM.check_equal(host(dp2), host(dp1), "dpred of 6 + 64")
    ref = LM.cells(x, y, alpha, q, w, cnt)
    SM.check_equal(host(dp1), LM.full_images(ref["dpred"], H, W, OY, OX), "dpred against the model")
    bounds = LM.order_bounds(ref["terms"], ref["live"])       # (168 350 cells: the any-order bound of the model's own terms)
    s1, e1, s2, e2 = host(s1), host(e1), host(stats), host(ens)
    for name, one, two in (("SA", e1[0], e2[0]), ("SD", e1[1], e2[1]), ("SV", e1[2], e2[2]), ("S2", s1[0], s2[0]), ("S1", s1[1], s2[1]),
                           ("Sy", s1[2], s2[2]), ("Syy", s1[3], s2[3])):
        exact, bound = bounds[LM.TERMS.index(name)]
        for v in (one, two):            # (two calls: one more addition joins them -- within the same bound's count of n_live - 1)
            assert abs(float(v) - exact) <= bound, (name, v, exact, bound)
    assert s1[4] == cnt and s2[4] == 2 * cnt and e1[3] == cnt and e2[3] == 2 * cnt


# =========================================================================== the memory contract
def test_memory_contract_guards_intact_and_poison_unread(lib):
    N, M, alpha = 3, 8, 0.5
    rng = np.random.default_rng(81)
    pred = rng.standard_normal((N, M, O, H, W)).astype(np.float32)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    wgt = (0.25 + rng.random((HC, WC))).astype(np.float32)
    ow = (0.5 + rng.random((2, O))).astype(np.float32)
    ow_row = [1, 0, 1]
    q, w, cnt = LM.weights(N, O, HC, WC, wgt, ow, ow_row)
    off, img = contiguous(N, M)

    def run(alloc, wrap):
        dp = alloc.empty(N, M, O, H, W, dtype=torch.float32, device="cuda")
        loss, stats, ens = call(lib, wrap(dev(pred)), off, img, dp, off, img, M, wrap(dev(y)), alpha, cnt, wrap(dev(wgt)), wrap(dev(ow)),
                                ow_row, alloc=alloc, nan_fill=False)
        torch.cuda.synchronize()
        return dp, loss, stats, ens

    plain = run(torch, lambda t: t)
    for mode in ("zero", "poison"):
        gt = GuardedTorch(mode)
        got = run(gt, gt.guard_copy)
        assert gt.verify() == 9                            # dpred, scratch, loss, stats, ens and the four inputs
        for a, b, what in zip(got, plain, ("dpred", "loss_out", "stats", "ens_out")):
            assert same_bits(a, b), f"{what} under {mode}"
