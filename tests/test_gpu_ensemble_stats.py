"""nint_ens_accum (csrc/ensemble.hip) against tests/ensemble_model.py, at the smallest shapes at which the kernel
can go wrong: a crop of 481 pixels (a second workgroup that is partly dead), O = 5 (a group of four outputs and a remainder),
M = 2, 3, 8 and the largest, 64; samples in non-monotone slot order with one left out and one slot that no sample names.

Integer data: every f64 sum is exact in any order, so every plane, sample column and bin must have the model's bits.
Random data: every value is held to the bound of ANY summation order against the exact value (python fractions):
    |got - exact| <= g(additions feeding the value + roundings inside one term) * sum of the terms' magnitudes,
g(k) = k u / (1 - k u), u = 2^-53; the counts are derived in ensemble_model.exact_cell -- nothing here is measured."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import ensemble_model as EM
from oracle import small_audit as SM
from oracle.guarded_alloc import GuardedTorch, same_bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
H, W, OY, OX, HC, WC = 17, 41, 2, 3, 13, 37
SENTINEL = np.frombuffer(np.uint64(0x7FF8_0000_DEAD_BEEF).tobytes(), np.float64)[0]     # a NaN whose payload must come back


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


def call(lib, pred, off, stride, M, y, slots, nslots, row_w, pix, hist, grid=(H, W), at=(OY, OX), mean=None, alloc=torch,
         nan_fill=True):
    """one nint_ens_accum call on device tensors; pix and hist grow in place; returns the sample rows.  sample and scratch
    start as NaN (they are overwritten / never read before written); the scratch has exactly the queried size."""
    N, O, Hc, Wc = y.shape
    nb = lib.nint_ens_scratch_bytes(N, M, O, Hc, Wc)
    assert nb == min(N, 64) * O * ((Hc * Wc + 255) // 256) * 4 * EM.SAMPLE * 8
    sample = alloc.empty(N, O, EM.SAMPLE, dtype=torch.float64, device="cuda")
    scratch = alloc.empty(nb // 8, dtype=torch.float64, device="cuda")
    if nan_fill:
        sample.fill_(NAN)
        scratch.fill_(NAN)
    sl = None if slots is None else (C.c_int32 * N)(*[int(v) for v in slots])
    rc = lib.nint_ens_accum(P(pred), (C.c_int64 * N)(*[int(v) for v in off]), int(stride), M, P(y), sl, nslots, P(row_w), P(pix),
                            P(sample), P(hist), P(mean), P(scratch), nb, N, O, grid[0], grid[1], at[0], at[1], Hc, Wc, None)
    assert rc == 0, rc
    return sample


def contiguous_offsets(N, M, O, grid=(H, W)):
    img = O * grid[0] * grid[1]
    return [n * M * img for n in range(N)], img


def before(nslots, O, M, Hc=HC, Wc=WC, seed=5):
    """non-zero integer maps and counts to grow from; the LAST slot is the one no sample names: a NaN sentinel and odd counts"""
    rng = np.random.default_rng(seed)
    pix = rng.integers(-4, 5, (nslots, EM.PIX, O, Hc, Wc)).astype(np.float64)
    pix[nslots - 1] = SENTINEL
    hist = rng.integers(0, 9, (nslots, O, M + 2)).astype(np.int64)
    return pix, hist


# =========================================================================== integer data: equal bits
@pytest.mark.parametrize("M", [2, 3, 8, 64])
def test_bits_on_integer_data(lib, M):
    N, O, slots, nslots = 3, 5, [1, -1, 0], 3
    rng = np.random.default_rng(100 + M)
    pred, x, y = EM.int_data(rng, N, M, O, H, W, OY, OX, HC, WC)
    row_w = EM.dyadic_rows(HC)
    pix0, hist0 = before(nslots, O, M)
    ref = EM.sums(x, y, slots, nslots, row_w, pix0, hist0)
    rk = EM.cells(x, y)["rank"]
    assert (rk == 0).any() and (rk == M).any() and (x == y[:, None]).any() and (rk <= M).all()      # what the data must contain
    pix, hist, mean = dev(pix0), dev(hist0), torch.full((N, O, HC, WC), NAN, device="cuda")
    off, img = contiguous_offsets(N, M, O)
    sample = call(lib, dev(pred), off, img, M, dev(y), slots, nslots, dev(row_w), pix, hist, mean=mean)
    got_pix, got_hist = host(pix), host(hist)
    SM.check_equal(got_pix, ref["pix"], "pix")
    SM.check_equal(host(sample), ref["sample"], "sample")
    SM.check_equal(got_hist, ref["rank_hist"], "rank_hist")
    SM.check_equal(host(mean), ref["mean"], "mean_out")
    SM.check_equal(got_pix[2], pix0[2], "the slot no sample names")
    SM.check_equal(got_hist[2], hist0[2], "the bins of the slot no sample names")
    added = (got_hist - hist0).sum(axis=2)                                      # per (slot, output): the cells folded in
    assert (added[:2] == HC * WC).all() and (added[2] == 0).all()
    # identical members: V = D = 0 there and A = M |x - t| (ensemble_model.int_data plants them at crop pixel (1, 0))
    t = ref["terms"]
    assert (t[1][:, :, 1, 0] == 0).all() and (t[3][:, :, 1, 0] == 0).all()


# =========================================================================== random data: the any-order bound, equal bits twice
@pytest.mark.parametrize("M", [3, 8])
def test_random_data_within_the_any_order_bound_and_reproducible(lib, M):
    N, O, slots, nslots = 4, 2, [1, 0, 1, -1], 3
    rng = np.random.default_rng(200 + M)
    x = rng.standard_normal((N, M, O, HC, WC)).astype(np.float32)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    pred = np.full((N, M, O, H, W), np.nan, np.float32)
    pred[:, :, :, OY:OY + HC, OX:OX + WC] = x
    row_w = 0.25 + rng.random(HC)
    pix0 = np.zeros((nslots, EM.PIX, O, HC, WC))
    pix0[:2] = rng.standard_normal(pix0[:2].shape)
    pix0[2] = SENTINEL
    hist0 = np.zeros((nslots, O, M + 2), np.int64)
    off, img = contiguous_offsets(N, M, O)
    runs = []
    for _ in range(2):
        pix, hist = dev(pix0), dev(hist0)
        sample = call(lib, dev(pred), off, img, M, dev(y), slots, nslots, dev(row_w), pix, hist)
        runs.append((host(pix), host(sample), host(hist)))
    for a, b, what in zip(runs[0], runs[1], ("pix", "sample", "rank_hist")):
        SM.check_equal(a, b, f"{what}: second run")
    got_pix, got_smp, got_hist = runs[0]
    # exact terms per cell
    val = np.empty((EM.PIX, N, O, HC, WC), object)
    mag = np.empty((EM.PIX, N, O, HC, WC), object)
    for n in range(N):
        for o in range(O):
            for cy in range(HC):
                for cx in range(WC):
                    v, m, rnd = EM.exact_cell(x[n, :, o, cy, cx], y[n, o, cy, cx])
                    val[:, n, o, cy, cx], mag[:, n, o, cy, cx] = v, m
    worst = [0.0, 0.0]

    def hold(got, exact, bound, k, what):
        err = abs(Fraction(float(got)) - exact)
        assert np.isfinite(got) and err <= bound, f"{what}: got {got!r}, exact {float(exact)!r}, |error| {float(err):.3e}, bound {float(bound):.3e}"
        if bound > 0:
            worst[k] = max(worst[k], float(err / bound))

    # a map cell: the stored value and the slot's samples, (addends - 1) additions
    for s in range(2):
        members = [n for n in range(N) if slots[n] == s]
        for k in range(EM.PIX):
            for o in range(O):
                for cy in range(HC):
                    for cx in range(WC):
                        b0 = Fraction(float(pix0[s, k, o, cy, cx]))
                        exact = b0 + sum(val[k, n, o, cy, cx] for n in members)
                        mags = abs(b0) + sum(mag[k, n, o, cy, cx] for n in members)
                        hold(got_pix[s, k, o, cy, cx], exact, EM.gamma(len(members) + rnd[k]) * mags, 0, f"pix{(s, k, o, cy, cx)}")
    SM.check_equal(got_pix[2], pix0[2], "the slot no sample names")
    # a sample row: Hc * Wc terms in a tree, Hc * Wc - 1 additions; a weighted column's product is one rounding more
    npx = HC * WC
    rwf = [Fraction(float(v)) for v in row_w]
    for n in range(N):
        for o in range(O):
            for k in range(4):
                exact = sum(val[k, n, o].reshape(-1).tolist())
                mags = sum(mag[k, n, o].reshape(-1).tolist())
                hold(got_smp[n, o, k], exact, EM.gamma(npx - 1 + rnd[k]) * mags, 1, f"sample{(n, o, k)}")
                exact = sum(rwf[cy] * val[k, n, o, cy, cx] for cy in range(HC) for cx in range(WC))
                mags = sum(rwf[cy] * mag[k, n, o, cy, cx] for cy in range(HC) for cx in range(WC))
                hold(got_smp[n, o, k + 4], exact, EM.gamma(npx + rnd[k]) * mags, 1, f"sample{(n, o, k + 4)}")
    print(f"  M = {M}: largest |error| / bound: maps {worst[0]:.3e}, sample rows {worst[1]:.3e}")
    # the maps grow in the documented order, one f64 operation per product and per sum: the numpy model's bits
    ref = EM.sums(x, y, slots, nslots, row_w, pix0, hist0)
    SM.check_equal(got_pix, ref["pix"], "pix in the documented order")
    SM.check_equal(got_hist, ref["rank_hist"], "rank_hist")


# =========================================================================== addressing: a roll-out's layout, read in place
def test_rollout_layout_equals_a_contiguous_copy(lib):
    """(lanes, T, O, H, W) with lanes = start * M + member, T = 4, spinup = 1: sample (start, lead j) at ((start * M) * T + 1 + j)
    images, member stride T images (larger than one image); the samples in shuffled order, one of them twice."""
    M, O, T, spinup, starts = 3, 5, 4, 1, 2
    img = O * H * W
    rng = np.random.default_rng(31)
    buf = rng.standard_normal((starts * M, T, O, H, W)).astype(np.float32)
    pairs = [(1, 2), (0, 0), (1, 0), (0, 2), (0, 1), (1, 1), (0, 0)]            # unordered, (0, 0) twice: overlapping reads
    off = [((s * M) * T + spinup + j) * img for s, j in pairs]
    slots, nslots, N = [j for _, j in pairs], 3, len(pairs)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    row_w = 0.25 + rng.random(HC)
    copy = np.stack([np.stack([buf[s * M + m, spinup + j] for m in range(M)]) for s, j in pairs])      # (N, M, O, H, W)
    out = []
    for pred, offs, stride in ((buf, off, T * img), (copy, contiguous_offsets(N, M, O)[0], img)):
        pix = torch.zeros(nslots, EM.PIX, O, HC, WC, dtype=torch.float64, device="cuda")
        hist = torch.zeros(nslots, O, M + 2, dtype=torch.int64, device="cuda")
        mean = torch.full((N, O, HC, WC), NAN, device="cuda")
        sample = call(lib, dev(pred), offs, stride, M, dev(y), slots, nslots, dev(row_w), pix, hist, mean=mean)
        out.append((host(pix), host(sample), host(hist), host(mean)))
    for a, b, what in zip(out[0], out[1], ("pix", "sample", "rank_hist", "mean_out")):
        SM.check_equal(a, b, what)
    ref = EM.sums(copy[:, :, :, OY:OY + HC, OX:OX + WC], y, slots, nslots, row_w, np.zeros((nslots, EM.PIX, O, HC, WC)),
                  np.zeros((nslots, O, M + 2), np.int64))
    SM.check_equal(out[0][0], ref["pix"], "pix against the model")
    SM.check_equal(out[0][2], ref["rank_hist"], "rank_hist against the model")


# =========================================================================== accumulation: splits, and N beyond one launch
def test_one_call_equals_two_consecutive_calls(lib):
    N, M, O, nslots, k = 6, 8, 5, 3, 2
    slots = [1, 0, -1, 1, 0, 1]
    rng = np.random.default_rng(41)
    pred = rng.standard_normal((N, M, O, H, W)).astype(np.float32)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    pix0, hist0 = before(nslots, O, M)
    off, img = contiguous_offsets(N, M, O)
    pd, yd = dev(pred), dev(y)
    pix, hist = dev(pix0), dev(hist0)
    whole = call(lib, pd, off, img, M, yd, slots, nslots, None, pix, hist)
    pix2, hist2 = dev(pix0), dev(hist0)
    a = call(lib, pd, off[:k], img, M, yd[:k], slots[:k], nslots, None, pix2, hist2)
    b = call(lib, pd, off[k:], img, M, yd[k:], slots[k:], nslots, None, pix2, hist2)
    SM.check_equal(host(pix2), host(pix), "pix of 2 + 4")
    SM.check_equal(host(hist2), host(hist), "rank_hist of 2 + 4")
    SM.check_equal(host(torch.cat([a, b])), host(whole), "sample of 2 + 4")


def test_more_samples_than_one_launch_holds(lib):
    N, M, O, Hc, Wc, grid, at, nslots = 70, 2, 1, 3, 5, (5, 8), (1, 2), 4
    slots = [(2 * n) % 3 if n % 7 else -1 for n in range(N)]                  # 0..2 in non-monotone order, -1 among them; 3 stays empty
    rng = np.random.default_rng(51)
    pred, x, y = EM.int_data(rng, N, M, O, grid[0], grid[1], at[0], at[1], Hc, Wc)
    row_w = EM.dyadic_rows(Hc)
    pix0, hist0 = before(nslots, O, M, Hc, Wc)
    ref = EM.sums(x, y, slots, nslots, row_w, pix0, hist0)
    pix, hist = dev(pix0), dev(hist0)
    off, img = contiguous_offsets(N, M, O, grid)
    sample = call(lib, dev(pred), off, img, M, dev(y), slots, nslots, dev(row_w), pix, hist, grid=grid, at=at)
    SM.check_equal(host(pix), ref["pix"], "pix")
    SM.check_equal(host(sample), ref["sample"], "sample")
    SM.check_equal(host(hist), ref["rank_hist"], "rank_hist")


# =========================================================================== NaN
def test_nan_cells_are_counted_and_spread_as_the_arithmetic_gives(lib):
    N, M, O, nslots = 2, 4, 5, 1
    rng = np.random.default_rng(61)
    pred, x, y = EM.int_data(rng, N, M, O, H, W, OY, OX, HC, WC)
    x[0, 2, 1, 4, 7] = np.nan                               # one member of cell (n 0, o 1, 4, 7)
    pred[0, 2, 1, OY + 4, OX + 7] = np.nan
    y[1, 4, 12, 36] = np.nan                                # the target of the crop's last pixel, second workgroup
    zero_p, zero_h = np.zeros((nslots, EM.PIX, O, HC, WC)), np.zeros((nslots, O, M + 2), np.int64)
    ref = EM.sums(x, y, None, nslots, None, zero_p, zero_h)
    pix, hist = dev(zero_p), dev(zero_h)
    off, img = contiguous_offsets(N, M, O)
    sample = call(lib, dev(pred), off, img, M, dev(y), None, nslots, None, pix, hist)
    got_pix, got_hist, got_smp = host(pix), host(hist), host(sample)
    SM.check_equal(got_hist, ref["rank_hist"], "rank_hist")
    assert got_hist[0, 1, M + 1] == 1 and got_hist[0, 4, M + 1] == 1 and got_hist[0, :, M + 1].sum() == 2
    assert (got_hist[0].sum(axis=1) == N * HC * WC).all()
    for got, want, what in ((got_pix, ref["pix"], "pix"), (got_smp, ref["sample"], "sample")):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        SM.check_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want), f"{what} off the NaN cells")
    # the NaN member: S, so E^2, V, A, D and E; the NaN target: E^2, A, E, t, t^2 -- V and D of that cell stay finite
    assert np.isnan(got_pix[0, [0, 1, 2, 3, 4], 1, 4, 7]).all() and np.isfinite(got_pix[0, [5, 6], 1, 4, 7]).all()
    assert np.isnan(got_pix[0, [0, 2, 4, 5, 6], 4, 12, 36]).all() and np.isfinite(got_pix[0, [1, 3], 4, 12, 36]).all()
    assert np.isnan(got_pix).sum() == 10


# =========================================================================== mean_out
def test_mean_out_is_the_rounded_quotient(lib):
    N, M, O = 2, 4, 5
    rng = np.random.default_rng(71)
    x = rng.standard_normal((N, M, O, HC, WC)).astype(np.float32)
    pred = np.full((N, M, O, H, W), np.nan, np.float32)
    pred[:, :, :, OY:OY + HC, OX:OX + WC] = x
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    S = ((x[:, 0].astype(np.float64) + x[:, 1]) + x[:, 2]) + x[:, 3]
    pix = torch.zeros(1, EM.PIX, O, HC, WC, dtype=torch.float64, device="cuda")
    hist = torch.zeros(1, O, M + 2, dtype=torch.int64, device="cuda")
    mean = torch.full((N, O, HC, WC), NAN, device="cuda")
    off, img = contiguous_offsets(N, M, O)
    call(lib, dev(pred), off, img, M, dev(y), [-1, 0], 1, None, pix, hist, mean=mean)       # also for a sample left out of the maps
    SM.check_equal(host(mean), (S / 4.0).astype(np.float32), "mean_out")


# =========================================================================== the memory contract
def test_memory_contract_guards_intact_and_poison_unread(lib):
    N, M, O, nslots, slots = 3, 8, 5, 3, [1, -1, 0]
    rng = np.random.default_rng(81)
    pred = rng.standard_normal((N, M, O, H, W)).astype(np.float32)
    y = rng.standard_normal((N, O, HC, WC)).astype(np.float32)
    row_w = 0.25 + rng.random(HC)
    off, img = contiguous_offsets(N, M, O)

    def run(alloc, wrap):
        pix = alloc.zeros(nslots, EM.PIX, O, HC, WC, dtype=torch.float64, device="cuda")
        hist = alloc.zeros(nslots, O, M + 2, dtype=torch.int64, device="cuda")
        mean = alloc.empty(N, O, HC, WC, dtype=torch.float32, device="cuda")
        sample = call(lib, wrap(dev(pred)), off, img, M, wrap(dev(y)), slots, nslots, wrap(dev(row_w)), pix, hist, mean=mean,
                      alloc=alloc, nan_fill=False)
        torch.cuda.synchronize()
        return pix, sample, hist, mean

    plain = run(torch, lambda t: t)
    for mode in ("zero", "poison"):
        gt = GuardedTorch(mode)
        got = run(gt, gt.guard_copy)
        assert gt.verify() == 8                            # pix, hist, mean, sample, scratch and the three inputs
        for a, b, what in zip(got, plain, ("pix", "sample", "rank_hist", "mean_out")):
            assert same_bits(a, b), f"{what} under {mode}"
