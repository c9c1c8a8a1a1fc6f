"""nint_spec_accum (csrc/spectrum.hip) against tests/spectrum_model.py at the smallest shapes at which the kernel
can go wrong: odd and even widths, K below one wave (3, 4), K = 37 and K = 73 (a row tile of three rows that ends in the middle
of the fourth wave), crops of fewer rows than a tile holds and of more (a last tile that is partly dead), M = 1, 2, 3, 8,
samples in non-monotone slot order with one left out and one slot that no sample names.  The crop sits inside a NaN-filled
frame with oy, ox > 0.

Integer data with an integer table: every f64 sum is exact in any order, so every entry must be the exact value, bit for bit.
Random data with the library's table: every entry is held to the bound of ANY evaluation order against the exact value formed
from the table's own f64 entries,   |got - exact| <= gamma(n_ops) * (|stored| + sum of the terms' magnitudes),
with n_ops counted from the order include/nint.h documents (spectrum_model.n_ops) -- nothing here is measured."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import spectrum_model as SP
from oracle import small_audit as SM
from oracle.guarded_alloc import GuardedTorch, same_bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
OY, OX = 2, 3
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


def frame(Hc, Wc):
    return Hc + OY + 1, Wc + OX + 2


def real_table(lib, Wc):
    tw = np.empty((Wc, 2))
    assert lib.nint_spec_twiddles(Wc, tw.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return tw


def call(lib, pred, off, stride, M, y, slots, nslots, row_w, tw, spec, grid, at=(OY, OX), alloc=torch, nan_fill=True):
    """one nint_spec_accum call on device tensors; spec grows in place.  The scratch has exactly the queried size and starts
    as NaN (it is never read before it is written)."""
    N, O, Hc, Wc = y.shape
    nb = lib.nint_spec_scratch_bytes(N, M, O, Hc, Wc)
    assert nb == min(N, 64) * O * SP.PLANES * (Wc // 2 + 1) * 8
    scratch = alloc.empty(nb // 8, dtype=torch.float64, device="cuda")
    if nan_fill:
        scratch.fill_(NAN)
    sl = None if slots is None else (C.c_int32 * N)(*[int(v) for v in slots])
    rc = lib.nint_spec_accum(P(pred), (C.c_int64 * N)(*[int(v) for v in off]), int(stride), M, P(y), sl, nslots, P(row_w), P(tw),
                             P(spec), P(scratch), nb, N, O, grid[0], grid[1], at[0], at[1], Hc, Wc, None)
    assert rc == 0, rc
    return scratch


def contiguous_offsets(N, M, O, grid):
    img = O * grid[0] * grid[1]
    return [n * M * img for n in range(N)], img


def framed(x, grid, fill=NAN, rng=None):
    """members on the crop (N, M, O, Hc, Wc) -> (N, M, O, H, W) with the crop at (OY, OX) and `fill` (or noise) around it"""
    N, M, O, Hc, Wc = x.shape
    pred = np.full((N, M, O) + tuple(grid), fill, np.float32) if rng is None else rng.standard_normal((N, M, O) + tuple(grid)).astype(np.float32)
    pred[:, :, :, OY:OY + Hc, OX:OX + Wc] = x
    return pred


def random_case(rng, N, M, O, Hc, Wc):
    x = rng.standard_normal((N, M, O, Hc, Wc)).astype(np.float32)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(np.float32)
    return x, y, 0.25 + rng.random(Hc)


def run(lib, x, y, tw, slots, nslots, row_w, spec0=None, **kw):
    N, M, O, Hc, Wc = x.shape
    grid = frame(Hc, Wc)
    off, img = contiguous_offsets(N, M, O, grid)
    spec = dev(np.zeros((nslots, SP.PLANES, O, Wc // 2 + 1)) if spec0 is None else spec0)
    call(lib, dev(framed(x, grid)), off, img, M, dev(y), slots, nslots, dev(row_w), dev(tw), spec, grid, **kw)
    return host(spec)


def within_bound(got, spec0, x, y, tw, row_w, slots, check_slots):
    """every entry of the named slots against the exact value grown from spec0, to the any-order bound of the documented order;
    returns the largest |error| / bound"""
    N, M, O, Hc, Wc = x.shape
    val, mag = SP.exact_planes(x, y, tw, row_w)
    worst = 0.0
    for s in check_slots:
        members = [n for n in range(N) if slots[n] == s]
        g = SP.gamma(SP.n_ops(Wc, M, Hc, len(members)))
        for idx in np.ndindex(SP.PLANES, O, Wc // 2 + 1):
            b0 = Fraction(float(spec0[(s,) + idx]))
            exact = b0 + sum(val[(n,) + idx] for n in members)
            bound = g * (abs(b0) + sum(mag[(n,) + idx] for n in members))
            v = got[(s,) + idx]
            assert np.isfinite(v), f"spec{(s,) + idx}: got {v!r}, exact {float(exact)!r}"
            err = abs(Fraction(float(v)) - exact)
            assert err <= bound, f"spec{(s,) + idx}: got {v!r}, exact {float(exact)!r}, |error| {float(err):.3e}, bound {float(bound):.3e}"
            if bound > 0:
                worst = max(worst, float(err / bound))
    return worst


# =========================================================================== 1. integer data, integer table: exact bits
@pytest.mark.parametrize("Wc,Hc,M", [(4, 3, 1), (7, 5, 3), (6, 2, 2), (72, 3, 8), (144, 2, 2)])
def test_bits_on_integer_data_with_an_integer_table(lib, Wc, Hc, M):
    N, O, slots, nslots = 3, 2, [1, -1, 0], 3
    K = Wc // 2 + 1
    rng = np.random.default_rng(1000 * Wc + M)
    assert SP.int_magnitude_bound(Wc, Hc, M, N) < 2 ** 45                            # far below 2^53: every sum is exact
    grid = frame(Hc, Wc)
    pred, x, y = SP.int_data(rng, N, M, O, grid[0], grid[1], OY, OX, Hc, Wc)
    pred[1] = np.nan                                                            # the sample that is left out is never read
    tw, row_w = SP.int_table(rng, Wc), SP.dyadic_rows(Hc)
    spec0 = rng.integers(-4, 5, (nslots, SP.PLANES, O, K)).astype(np.float64)
    spec0[2] = SENTINEL                                                         # the slot no sample names
    spec = dev(spec0)
    off, img = contiguous_offsets(N, M, O, grid)
    call(lib, dev(pred), off, img, M, dev(y), slots, nslots, dev(row_w), dev(tw), spec, grid)
    got = host(spec)
    SM.check_equal(got[2], spec0[2], "the slot no sample names")
    keep = [0, 2]
    val, _ = SP.exact_planes(x[keep], y[keep], tw, row_w)
    for s, n in ((1, 0), (0, 1)):                                               # slot 1 <- sample 0, slot 0 <- sample 2
        for idx in np.ndindex(SP.PLANES, O, K):
            exact = Fraction(float(spec0[(s,) + idx])) + val[(n,) + idx]
            assert Fraction(float(got[(s,) + idx])) == exact, f"spec{(s,) + idx}: got {got[(s,) + idx]!r}, exact {float(exact)!r}"
    SM.check_equal(got[:2], SP.sums(x[keep], y[keep], tw, [1, 0], nslots, row_w, spec0)[:2], "spec against the numpy model")


# =========================================================================== 2. random data, the library's table
@pytest.mark.parametrize("Wc,Hc,M,N,O", [(144, 3, 3, 4, 2), (9, 4, 1, 3, 2)])
def test_random_data_within_the_any_order_bound_and_reproducible(lib, Wc, Hc, M, N, O):
    slots, nslots = ([1, 0, 1, -1] if N == 4 else [1, 0, 1]), 3
    K = Wc // 2 + 1
    rng = np.random.default_rng(2000 + Wc)
    x, y, row_w = random_case(rng, N, M, O, Hc, Wc)
    tw = real_table(lib, Wc)
    spec0 = np.zeros((nslots, SP.PLANES, O, K))
    spec0[:2] = rng.standard_normal(spec0[:2].shape)
    spec0[2] = SENTINEL
    runs = [run(lib, x, y, tw, slots, nslots, row_w, spec0) for _ in range(2)]
    SM.check_equal(runs[0], runs[1], "spec: second run")
    got = runs[0]
    SM.check_equal(got[2], spec0[2], "the slot no sample names")
    worst = within_bound(got, spec0, x, y, tw, row_w, slots, range(2))
    print(f"  (Wc, Hc, M) = {(Wc, Hc, M)}: largest |error| / bound {worst:.3e}")


# =========================================================================== 3. addressing: a roll-out's layout, read in place
def test_rollout_layout_equals_a_contiguous_copy(lib):
    """(lanes, T, O, H, W) with lanes = start * M + member, T = 4, spinup = 1: sample (start, lead j) at ((start * M) * T + 1 + j)
    images, member stride T images; the samples in shuffled order, one of them twice"""
    M, O, T, spinup, starts, Hc, Wc = 3, 2, 4, 1, 2, 5, 10
    H, W = frame(Hc, Wc)
    img = O * H * W
    rng = np.random.default_rng(31)
    buf = rng.standard_normal((starts * M, T, O, H, W)).astype(np.float32)
    pairs = [(1, 2), (0, 0), (1, 0), (0, 2), (0, 1), (1, 1), (0, 0)]
    off = [((s * M) * T + spinup + j) * img for s, j in pairs]
    slots, nslots, N = [j for _, j in pairs], 3, len(pairs)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(np.float32)
    row_w, tw = 0.25 + rng.random(Hc), real_table(lib, Wc)
    copy = np.stack([np.stack([buf[s * M + m, spinup + j] for m in range(M)]) for s, j in pairs])      # (N, M, O, H, W)
    out = []
    for pred, offs, stride in ((buf, off, T * img), (copy, contiguous_offsets(N, M, O, (H, W))[0], img)):
        spec = torch.zeros(nslots, SP.PLANES, O, Wc // 2 + 1, dtype=torch.float64, device="cuda")
        call(lib, dev(pred), offs, stride, M, dev(y), slots, nslots, dev(row_w), dev(tw), spec, (H, W))
        out.append(host(spec))
    SM.check_equal(out[0], out[1], "in place against the gathered copy")
    within_bound(out[0], np.zeros_like(out[0]), copy[:, :, :, OY:OY + Hc, OX:OX + Wc], y, tw, row_w, slots, range(nslots))


# =========================================================================== 4. accumulation: splits, and N beyond one launch
@pytest.mark.parametrize("Wc,Hc,M,O,N,cut", [(10, 5, 3, 2, 5, 2), (6, 2, 2, 1, 70, 64)])
def test_one_call_equals_consecutive_calls(lib, Wc, Hc, M, O, N, cut):
    nslots = 3
    slots = [(2 * n) % 3 if n % 7 != 3 else -1 for n in range(N)]               # non-monotone, -1 among them
    rng = np.random.default_rng(41 + N)
    x, y, row_w = random_case(rng, N, M, O, Hc, Wc)
    tw = real_table(lib, Wc)
    grid = frame(Hc, Wc)
    off, img = contiguous_offsets(N, M, O, grid)
    pd, yd, rw, td = dev(framed(x, grid)), dev(y), dev(row_w), dev(tw)
    spec0 = rng.standard_normal((nslots, SP.PLANES, O, Wc // 2 + 1))
    whole, parts = dev(spec0), dev(spec0)
    call(lib, pd, off, img, M, yd, slots, nslots, rw, td, whole, grid)
    call(lib, pd, off[:cut], img, M, yd[:cut], slots[:cut], nslots, rw, td, parts, grid)
    call(lib, pd, off[cut:], img, M, yd[cut:], slots[cut:], nslots, rw, td, parts, grid)
    SM.check_equal(host(parts), host(whole), f"{cut} + {N - cut} against {N}")
    within_bound(host(whole), spec0, x, y, tw, row_w, slots, range(nslots))


# =========================================================================== 5. row_w NULL
def test_no_row_weights_is_a_table_of_ones(lib):
    rng = np.random.default_rng(51)
    x, y, _ = random_case(rng, 3, 2, 2, 5, 12)
    tw = real_table(lib, 12)
    a = run(lib, x, y, tw, [0, 1, 0], 2, None)
    b = run(lib, x, y, tw, [0, 1, 0], 2, np.ones(5))
    SM.check_equal(a, b, "row_w NULL against ones")
    assert np.isfinite(a).all() and (a[:, SP.YY] > 0).all()


# =========================================================================== 6. NaN
def test_nan_goes_where_the_arithmetic_takes_it(lib):
    rng = np.random.default_rng(61)
    N, M, O, Hc, Wc = 2, 3, 3, 4, 9
    x, y, row_w = random_case(rng, N, M, O, Hc, Wc)
    tw = real_table(lib, Wc)
    clean = run(lib, x, y, tw, [0, 1], 2, row_w)
    assert np.isfinite(clean).all()
    # a NaN in one target row (sample 0 -> slot 0, output 1): YY, CR, CI of that (slot, output), every k; PP and SS stay finite
    y2 = y.copy()
    y2[0, 1, 2, 5] = np.nan
    got = run(lib, x, y2, tw, [0, 1], 2, row_w)
    bad = ~np.isfinite(got)
    want = np.zeros_like(bad)
    want[0, [SP.YY, SP.CR, SP.CI], 1, :] = True
    assert np.array_equal(bad, want)
    SM.check_equal(np.where(want, 0.0, got), np.where(want, 0.0, clean), "off the NaN entries")
    # a NaN in one member (sample 1 -> slot 1, output 2, member 1): PP, CR, CI, SS; YY stays finite
    x2 = x.copy()
    x2[1, 1, 2, 0, 0] = np.nan
    got = run(lib, x2, y, tw, [0, 1], 2, row_w)
    bad = ~np.isfinite(got)
    want = np.zeros_like(bad)
    want[1, [SP.PP, SP.CR, SP.CI, SP.SS], 2, :] = True
    assert np.array_equal(bad, want)
    SM.check_equal(np.where(want, 0.0, got), np.where(want, 0.0, clean), "off the NaN entries")


# =========================================================================== 7. the memory contract
def test_memory_contract_guards_intact_and_poison_unread(lib):
    N, M, O, Hc, Wc, nslots, slots = 3, 3, 2, 5, 72, 3, [1, -1, 0]
    rng = np.random.default_rng(81)
    x, y, row_w = random_case(rng, N, M, O, Hc, Wc)
    tw = real_table(lib, Wc)
    grid = frame(Hc, Wc)
    off, img = contiguous_offsets(N, M, O, grid)

    def go(alloc, wrap, pred):
        spec = alloc.zeros(nslots, SP.PLANES, O, Wc // 2 + 1, dtype=torch.float64, device="cuda")
        scratch = call(lib, wrap(dev(pred)), off, img, M, wrap(dev(y)), slots, nslots, wrap(dev(row_w)), wrap(dev(tw)), spec, grid,
                       alloc=alloc, nan_fill=False)
        torch.cuda.synchronize()
        return spec, scratch

    plain, _ = go(torch, lambda t: t, framed(x, grid, rng=rng))                 # noise around the crop
    assert np.isfinite(host(plain)).all()
    for mode, fill in (("zero", 0.0), ("poison", NAN)):
        gt = GuardedTorch(mode)
        got, _ = go(gt, gt.guard_copy, framed(x, grid, fill=fill))              # another frame around the same crop
        assert gt.verify() == 6                            # spec, scratch and the four inputs
        assert same_bits(got, plain), f"spec under {mode}"


# =========================================================================== 8. end to end
STARTS, HORIZON, SPINUP, M_ENS, SEED = [1, 7], 3, 2, 3, 11


def _stack(pkg):
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from oracle import convlstm_oracle as OR
    ds = SyntheticE33OMA_CRNN("train", padding=None, in_channels=10, sequence_length=4, levels=2, n_steps=20, grid=(12, 16),
                              device="cuda", tracer_input=True)
    net = pkg.ConvLSTM(10, [8], [3], 1, out_channels=2, compute_dtype="f32", lon_cyclic=True, feedback=True).cuda()
    net.load_state_dict(OR.synth_params(10, [8], [3], 1, out_channels=2, seed=5))
    return ds, net, np.linspace(-80, 80, 12)


def _hold(spec, x, y, tw, row_w, M, what):
    """spec (HORIZON, 5, O, K) against the exact values of the members x (starts, M, HORIZON, O, Hc, Wc) and targets y"""
    S, _, Hz, O, Hc, Wc = x.shape
    K = Wc // 2 + 1
    g = SP.gamma(SP.n_ops(Wc, M, Hc, S))
    worst = 0.0
    for j in range(Hz):
        val, mag = SP.exact_planes(x[:, :, j], y[:, j], tw, row_w, data_bits=160)
        for idx in np.ndindex(SP.PLANES, O, K):
            exact, bound = sum(val[(n,) + idx] for n in range(S)), g * sum(mag[(n,) + idx] for n in range(S))
            v = spec[(j,) + idx]
            assert np.isfinite(v) and abs(Fraction(float(v)) - exact) <= bound, f"{what} spec{(j,) + idx}: got {v!r}, exact {float(exact)!r}"
            if bound > 0:
                worst = max(worst, float(abs(Fraction(float(v)) - exact) / bound))
    print(f"  {what}: largest |error| / bound {worst:.3e}")


def test_rollouts_fill_the_accumulator_and_leave_their_own_sums_alone():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.dataset import SlabBatch
    from nasa_niswan_amd.engine import InputNoise
    from nasa_niswan_amd.inference import (LEAD_SPECTRUM_COLUMNS, SpectrumAccumulator, _step_targets, lead_time_spectrum, rollout_ensemble,
                                           rollout_skill)
    pkg.load_library()
    ds, net, lat = _stack(pkg)
    Hc, Wc = ds.grid
    O, T, S = 2, SPINUP + HORIZON, len(STARTS)
    row_w = np.cos(np.deg2rad(lat))
    kw = dict(ic_noise=0.05, feedback_noise=0.02, seed=SEED, batch_size=8, lat=lat)
    # ---- the ensemble
    acc = SpectrumAccumulator(O, Hc, Wc, M=M_ENS, nslots=HORIZON, lat=lat)
    with_spec = rollout_ensemble(net, ds, STARTS, HORIZON, SPINUP, M_ENS, spectrum=acc, **kw)
    without = rollout_ensemble(net, ds, STARTS, HORIZON, SPINUP, M_ENS, **kw)
    for a, b, name in zip(with_spec.sums(), without.sums(), ("pix", "counts", "sample", "rank_hist")):
        SM.check_equal(a, b, f"rollout_ensemble with a spectrum: {name}")
    spec, counts = acc.sums()
    assert list(counts) == [S] * HORIZON and spec.shape == (HORIZON, 5, O, Wc // 2 + 1)
    eng = net._engine(torch.device("cuda", torch.cuda.current_device()))
    y = host(_step_targets(ds, ds._device_arrays(), STARTS, T)[:, SPINUP:])      # (S, HORIZON, O, Hc, Wc)
    with torch.no_grad():
        with eng.window(S * M_ENS, T, Hc, Wc, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, SlabBatch(ds, np.asarray([t for t in STARTS for _ in range(M_ENS)]), T),
                        feedback=(net.conv.weight, net.conv.bias, SPINUP), noise=InputNoise(0.05, seed=SEED, draw=0, lane0=0),
                        feedback_noise=InputNoise(0.02, seed=SEED, draw=1, lane0=0))
            seq = host(eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(S, M_ENS, T, O, Hc, Wc))
    assert not np.array_equal(seq[:, 0], seq[:, 1])                             # the members differ
    _hold(spec, seq[:, :, SPINUP:], y, acc.tw_host, row_w, M_ENS, "rollout_ensemble")
    table = lead_time_spectrum(acc)
    assert table.shape == (HORIZON, len(LEAD_SPECTRUM_COLUMNS)) and np.isfinite(table).all()
    rep = acc.report(slots=[0])
    assert rep.count == S and (rep.power_mean <= rep.power_member * (1 + 1e-12)).all()
    # ---- the deterministic roll-out, M = 1
    acc1 = SpectrumAccumulator(O, Hc, Wc, M=1, nslots=HORIZON, lat=lat)
    a = rollout_skill(net, ds, STARTS, HORIZON, SPINUP, 8, lat=lat, spectrum=acc1)
    b = rollout_skill(net, ds, STARTS, HORIZON, SPINUP, 8, lat=lat)
    for u, v, name in zip(a.sums(), b.sums(), ("pix", "counts", "sample")):
        SM.check_equal(u, v, f"rollout_skill with a spectrum: {name}")
    with torch.no_grad():
        with eng.window(S, T, Hc, Wc, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, SlabBatch(ds, np.asarray(STARTS), T), feedback=(net.conv.weight, net.conv.bias, SPINUP))
            seq1 = host(eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(S, 1, T, O, Hc, Wc))
    spec1, counts1 = acc1.sums()
    assert list(counts1) == [S] * HORIZON
    _hold(spec1, seq1[:, :, SPINUP:], y, acc1.tw_host, row_w, 1, "rollout_skill")
    rep1 = acc1.report()
    np.testing.assert_allclose(rep1.power_member, rep1.power_mean, rtol=1e-12)    # one member is its own mean
    # a mismatch is refused
    with pytest.raises(ValueError, match="spectrum must be"):
        rollout_skill(net, ds, STARTS, HORIZON, SPINUP, 8, lat=lat, spectrum=acc)


def test_train_py_test_spectrum_end_to_end(tmp_path, monkeypatch, capsys):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from nasa_niswan_amd import train as T
    from nasa_niswan_amd.inference import LEAD_SPECTRUM_COLUMNS
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    snap = tmp_path / "s"
    argv = ["--model", "LSTM-sp", "--in-channels", "5", "--hidden-channels", "8", "--kernel-size", "3", "--num-layers", "1",
            "--sequence-length", "4", "--input-size", "12", "16", "--grid", "12", "16", "--batch-size", "2", "--num-epochs", "1",
            "--learning-rate", "1e-4", "--synthetic-steps", "60", "--dtype", "f32", "--snapshot-dir", str(snap),
            "--cyclic-longitude", "--tracer-input", "--test-rollout", "3", "--test-spectrum"]
    logger = T.main(T.get_arguments(argv))
    out = capsys.readouterr().out
    assert "Zonal spectra of the rollout" in out
    table = logger["rollout_spectrum"]["rollout"]
    assert table.shape == (3, len(LEAD_SPECTRUM_COLUMNS)) and np.isfinite(table).all()
    z = np.load(snap / "rollout_spectrum.npz")
    K = 16 // 2 + 1
    assert list(z["columns"]) == list(LEAD_SPECTRUM_COLUMNS)
    assert z["rollout_spec"].shape == (3, 5, 1, K) and z["rollout_counts"].shape == (3,) and (z["rollout_counts"] > 0).all()
    assert int(z["rollout_members"]) == 1 and np.array_equal(z["rollout_table"], table)
    for k in ("power_target", "power_member", "power_mean", "power_error", "ratio_member", "ratio_mean", "coherence"):
        assert z[f"rollout_{k}"].shape == (1, K) and np.isfinite(z[f"rollout_{k}"]).all(), k
