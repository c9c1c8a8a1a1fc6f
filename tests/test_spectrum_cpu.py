"""CPU: the zonal power spectra at the boundary -- nint_spec_twiddles against numpy.longdouble, the model of
tests/spectrum_model.py against numpy's rfft, inference.spectrum_from_sums against the definitions, the entries declared /
exported / bound, every refusal of include/nint.h before any HIP call (made-up aligned addresses), and the host layers' and
train.py's refusals without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spectrum_model as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4
A = 4096          # a made-up aligned address: every call below is refused before it is read
WIDTHS = (2, 3, 4, 7, 8, 12, 144, 288, 512)


def twiddles(Wc):
    from nasa_niswan_amd import _lib
    tw = np.full((Wc, 2), np.nan)
    assert _lib.load().nint_spec_twiddles(Wc, tw.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return tw


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("Wc", WIDTHS)
def test_twiddles_within_one_ulp_exact_at_quarter_turns_and_conjugate_symmetric(Wc):
    tw = twiddles(Wc)
    ref, exact = SP.reference_twiddles(Wc)
    assert np.isfinite(tw).all() and not np.signbit(tw[tw == 0]).any()          # no negative zero
    # whole quarter turns: exactly 0 and +-1
    assert np.array_equal(tw[exact], ref[exact].astype(np.float64)) and exact[0].all() and (tw[0] == (1.0, 0.0)).all()
    if Wc % 4 == 0:
        assert (tw[Wc // 4] == (0.0, -1.0)).all() and (tw[Wc // 2] == (-1.0, 0.0)).all() and (tw[3 * Wc // 4] == (0.0, 1.0)).all()
    # elsewhere: within 1 ulp of f64 of the longdouble value (whose own error is 2^-11 of that)
    err = np.abs(tw.astype(np.longdouble) - ref)
    assert (tw[~exact] != 0).all() and (err[~exact] <= np.spacing(np.abs(tw[~exact]))).all()
    # tw[Wc - j] = conj(tw[j]) bit for bit (equal f64 values without a negative zero have equal bits)
    back = (-np.arange(Wc)) % Wc
    assert np.array_equal(tw[back, 0], tw[:, 0]) and np.array_equal(tw[back, 1], -tw[:, 1] + 0.0)
    assert tw[back].tobytes() == np.stack([tw[:, 0], -tw[:, 1] + 0.0], axis=1).tobytes()


def test_twiddles_refusals():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 8)()
    assert lib.nint_spec_twiddles(4, None) == E_ARG and lib.nint_spec_twiddles(1, buf) == E_ARG and lib.nint_spec_twiddles(0, buf) == E_ARG
    assert lib.nint_spec_twiddles(513, buf) == E_SHAPE


@pytest.mark.parametrize("Wc", (7, 8, 9, 144, 288))
def test_model_transform_is_numpys_rfft(Wc):
    """F_k with the library's table against np.fft.rfft of the f64 row, to 4 Wc 2^-53 sum |f|: both are sums of Wc products of
    magnitude <= |f[x]| whose factors are within an ulp of the same numbers"""
    rng = np.random.default_rng(Wc)
    f = rng.standard_normal((5, Wc)).astype(np.float32).astype(np.float64)
    re, im = SP.transform(f, twiddles(Wc))
    ref = np.fft.rfft(f, axis=-1)
    assert re.shape == (5, Wc // 2 + 1) == ref.shape
    tol = 4 * Wc * 2.0 ** -53 * np.abs(f).sum(axis=1, keepdims=True)
    assert (np.abs(re - ref.real) <= tol).all() and (np.abs(im - ref.imag) <= tol).all()


def test_exact_planes_agree_with_the_f64_model_within_the_bound():
    rng = np.random.default_rng(12)
    N, M, O, Hc, Wc = 2, 3, 2, 4, 9
    x = rng.standard_normal((N, M, O, Hc, Wc)).astype(np.float32)
    t = rng.standard_normal((N, O, Hc, Wc)).astype(np.float32)
    tw, row_w = twiddles(Wc), 0.25 + rng.random(Hc)
    got = SP.planes(x, t, tw, row_w)
    val, mag = SP.exact_planes(x, t, tw, row_w)
    g = SP.gamma(SP.n_ops(Wc, M, Hc, 0))
    for idx in np.ndindex(got.shape):
        assert abs(SP.Fraction(float(got[idx])) - val[idx]) <= g * mag[idx], idx
    assert (mag >= abs(val)).all()
    # integers: the model is exact
    tb = SP.int_table(rng, Wc)
    _, xi, yi = SP.int_data(rng, N, M, O, Hc, Wc, 0, 0, Hc, Wc)
    vi, _ = SP.exact_planes(xi, yi, tb, SP.dyadic_rows(Hc))
    gi = SP.planes(xi, yi, tb, SP.dyadic_rows(Hc))
    assert all(SP.Fraction(float(gi[idx])) == vi[idx] for idx in np.ndindex(gi.shape))
    assert SP.int_magnitude_bound(144, 5, 8, 5) < 2 ** 50


# ------------------------------------------------------------------ spectrum_from_sums
def _sums_of(x, t, row_w, slots, nslots):
    Wc = x.shape[-1]
    spec = SP.sums(x, t, twiddles(Wc), slots, nslots, row_w, np.zeros((nslots, SP.PLANES, x.shape[2], Wc // 2 + 1)))
    counts = np.array([sum(1 for s in slots if s == j) for j in range(nslots)], np.float64)
    return spec, counts


@pytest.mark.parametrize("Wc", (9, 12))
def test_parseval_and_the_derived_figures(Wc):
    from nasa_niswan_amd.inference import spectrum_from_sums
    rng = np.random.default_rng(20 + Wc)
    N, M, O, Hc = 5, 3, 2, 4
    x = rng.standard_normal((N, M, O, Hc, Wc)).astype(np.float32)
    t = rng.standard_normal((N, O, Hc, Wc)).astype(np.float32)
    row_w = np.cos(np.deg2rad(np.linspace(-60, 60, Hc)))
    slots = [0, 1, 0, 2, 0]
    spec, counts = _sums_of(x, t, row_w, slots, 4)                                  # slot 3 stays empty
    w = row_w[None, None, :, None]
    for sel in (None, [0], [1, 2]):
        pick = [n for n in range(N) if sel is None or slots[n] in sel]
        rep = spectrum_from_sums(spec, counts, M, Wc, row_w.sum(), sel)
        assert rep.count == len(pick) and rep.members == M and rep.width == Wc and rep.power_target.shape == (O, Wc // 2 + 1)
        xs, ts = x[pick].astype(np.float64), t[pick].astype(np.float64)
        mean = xs.mean(axis=1)

        def wms(f):                                                                # the weighted mean square per output
            return (w * f * f).sum(axis=(0, 2, 3)) / (len(pick) * Wc * row_w.sum())

        np.testing.assert_allclose(rep.power_target.sum(axis=1), wms(ts), rtol=1e-12)
        np.testing.assert_allclose(rep.power_mean.sum(axis=1), wms(mean), rtol=1e-12)
        np.testing.assert_allclose(rep.power_error.sum(axis=1), wms(mean - ts), rtol=1e-12)
        np.testing.assert_allclose(rep.power_member.sum(axis=1), np.mean([wms(xs[:, i]) for i in range(M)], axis=0), rtol=1e-12)
        np.testing.assert_allclose(rep.ratio_member, rep.power_member / rep.power_target, rtol=1e-15)
        np.testing.assert_allclose(rep.ratio_mean, rep.power_mean / rep.power_target, rtol=1e-15)
        assert (rep.coherence >= 0).all() and (rep.coherence <= 1 + 1e-12).all()
        assert (rep.power_mean <= rep.power_member * (1 + 1e-12)).all()            # the mean is smoother than its members
    # an empty slot: nan
    rep = spectrum_from_sums(spec, counts, M, Wc, row_w.sum(), [3])
    assert rep.count == 0 and all(np.isnan(getattr(rep, k)).all() for k in ("power_target", "power_member", "power_mean", "power_error",
                                                                             "ratio_member", "ratio_mean", "coherence"))
    with pytest.raises(ValueError, match="members"):
        spectrum_from_sums(spec, counts, 0, Wc, 1.0)
    with pytest.raises(ValueError, match="spec must be"):
        spectrum_from_sums(spec[:, :4], counts, M, Wc, 1.0)
    with pytest.raises(ValueError, match="spec must be"):
        spectrum_from_sums(spec, counts, M, Wc + 2, 1.0)


def test_identical_members_a_perfect_prediction_and_a_single_wave():
    from nasa_niswan_amd.inference import LEAD_SPECTRUM_COLUMNS, lead_spectrum_from_sums, spectrum_from_sums
    rng = np.random.default_rng(31)
    N, M, O, Hc, Wc = 3, 4, 2, 3, 16
    K = Wc // 2 + 1
    t = rng.standard_normal((N, O, Hc, Wc)).astype(np.float32)
    one = rng.standard_normal((N, 1, O, Hc, Wc)).astype(np.float32)
    # identical members: the mean is each member
    spec, counts = _sums_of(np.repeat(one, M, axis=1), t, None, [0] * N, 1)
    rep = spectrum_from_sums(spec, counts, M, Wc, Hc)
    np.testing.assert_allclose(rep.power_member, rep.power_mean, rtol=1e-13)
    np.testing.assert_allclose(rep.ratio_member, rep.ratio_mean, rtol=1e-13)
    # pred == y: coherence 1, no error power
    spec, counts = _sums_of(np.repeat(t[:, None], M, axis=1), t, None, [0] * N, 1)
    rep = spectrum_from_sums(spec, counts, M, Wc, Hc)
    np.testing.assert_allclose(rep.coherence, 1.0, rtol=1e-12)
    assert (np.abs(rep.power_error) <= 1e-12 * rep.power_target).all()
    np.testing.assert_allclose(rep.ratio_mean, 1.0, rtol=1e-12)
    table = lead_spectrum_from_sums(spec, counts, M, Wc)
    assert table.shape == (1, len(LEAD_SPECTRUM_COLUMNS)) and abs(table[0, 0] - 1) <= 1e-12 and abs(table[0, 1] - 1) <= 1e-12
    assert table[0, 2] == K                                                       # coherent at every wavenumber
    # a single wave k0 as the target: its spectrum is zero elsewhere
    k0 = 3
    wave = np.cos(2 * np.pi * k0 * np.arange(Wc) / Wc + 0.4).astype(np.float32)
    tk = np.broadcast_to(wave, (N, O, Hc, Wc)).copy()
    spec, counts = _sums_of(np.repeat(one, M, axis=1), tk, None, [0, 1, 0], 3)
    rep = spectrum_from_sums(spec, counts, M, Wc, Hc, [0, 1])
    off = np.arange(K) != k0
    assert (rep.power_target[:, off] <= 1e-13).all()
    np.testing.assert_allclose(rep.power_target[:, k0], 0.5, rtol=1e-6)             # the mean square of a cosine (f32 samples)
    # the lead-time table: an empty slot is nan, the others are finite; kmin is checked
    table = lead_spectrum_from_sums(spec, counts, M, Wc)
    assert np.isfinite(table[:2]).all() and np.isnan(table[2]).all()
    uncorrelated = lead_spectrum_from_sums(*_sums_of(np.repeat(one, M, axis=1), t, None, [0] * N, 1), M, Wc)
    assert 0 <= uncorrelated[0, 2] < K and 0 < uncorrelated[0, 3] <= 1
    for bad in (-1, K):
        with pytest.raises(ValueError, match="kmin"):
            lead_spectrum_from_sums(spec, counts, M, Wc, kmin=bad)


# ------------------------------------------------------------------ the boundary
def test_entries_are_declared_exported_and_bound():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nint.h")).read(), flags=re.S)
    for name, nargs in (("nint_spec_scratch_bytes", 5), ("nint_spec_twiddles", 2), ("nint_spec_accum", 21)):
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", src), name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
        assert len(re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1).split(",")) == nargs
    assert "spectrum.hip" in open(os.path.join(ROOT, "nasa-niswan_amd", "build.py")).read()
    assert (_lib.NINT_SPEC_PLANES, _lib.NINT_SPEC_MAX_W, _lib.NINT_SPEC_MAX_N) == (5, 512, 64)
    for macro, v in (("NINT_SPEC_PLANES", 5), ("NINT_SPEC_MAX_W", 512), ("NINT_SPEC_MAX_N", 64)):
        assert re.search(rf"#define\s+{macro}\s+{v}\b", src), macro


def test_scratch_query_is_host_arithmetic():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    assert lib.nint_spec_scratch_bytes(3, 8, 5, 13, 37) == 3 * 5 * 5 * 19 * 8
    assert lib.nint_spec_scratch_bytes(70, 2, 1, 2, 6) == 64 * 1 * 5 * 4 * 8
    assert lib.nint_spec_scratch_bytes(88, 8, 20, 100, 144) == 64 * 20 * 5 * 73 * 8
    assert lib.nint_spec_scratch_bytes(0, 2, 1, 3, 5) == 0 and lib.nint_spec_scratch_bytes(3, 8, 5, 0, 37) == 0
    assert lib.nint_spec_scratch_bytes(3, 8, 5, 4, 1) == 0


def test_spec_accum_refusals_without_touching_the_gpu():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    N = 3

    def call(pred=A, off=(0, 100, 50), stride=1000, M=4, y=A, slot=(0, -1, 1), nslots=2, row_w=A, tw=A, spec=A, scratch=A, nb=None,
             N=N, O=5, H=17, W=41, oy=2, ox=3, Hc=13, Wc=37):
        offs = None if off is None else (C.c_int64 * len(off))(*off)
        sl = None if slot is None else (C.c_int32 * len(slot))(*slot)
        nb = lib.nint_spec_scratch_bytes(N, M, O, Hc, Wc) if nb is None else nb
        return lib.nint_spec_accum(pred, offs, stride, M, y, sl, nslots, row_w, tw, spec, scratch, nb, N, O, H, W, oy, ox, Hc, Wc, None)

    for kw in (dict(pred=None), dict(off=None), dict(y=None), dict(tw=None), dict(spec=None), dict(scratch=None)):
        assert call(**kw) == E_ARG, kw
    for kw in (dict(M=0), dict(M=-1), dict(M=65), dict(N=0), dict(O=0), dict(nslots=0), dict(off=(0, -1, 5)), dict(stride=-1),
               dict(slot=(0, 2, 1)), dict(slot=(0, -2, 1)), dict(oy=5), dict(ox=5), dict(oy=-1), dict(ox=-1), dict(Hc=0),
               dict(Hc=18, oy=0), dict(Wc=1), dict(Wc=0), dict(nb=8)):
        assert call(**kw) == E_ARG, kw
    assert call(nb=lib.nint_spec_scratch_bytes(N, 4, 5, 13, 37) - 8) == E_ARG
    # a crop wider than the kernel holds: NINT_E_SHAPE (with a grid that contains it and a scratch that would do)
    assert call(Wc=513, W=600, nb=1 << 30) == E_SHAPE
    assert call(Wc=513, W=600, nb=1 << 30, M=0) == E_ARG
    # alignment, after every argument check: f64 buffers 8 bytes, f32 buffers 4
    for kw in (dict(spec=A + 4), dict(scratch=A + 4), dict(row_w=A + 4), dict(tw=A + 4), dict(pred=A + 2), dict(y=A + 2)):
        assert call(**kw) == E_ALIGN, kw
    assert call(spec=A + 4, M=0) == E_ARG and call(spec=A + 4, Wc=513, W=600, nb=1 << 30) == E_SHAPE
    # M = 1 is the deterministic roll-out, not a refusal: with a bad alignment the call gets past the argument checks
    assert call(M=1, spec=A + 4) == E_ALIGN


# ------------------------------------------------------------------ the host layers, without a device
class _Record:
    """what the roll-outs look at before they ask for a device"""
    tracer_input, levels, grid = True, 1, (8, 8)
    yraw = np.zeros((20, 1, 8, 8))


class _Shape:
    """a SpectrumAccumulator's shape without its device buffers: what _check_rollout compares"""
    def __init__(self, O, Hc, Wc, M, nslots, halo=None):
        from nasa_niswan_amd.inference import SpectrumAccumulator
        self.O, self.Hc, self.Wc, self.M, self.nslots, self.halo = O, Hc, Wc, M, nslots, halo
        self._check_rollout = SpectrumAccumulator._check_rollout.__get__(self)


def test_accumulator_and_rollout_refusals_come_before_any_device():
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.inference import SpectrumAccumulator, rollout_ensemble, rollout_skill
    for kw, msg in ((dict(M=0), "members"), (dict(M=65), "members"), (dict(nslots=0), "nslots"), (dict(Wc=1), "width"),
                    (dict(Wc=513), "width"), (dict(lat=np.zeros(3)), "latitudes"), (dict(O=0), "O and Hc")):
        with pytest.raises(ValueError, match=msg):
            SpectrumAccumulator(**{**dict(O=1, Hc=8, Wc=8, M=2, nslots=1, device="cuda"), **kw})
    fb = pkg.ConvLSTM(4, [8], [3], 1, out_channels=1, feedback=True)
    ds = _Record()
    # the roll-outs: a spectrum whose shape is not the roll-out's is a ValueError (the net lives on the CPU: no device was asked)
    for bad in (_Shape(2, 8, 8, 1, 3), _Shape(1, 8, 9, 1, 3), _Shape(1, 7, 8, 1, 3), _Shape(1, 8, 8, 2, 3), _Shape(1, 8, 8, 1, 4),
                _Shape(1, 8, 8, 1, 3, halo=(0, 0))):
        with pytest.raises(ValueError, match="spectrum must be"):
            rollout_skill(fb, ds, [1], 3, 2, spectrum=bad)
    for bad in (_Shape(1, 8, 8, 1, 3), _Shape(1, 8, 8, 3, 3), _Shape(1, 8, 8, 4, 2), _Shape(1, 8, 16, 4, 3)):
        with pytest.raises(ValueError, match="spectrum must be"):
            rollout_ensemble(fb, ds, [1], 3, 2, 4, spectrum=bad)
    # the older refusals still come first
    with pytest.raises(ValueError, match="every start"):
        rollout_skill(fb, ds, [16], 3, 2, spectrum=_Shape(2, 8, 8, 1, 3))
    with pytest.raises(ValueError, match="members"):
        rollout_ensemble(fb, ds, [1], 3, 2, 1, spectrum=_Shape(1, 8, 8, 1, 3))


def _train_args(*extra):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nint_train_cli_spectrum", os.path.join(ROOT, "nasa-niswan_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.get_arguments(list(extra))


def test_train_cli_flag(capsys, tmp_path):
    base = ["--input-size", "20", "28", "--grid", "20", "28", "--snapshot-dir", str(tmp_path), "--tracer-input"]
    assert _train_args(*base, "--test-rollout", "5", "--test-spectrum").test_spectrum is True
    assert _train_args(*base, "--test-rollout", "5", "--test-spectrum", "--ensemble-members", "4").test_spectrum is True
    assert _train_args(*base, "--test-rollout", "5").test_spectrum is False
    with pytest.raises(SystemExit):
        _train_args(*base, "--test-spectrum")
    assert "--test-spectrum needs --test-rollout" in capsys.readouterr().err
