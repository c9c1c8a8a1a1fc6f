"""CPU: the ensemble statistics and the stochastic feedback at the boundary -- the numpy model against brute
force, inference.ensemble_from_sums against the definitions, the entries declared / exported / bound, every refusal of
include/nint.h before any HIP call (made-up aligned addresses), and the host layers' refusals without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ensemble_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_ALIGN = -1, -4
A = 4096          # a made-up aligned address: every call below is refused before it is read


# ------------------------------------------------------------------ the model against brute force
def test_identical_members_have_no_spread_and_crps_is_the_absolute_error():
    rng = np.random.default_rng(1)
    for M in (2, 3, 8):
        one = rng.standard_normal((3, 1, 2, 4, 5)).astype(np.float32)
        x, t = np.repeat(one, M, axis=1), rng.standard_normal((3, 2, 4, 5)).astype(np.float32)
        c = EM.cells(x, t)
        assert (c["V"] == 0).all() and (c["D"] == 0).all()
        err = np.abs(one[:, 0].astype(np.float64) - t)
        np.testing.assert_allclose(c["A"] / M - c["D"] / (M * (M - 1)), err, rtol=1e-15)
        np.testing.assert_allclose(c["A"] / M - c["D"] / (M * M), err, rtol=1e-15)


def test_fair_crps_of_two_members_and_the_exact_values():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 2, 1, 3, 3)).astype(np.float32)
    t = rng.standard_normal((5, 1, 3, 3)).astype(np.float32)
    c = EM.cells(x, t)
    a, b, tt = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64), t.astype(np.float64)
    np.testing.assert_allclose(c["A"] / 2 - c["D"] / 2, (np.abs(a - tt) + np.abs(b - tt)) / 2 - np.abs(a - b) / 2, rtol=1e-14, atol=1e-16)
    # the f64 model against the exact (fractions) values, within the bound the GPU test applies to the kernel
    for n in range(5):
        vals, mags, rnd = EM.exact_cell(x[n, :, 0, 1, 2], t[n, 0, 1, 2])
        got = [c["E"][n, 0, 1, 2] ** 2, c["V"][n, 0, 1, 2], c["A"][n, 0, 1, 2], c["D"][n, 0, 1, 2], c["E"][n, 0, 1, 2], tt[n, 0, 1, 2],
               tt[n, 0, 1, 2] ** 2]
        for g, v, m, r in zip(got, vals, mags, rnd):
            assert abs(EM.Fraction(float(g)) - v) <= EM.gamma(r) * m


def test_histogram_totals_and_ties_go_low():
    rng = np.random.default_rng(3)
    N, M, O, Hc, Wc = 4, 5, 2, 3, 7
    _, x, y = EM.int_data(rng, N, M, O, Hc, Wc, 0, 0, Hc, Wc)
    slots = [1, -1, 0, 1]
    r = EM.sums(x, y, slots, 3, None, np.zeros((3, EM.PIX, O, Hc, Wc)), np.zeros((3, O, M + 2), np.int64))
    assert (r["rank_hist"].sum(axis=2) == np.array([[1], [2], [0]]) * Hc * Wc).all()
    # brute force, cell by cell: strictly-below counts, so a tie with every member is rank 0
    rk = EM.cells(x, y)["rank"]
    for n, o, cy, cx in ((0, 0, 0, 0), (1, 1, 0, 1), (2, 0, 0, 2), (3, 1, 1, 1), (0, 1, 2, 3)):
        assert rk[n, o, cy, cx] == sum(float(v) < float(y[n, o, cy, cx]) for v in x[n, :, o, cy, cx])
    assert (rk[:, :, 0, 1] == 0).all() and (rk[:, :, 0, 2] == M).all()
    same = np.repeat(y[:, None], M, axis=1)
    assert (EM.cells(same, y)["rank"] == 0).all()
    # a NaN target or member: bin M + 1
    x2, y2 = x.copy(), y.copy()
    x2[0, 3, 1, 2, 2], y2[2, 0, 1, 4] = np.nan, np.nan
    rk2 = EM.cells(x2, y2)["rank"]
    assert rk2[0, 1, 2, 2] == M + 1 and rk2[2, 0, 1, 4] == M + 1 and (rk2 == M + 1).sum() == 2


def test_ensemble_from_sums_against_the_definitions():
    from nasa_niswan_amd.inference import ensemble_from_sums
    rng = np.random.default_rng(4)
    N, M, O, Hc, Wc = 6, 5, 2, 3, 4
    x = rng.standard_normal((N, M, O, Hc, Wc)).astype(np.float32)
    t = (0.5 * rng.standard_normal((N, O, Hc, Wc)) + 0.2).astype(np.float32)
    slots = [0, 1, 0, 1, 1, 0]
    row_w = np.cos(np.deg2rad(np.linspace(-60, 60, Hc)))
    r = EM.sums(x, t, slots, 2, row_w, np.zeros((2, EM.PIX, O, Hc, Wc)), np.zeros((2, O, M + 2), np.int64))
    counts = np.array([3.0, 3.0])
    for sel in (None, [0], [1]):
        pick = [n for n in range(N) if sel is None or slots[n] in sel]
        rep = ensemble_from_sums(r["pix"], counts, r["sample"], r["rank_hist"], M, row_w, y_std=2.5, slots=sel, sample_slots=slots)
        xs = x[pick].transpose(0, 2, 3, 4, 1).reshape(-1, M)
        want = EM.brute_stats(xs, t[pick].reshape(-1))
        for k, v in want.items():
            assert abs(getattr(rep, k) - v) <= 1e-12 * max(1.0, abs(v)), (sel, k, getattr(rep, k), v)
        assert rep.count == len(pick) and rep.members == M and rep.rank_hist.sum() == len(pick) * O * Hc * Wc
        assert abs(rep.rmse_mean_phys - 2.5 * want["rmse_mean"]) <= 1e-12 and abs(rep.crps_fair_phys - 2.5 * want["crps_fair"]) <= 1e-12
        # a map cell and a cos-latitude row, by brute force
        cell = EM.brute_stats(x[pick][:, :, 1, 2, 3], t[pick][:, 1, 2, 3])
        assert abs(rep.spread_map[1, 2, 3] - cell["spread"]) <= 1e-12 and abs(rep.crps_fair_map[1, 2, 3] - cell["crps_fair"]) <= 1e-12
        assert abs(rep.rmse_mean_map[1, 2, 3] - cell["rmse_mean"]) <= 1e-12
        n0 = pick[0]
        mean = x[n0].astype(np.float64).mean(axis=0)
        wm = (row_w[None, :, None] * (mean - t[n0]) ** 2).sum(axis=(1, 2)) / (Wc * row_w.sum())
        np.testing.assert_allclose(rep.coslat_mse_mean[0], wm, rtol=1e-12)
        assert rep.coslat_crps_fair.shape == (len(pick), O)
    with pytest.raises(ValueError, match="members"):
        ensemble_from_sums(r["pix"], counts, r["sample"], r["rank_hist"], 1)


# ------------------------------------------------------------------ the boundary
def test_entries_are_declared_exported_and_bound():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nint.h")).read(), flags=re.S)
    for name, nargs in (("nint_ens_scratch_bytes", 5), ("nint_ens_accum", 23), ("nint_head_feedback_noise", 22),
                        ("nint_seq_fwd_stochastic", 6)):
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", src), name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)
        assert len(m.split(",")) == nargs
    assert "ensemble.hip" in open(os.path.join(ROOT, "nasa-niswan_amd", "build.py")).read()
    assert (_lib.NINT_ENS_PIX, _lib.NINT_ENS_SAMPLE, _lib.NINT_ENS_MAX_N, _lib.NINT_ENS_MAX_M) == (7, 8, 64, 64)
    for macro, v in (("NINT_ENS_MAX_M", 64), ("NINT_ENS_MAX_N", 64), ("NINT_ENS_PIX", 7), ("NINT_ENS_SAMPLE", 8)):
        assert re.search(rf"#define\s+{macro}\s+{v}\b", src), macro
    # the structure beside nint_feedback: a pointer and four 32-bit words
    assert C.sizeof(_lib.NintFeedbackNoise) == 24 and _lib.NintFeedbackNoise.seed.offset == 8 and _lib.NintFeedbackNoise.lane0.offset == 20
    assert re.search(r"typedef struct nint_feedback_noise \{\s*const float\* sigma;\s*uint32_t seed, draw, step0, lane0;\s*\} nint_feedback_noise;", src)


def test_scratch_query_is_host_arithmetic():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    assert lib.nint_ens_scratch_bytes(3, 8, 5, 13, 37) == 3 * 5 * 2 * 4 * 8 * 8
    assert lib.nint_ens_scratch_bytes(70, 2, 1, 3, 5) == 64 * 1 * 1 * 4 * 8 * 8
    assert lib.nint_ens_scratch_bytes(0, 2, 1, 3, 5) == 0 and lib.nint_ens_scratch_bytes(3, 8, 5, 0, 37) == 0


def test_ens_accum_refusals_without_touching_the_gpu():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    N = 3

    def call(pred=A, off=(0, 100, 50), stride=1000, M=4, y=A, slot=(0, -1, 1), nslots=2, row_w=A, pix=A, sample=A, hist=A, mean=A,
             scratch=A, nb=None, N=N, O=5, H=17, W=41, oy=2, ox=3, Hc=13, Wc=37):
        offs = None if off is None else (C.c_int64 * len(off))(*off)
        sl = None if slot is None else (C.c_int32 * len(slot))(*slot)
        nb = lib.nint_ens_scratch_bytes(N, M, O, Hc, Wc) if nb is None else nb
        return lib.nint_ens_accum(pred, offs, stride, M, y, sl, nslots, row_w, pix, sample, hist, mean, scratch, nb, N, O, H, W, oy,
                                  ox, Hc, Wc, None)

    for kw in (dict(pred=None), dict(off=None), dict(y=None), dict(pix=None), dict(sample=None), dict(hist=None), dict(scratch=None)):
        assert call(**kw) == E_ARG, kw
    for kw in (dict(M=1), dict(M=0), dict(M=65), dict(N=0), dict(O=0), dict(off=(0, -1, 5)), dict(stride=-1), dict(nslots=0),
               dict(slot=(0, 2, 1)), dict(slot=(0, -2, 1)), dict(oy=5), dict(ox=5), dict(oy=-1), dict(Hc=0), dict(Wc=0), dict(Hc=18, oy=0),
               dict(nb=8)):
        assert call(**kw) == E_ARG, kw
    assert call(nb=lib.nint_ens_scratch_bytes(N, 4, 5, 13, 37) - 8) == E_ARG
    # alignment, after every argument check: f64 / int64 buffers 8 bytes, f32 buffers 4
    for kw in (dict(pix=A + 4), dict(sample=A + 4), dict(hist=A + 4), dict(scratch=A + 4), dict(row_w=A + 4), dict(pred=A + 2), dict(y=A + 2),
               dict(mean=A + 2)):
        assert call(**kw) == E_ALIGN, kw
    assert call(pix=A + 4, M=1) == E_ARG
    # optional pointers may be NULL: the call then gets as far as the launch, which this machine cannot do -- so only the
    # refusals are exercised here


def _seq_struct(_lib):
    """a window that passes pass_check's step 1 and whose first gate launch would stop at an alignment check"""
    seq = _lib.NintSeq()
    seq.L, seq.B, seq.T, seq.dtype, seq.xs, seq.h[0], seq.c[0] = 1, 1, 2, 1, 8, 16, 16
    seq.layer[0].k, seq.layer[0].Cx = 1, 4
    return seq


def test_stochastic_entries_refuse_before_any_hip_call():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 13, 37, 2) == 0
    fn = _lib.NintFeedbackNoise()
    fn.sigma, fn.seed, fn.draw, fn.step0, fn.lane0 = A, 1, 2, 3, 4

    def head(h=A, n0=0, N=2, Ch=8, Chp=32, O=3, w=A, b=A, xs=A, x_n0=2, Cx=8, Cxp=16, c0=5, k=0, cyc=0, base=-1, fed=None, geom=C.byref(g),
             dt=1, noise=C.byref(fn)):
        return lib.nint_head_feedback_noise(h, n0, N, Ch, Chp, O, w, b, xs, x_n0, Cx, Cxp, c0, k, cyc, base, fed, geom, dt, None, noise, 7)

    # nint_head_feedback_res's refusals, unchanged, with and without the noise
    for noise in (C.byref(fn), None):
        for kw in (dict(h=None), dict(w=None), dict(xs=None), dict(N=0), dict(O=0), dict(c0=6), dict(k=2), dict(cyc=2), dict(dt=2),
                   dict(geom=None), dict(Chp=24), dict(base=1)):
            assert head(noise=noise, **kw) == E_ARG, kw
        assert head(noise=noise, xs=A + 8) == E_ALIGN
    bad = _lib.NintFeedbackNoise()
    bad.sigma = A + 2
    assert head(noise=C.byref(bad)) == E_ALIGN                           # the noise's own check: sigma 4-byte aligned
    assert head(noise=C.byref(bad), c0=6) == E_ARG                       # ... after the launch's
    # the pass
    seq = _seq_struct(_lib)
    fb = _lib.NintFeedback()
    fb.w, fb.b, fb.O, fb.from_step = A, A, 2, 1
    assert lib.nint_seq_fwd_stochastic(None, C.byref(fb), None, 0, C.byref(fn), None) == E_ARG
    assert lib.nint_seq_fwd_stochastic(C.byref(seq), C.byref(fb), None, 2, C.byref(fn), None) == E_ARG          # residual: 0 or 1
    assert lib.nint_seq_fwd_stochastic(C.byref(seq), C.byref(fb), None, -1, C.byref(fn), None) == E_ARG
    fb.O = 5
    assert lib.nint_seq_fwd_stochastic(C.byref(seq), C.byref(fb), None, 0, C.byref(fn), None) == E_ARG          # more outputs than input channels
    fb.O, fb.from_step = 2, 0
    assert lib.nint_seq_fwd_stochastic(C.byref(seq), C.byref(fb), None, 0, C.byref(fn), None) == E_ARG          # step 0 fed without a state
    fb.from_step = 1
    assert lib.nint_seq_fwd_stochastic(C.byref(seq), C.byref(fb), None, 1, C.byref(fn), None) == \
        lib.nint_seq_fwd_residual(C.byref(seq), C.byref(fb), None, None)                                        # the entry it extends
    # with or without the structure, the pass is refused where nint_seq_fwd_closed refuses it (the first gate's alignment)
    for noise in (None, C.byref(fn), C.byref(_lib.NintFeedbackNoise())):
        assert lib.nint_seq_fwd_stochastic(C.byref(seq), C.byref(fb), None, 0, noise, None) == lib.nint_seq_fwd_closed(C.byref(seq), C.byref(fb), None)
    assert lib.nint_seq_fwd_closed(C.byref(seq), C.byref(fb), None) < 0


# ------------------------------------------------------------------ the host layers, without a device
def test_module_refusals_come_before_any_device():
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.engine import InputNoise
    x = torch.zeros(1, 3, 4, 8, 8)
    plain = pkg.ConvLSTM(4, [8], [3], 1)
    fb = pkg.ConvLSTM(4, [8], [3], 1, out_channels=2, feedback=True)
    with pytest.raises(ValueError, match="feedback=True"):
        plain(x, feedback_noise=InputNoise(0.1))
    with pytest.raises(ValueError, match="InputNoise"):
        fb(x, free_from=1, feedback_noise=0.1)
    with pytest.raises(ValueError, match="channels must be None"):
        fb(x, free_from=1, feedback_noise=InputNoise(0.1, channels=(2, 2)))
    with pytest.raises(ValueError, match="feedback_grad"):
        fb(x, free_from=1, feedback_grad=True, feedback_noise=InputNoise(0.1))
    with pytest.raises(ValueError, match="std values"):
        fb(x, free_from=1, feedback_noise=InputNoise((0.1, 0.2, 0.3)))
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="std"):
            fb(x, free_from=1, feedback_noise=InputNoise(bad))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU path"):          # a valid request gets as far as the device check
            fb(x, free_from=1, feedback_noise=InputNoise((0.1, 0.0)))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fb(x, free_mask=torch.tensor([[0, 1, 1]], dtype=torch.uint8), feedback_noise=InputNoise(0.1, seed=3, draw=1, step0=2, lane0=5))
        # a call that feeds nothing is the call without the argument: it too gets as far as the device check, no further refusal
        for kw in (dict(), dict(free_mask=torch.zeros(1, 3, dtype=torch.uint8)), dict(free_from=3)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                fb(x, feedback_noise=InputNoise(0.1), **kw)


class _Record:
    """what rollout_ensemble looks at before it asks for a device"""
    tracer_input, levels, grid = True, 1, (8, 8)
    yraw = np.zeros((20, 1, 8, 8))


def test_rollout_ensemble_refusals_come_before_any_device():
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.inference import EnsembleAccumulator, rollout_ensemble
    fb = pkg.ConvLSTM(4, [8], [3], 1, out_channels=1, feedback=True)
    ds = _Record()
    with pytest.raises(ValueError, match="feedback=True"):
        rollout_ensemble(pkg.ConvLSTM(4, [8], [3], 1), ds, [1], 3, 2, 4)
    for kw in (dict(horizon=0), dict(spinup=0)):
        with pytest.raises(ValueError, match="horizon and spinup"):
            rollout_ensemble(fb, ds, [1], **{**dict(horizon=3, spinup=2), **kw}, members=4)
    for m in (1, 65, 0, 2.5, True):
        with pytest.raises(ValueError, match="members"):
            rollout_ensemble(fb, ds, [1], 3, 2, m)
    for starts in ([], [0], [16]):
        with pytest.raises(ValueError, match="every start"):
            rollout_ensemble(fb, ds, starts, 3, 2, 4)
    with pytest.raises(ValueError, match="no spread"):
        rollout_ensemble(fb, ds, [1], 3, 2, 4, ic_noise=0.0, feedback_noise=0.0)
    for kw in (dict(ic_noise=-1.0), dict(feedback_noise=float("nan")), dict(ic_noise=float("inf"))):
        with pytest.raises(ValueError, match="std"):
            rollout_ensemble(fb, ds, [1], 3, 2, 4, **kw)
    with pytest.raises(ValueError, match="seed"):
        rollout_ensemble(fb, ds, [1], 3, 2, 4, seed=-1)
    wide = pkg.ConvLSTM(4, [8], [3], 1, out_channels=2, feedback=True)
    with pytest.raises(ValueError, match="levels"):
        rollout_ensemble(wide, ds, [1], 3, 2, 4)
    for m in (1, 65):
        with pytest.raises(ValueError, match="members"):
            EnsembleAccumulator(1, 8, 8, m)
    with pytest.raises(ValueError, match="nslots"):
        EnsembleAccumulator(1, 8, 8, 4, nslots=0)


def _train_args(*extra):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nint_train_cli", os.path.join(ROOT, "nasa-niswan_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.get_arguments(list(extra))


def test_train_cli_flags(capsys, tmp_path):
    base = ["--input-size", "20", "28", "--grid", "20", "28", "--snapshot-dir", str(tmp_path), "--tracer-input"]
    a = _train_args(*base, "--test-rollout", "5", "--ensemble-members", "8", "--ensemble-feedback-noise", "0.02", "--ensemble-seed", "3")
    assert (a.ensemble_members, a.ensemble_noise, a.ensemble_feedback_noise, a.ensemble_seed) == (8, 0.05, 0.02, 3)
    a = _train_args(*base, "--test-rollout", "5")
    assert a.ensemble_members is None
    for extra, msg in ((["--ensemble-members", "8"], "needs --test-rollout"), (["--ensemble-noise", "0.1"], "needs --test-rollout"),
                       (["--test-rollout", "5", "--ensemble-seed", "1"], "needs --ensemble-members"),
                       (["--test-rollout", "5", "--ensemble-members", "1"], "[2, 64]"),
                       (["--test-rollout", "5", "--ensemble-members", "65"], "[2, 64]"),
                       (["--test-rollout", "5", "--ensemble-members", "4", "--ensemble-noise", "-1"], "finite standard deviation"),
                       (["--test-rollout", "5", "--ensemble-members", "4", "--ensemble-feedback-noise", "nan"], "finite standard deviation"),
                       (["--test-rollout", "5", "--ensemble-members", "4", "--ensemble-noise", "0"], "no spread"),
                       (["--test-rollout", "5", "--ensemble-members", "4", "--ensemble-seed", "-2"], "ensemble-seed")):
        with pytest.raises(SystemExit):
            _train_args(*base, *extra)
        assert msg in capsys.readouterr().err, extra
