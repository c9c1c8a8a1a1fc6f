"""Evaluation skill sums without a GPU: the argument checks of nint_skill_accum / nint_head_skill_accum from the real
library (they run before any HIP call), the scratch-size query, and inference.skill_from_sums against the reference
expressions of the analysis notebook (test.ipynb:377-385, :462-485, :605, :630, :796-803) in f64."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from nasa_niswan_amd import _lib
    return _lib.load()


def test_binding_constants_match_the_header():
    import os
    import re
    from nasa_niswan_amd import _lib, inference
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nint.h")).read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert (val("NINT_SKILL_PIX"), val("NINT_SKILL_SAMPLE"), val("NINT_SKILL_MAX_N")) == \
        (_lib.NINT_SKILL_PIX, _lib.NINT_SKILL_SAMPLE, _lib.NINT_SKILL_MAX_N) == (5, 8, 64)
    assert (inference.NINT_SKILL_PIX, inference.NINT_SKILL_SAMPLE) == (5, 8)
    assert val("NINT_VERSION") == _lib.NINT_VERSION == 113


def test_scratch_bytes_is_positive_and_monotone(lib):
    f = lib.nint_skill_scratch_bytes
    assert f(1, 1, 1, 1) > 0 and f(0, 1, 1, 1) == 0 and f(1, 1, 0, 5) == 0
    for Hc, Wc in ((9, 15), (90, 144), (1, 257)):
        prev = 0
        for N in (1, 2, 5, 63, 64, 65, 70, 1000):
            cur = f(N, 3, Hc, Wc)
            assert cur >= prev > -1 and cur > 0
            prev = cur
        prev = 0
        for O in (1, 2, 3, 4, 5, 20, 200):
            cur = f(8, O, Hc, Wc)
            assert cur > prev
            prev = cur
    assert f(64, 2, 9, 15) == f(70, 2, 9, 15)         # larger calls run in pieces that reuse the scratch
    assert f(8, 20, 90, 144) % 8 == 0


def test_skill_entries_reject_bad_arguments_without_touching_the_gpu(lib):
    """Every return code of the two entries, with dummy pointers: the checks run before any HIP call."""
    from nasa_niswan_amd import _lib
    N, O, H, W, oy, ox, Hc, Wc = 5, 2, 13, 21, 2, 3, 9, 15
    need = lib.nint_skill_scratch_bytes(N, O, Hc, Wc)
    slot = (C.c_int32 * N)(0, 1, -1, 0, 1)
    P, Y, PIX, SMP, SCR = 64, 128, 256, 512, 1024      # dummy, aligned

    def plain(pred=P, y=Y, slot=slot, nslots=2, row_w=None, pix=PIX, sample=SMP, scratch=SCR, sb=need, N=N, O=O, H=H, W=W,
              oy=oy, ox=ox, Hc=Hc, Wc=Wc):
        return lib.nint_skill_accum(pred, y, slot, nslots, row_w, pix, sample, scratch, sb, N, O, H, W, oy, ox, Hc, Wc, None)

    for kw in (dict(pred=None), dict(y=None), dict(pix=None), dict(sample=None), dict(scratch=None), dict(sb=need - 1), dict(sb=0),
               dict(nslots=0), dict(nslots=-3), dict(nslots=1),                       # slot 1 outside [-1, 1)
               dict(slot=(C.c_int32 * N)(0, 1, -2, 0, 1)), dict(slot=(C.c_int32 * N)(0, 2, 0, 0, 0)),
               dict(oy=-1), dict(ox=-1), dict(oy=5), dict(ox=7), dict(Hc=0), dict(Wc=0), dict(N=0), dict(O=0)):
        assert plain(**kw) == E_ARG, kw
    for kw in (dict(pix=PIX + 4), dict(sample=SMP + 4), dict(scratch=SCR + 4), dict(row_w=36), dict(pix=PIX + 1)):
        assert plain(**kw) == E_ALIGN, kw

    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), H, W, 2) == 0
    Wp, Bp, HS = 2048, 4096, 8192

    def fused(h=HS, n0=N, N=N, Ch=16, Chp=16, O=O, w=Wp, b=Bp, y=Y, slot=slot, nslots=2, row_w=None, pix=PIX, sample=SMP,
              pred_out=None, scratch=SCR, sb=need, g=C.byref(g), oy=oy, ox=ox, Hc=Hc, Wc=Wc, dt=0):
        return lib.nint_head_skill_accum(h, n0, N, Ch, Chp, O, w, b, y, slot, nslots, row_w, pix, sample, pred_out, scratch, sb,
                                         g, oy, ox, Hc, Wc, dt, None)

    for kw in (dict(h=None), dict(w=None), dict(g=None), dict(y=None), dict(pix=None), dict(sample=None), dict(scratch=None),
               dict(sb=need - 1), dict(nslots=0), dict(nslots=1), dict(slot=(C.c_int32 * N)(0, 1, -2, 0, 1)),
               dict(slot=(C.c_int32 * N)(2, 0, 0, 0, 0)), dict(oy=-1), dict(oy=5), dict(ox=7), dict(dt=7), dict(dt=-1),
               dict(N=0), dict(O=0), dict(Ch=0), dict(Ch=17)):                        # Chp < Ch
        assert fused(**kw) == E_ARG, kw
    for kw in (dict(Chp=192), dict(Ch=130, Chp=144), dict(Chp=18),                    # beyond nint_head_loss_fused's limits
               dict(O=2000, sb=lib.nint_skill_scratch_bytes(N, 2000, Hc, Wc))):      # [O][CHV] weights beyond the LDS
        assert fused(**kw) == E_SHAPE, kw
    for kw in (dict(pix=PIX + 4), dict(sample=SMP + 4), dict(scratch=SCR + 4), dict(h=HS + 8), dict(row_w=36)):
        assert fused(**kw) == E_ALIGN, kw
    # a NULL slot array means "all 0", a NULL bias "no bias", a NULL pred_out "do not store": not errors -- the first check
    # that fails for them is the next one
    assert fused(slot=None, b=None, pix=PIX + 4) == E_ALIGN and plain(slot=None, pix=PIX + 4) == E_ALIGN


# ------------------------------------------------------------------------------ skill_from_sums vs the notebook
Y_MEAN, Y_STD = 3.2e-9, 1.7e-9


def r_squared_spatial_notebook(real_data, model_output):
    """test.ipynb:480-485, verbatim arithmetic"""
    ss_res = np.sum((real_data - model_output) ** 2, axis=0)
    ss_tot = np.sum((real_data - np.mean(real_data, axis=0)) ** 2, axis=0)
    return 1 - (ss_res / ss_tot)


def sums_np(y, p, slot, nslots, row_w):
    """the f64 sums of the device pass, in numpy: y, p (N, O, Hc, Wc) f32"""
    y, p = y.astype(np.float64), p.astype(np.float64)
    d = p - y
    N, O, Hc, Wc = y.shape
    pix = np.zeros((nslots, 5, O, Hc, Wc))
    counts = np.zeros(nslots)
    for n in range(N):
        if slot[n] >= 0:
            pix[slot[n]] += np.stack([y[n], p[n], y[n] ** 2, p[n] ** 2, d[n] ** 2])
            counts[slot[n]] += 1
    w = np.ones(Hc) if row_w is None else row_w
    s = lambda a: a.sum(axis=(2, 3))
    wv = w[None, None, :, None]
    sample = np.stack([s(d * d), s(np.abs(d)), s(y), s(y * y), s(p), s(p * p), s(wv * y), s(wv * p)], axis=-1)
    return pix, counts, sample


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(5)
    y = rng.standard_normal((11, 2, 9, 15)).astype(np.float32)
    p = (0.8 * y + 0.3 * rng.standard_normal(y.shape)).astype(np.float32)
    y[:, 0, 2, 3] = np.float32(0.75)                      # a constant-target pixel with a wrong prediction ...
    y[:, 1, 4, 5] = np.float32(-0.5)                      # ... and one that is fit exactly
    p[:, 1, 4, 5] = np.float32(-0.5)
    lat = np.linspace(-60.0, 60.0, 9)
    return y, p, lat


def close(a, b, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= rtol * np.abs(b)), float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_skill_from_sums_matches_the_notebook_expressions(case):
    from sklearn.metrics import r2_score
    from nasa_niswan_amd.inference import skill_from_sums
    y, p, lat = case
    N, O, Hc, Wc = y.shape
    w = np.cos(np.deg2rad(lat))
    pix, counts, sample = sums_np(y, p, [0] * N, 1, w)
    rep = skill_from_sums(pix, counts, sample, w, Y_MEAN, Y_STD)
    G = y.astype(np.float64) * Y_STD + Y_MEAN              # de-normalised in f64 (test.ipynb cell 8)
    Pd = p.astype(np.float64) * Y_STD + Y_MEAN
    const = np.zeros((O, Hc, Wc), dtype=bool)
    const[0, 2, 3] = const[1, 4, 5] = True
    # R2 per grid cell: sklearn per pixel everywhere, the notebook's vectorised cell wherever it is finite
    r2_sk = np.array([[[r2_score(G[:, o, i, j], Pd[:, o, i, j]) for j in range(Wc)] for i in range(Hc)] for o in range(O)])
    assert np.max(np.abs(rep.r2_spatial - r2_sk)[~const]) <= 1e-12
    # the two constant-target pixels: 11 equal de-normalised f64 values do not average to that value exactly, so in physical
    # units sklearn sees ss_tot ~ 1e-50 instead of 0; in z-score units (0.75 and -0.5: exact sums) it sees the constant target
    # that is meant, and R2 does not depend on the units
    for o, i, j in ((0, 2, 3), (1, 4, 5)):
        assert rep.r2_spatial[o, i, j] == r2_score(y[:, o, i, j].astype(np.float64), p[:, o, i, j].astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r2_nb = np.stack([r_squared_spatial_notebook(G[:, o], Pd[:, o]) for o in range(O)])
    assert np.max(np.abs(rep.r2_spatial - r2_nb)[~const]) <= 1e-12
    # sklearn's constant-target convention, pinned (the notebook's vectorised cell has -inf and nan at these two)
    assert rep.r2_spatial[0, 2, 3] == 0.0 and rep.r2_spatial[1, 4, 5] == 1.0
    # Pearson r per grid cell
    r_ref = np.array([[[np.corrcoef(G[:, o, i, j], Pd[:, o, i, j])[0, 1] if not const[o, i, j] else np.nan
                        for j in range(Wc)] for i in range(Hc)] for o in range(O)])
    assert np.all(np.isnan(rep.pearson[const])) and np.max(np.abs(rep.pearson - r_ref)[~const]) <= 1e-12
    close(rep.mean_gt, G.mean(axis=0)); close(rep.mean_pd, Pd.mean(axis=0))
    close(rep.rmse, np.sqrt(((Pd - G) ** 2).mean(axis=0)))
    bias = (Pd - G).mean(axis=0)
    close(rep.bias[~const], bias[~const])
    assert rep.bias[1, 4, 5] == 0.0
    # per sample
    r2t = np.array([r2_score(G[n].flatten(), Pd[n].flatten()) for n in range(N)])          # test.ipynb:377-385
    assert np.max(np.abs(rep.r2_temporal - r2t)) <= 1e-12
    r2to = np.array([[r2_score(G[n, o].flatten(), Pd[n, o].flatten()) for o in range(O)] for n in range(N)])
    assert np.max(np.abs(rep.r2_temporal_per_output - r2to)) <= 1e-12
    dz = p.astype(np.float64) - y.astype(np.float64)
    close(rep.loss, (dz ** 2).mean(axis=(1, 2, 3)) + np.abs(dz).mean(axis=(1, 2, 3)))
    # cos-latitude weighted mean over (lat, lon) (test.ipynb:796-803: ds.weighted(weights).mean(("lat", "lon")))
    wm = lambda a: (a * w[None, None, :, None]).sum(axis=(2, 3)) / (w.sum() * Wc)
    close(rep.global_mean_gt, wm(G)); close(rep.global_mean_pd, wm(Pd))
    assert abs(rep.r2 - r2_score(G.flatten(), Pd.flatten())) <= 1e-12
    assert rep.count == N
    # uniform weights: the plain mean
    rep1 = skill_from_sums(*sums_np(y, p, [0] * N, 1, None), None, Y_MEAN, Y_STD)
    close(rep1.global_mean_gt, G.mean(axis=(2, 3))); close(rep1.global_mean_pd, Pd.mean(axis=(2, 3)))
    # z-score units by default
    rep0 = skill_from_sums(pix, counts, sample, w)
    close(rep0.mean_gt, y.astype(np.float64).mean(axis=0))
    assert np.array_equal(rep0.r2_spatial, rep.r2_spatial) and set(rep.arrays()) >= {"r2_spatial", "r2_temporal", "global_mean_pd"}


def test_union_of_slots_equals_the_report_of_the_pooled_samples(case):
    from nasa_niswan_amd.inference import skill_from_sums
    y, p, lat = case
    N = y.shape[0]
    w = np.cos(np.deg2rad(lat))
    slot = [0, 1, 2, -1, 0, 1, 2, 0, 1, 2, 0]
    pix, counts, sample = sums_np(y, p, slot, 3, w)
    union = skill_from_sums(pix, counts, sample, w, Y_MEAN, Y_STD, slots=[0, 2])
    keep = [n for n in range(N) if slot[n] in (0, 2)]
    pooled = skill_from_sums(*sums_np(y[keep], p[keep], [0] * len(keep), 1, w), w, Y_MEAN, Y_STD)
    assert union.count == pooled.count == len(keep)
    for name in ("r2_spatial", "rmse", "mean_gt", "mean_pd"):
        a, b = getattr(union, name), getattr(pooled, name)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), name
    ok = ~np.isnan(pooled.pearson)
    assert np.array_equal(ok, ~np.isnan(union.pearson)) and np.max(np.abs(union.pearson - pooled.pearson)[ok]) <= 1e-12
    assert np.max(np.abs(union.bias - pooled.bias)) <= 1e-12 * Y_STD
    # the per-sample series cover every sample, whatever its slot
    assert union.r2_temporal.shape == (N,) and pooled.r2_temporal.shape == (len(keep),)
    assert np.array_equal(union.r2_temporal[keep], pooled.r2_temporal)
    # all slots = every sample that has one
    full = skill_from_sums(pix, counts, sample, w, Y_MEAN, Y_STD)
    assert full.count == N - 1


def test_constant_targets_with_full_mantissa_values_are_recognised():
    """A tracer clamped at zero is the same z-score -- an arbitrary f32 -- in every window of a group.  (sum y)^2 / n then does
    not cancel sum y^2 exactly in f64; the convention must hold all the same, for every such value and group size."""
    from sklearn.metrics import r2_score
    from nasa_niswan_amd.inference import skill_from_sums
    rng = np.random.default_rng(11)
    for n in (2, 3, 7, 21, 64, 1000):
        y = rng.standard_normal((n, 1, 4, 50)).astype(np.float32)
        p = (y + 0.1 * rng.standard_normal(y.shape)).astype(np.float32)
        y[:, 0, 0, :] = ((0.0 - rng.uniform(1, 30, 50)) / rng.uniform(20, 80, 50)).astype(np.float32)[None]   # (0 - mean) / std
        y[:, 0, 1, :] = y[:1, 0, 1, :]
        p[:, 0, 1, :] = y[:, 0, 1, :]                                                                         # ... fit exactly
        rep = skill_from_sums(*sums_np(y, p, [0] * n, 1, None))
        assert np.all(rep.r2_spatial[0, 0] == 0.0) and np.all(rep.r2_spatial[0, 1] == 1.0)
        assert np.all(np.isnan(rep.pearson[0, :2])) and np.all(np.isfinite(rep.pearson[0, 2:]))
        y64, p64 = y.astype(np.float64), p.astype(np.float64)
        ref = np.array([[r2_score(y64[:, 0, i, j], p64[:, 0, i, j]) for j in range(50)] for i in (2, 3)])
        assert np.max(np.abs(rep.r2_spatial[0, 2:] - ref)) <= 1e-12
        if n <= 21:
            # ... and a target that BARELY varies (zero in all windows but one): ss_tot is ~1e-5 of sum y^2 and R2 is -1e3 ... -1e6.
            # A few f32 values and their squares add exactly in f64, so the sums hold the answer, and the report has to get it out
            # of them to the precision of a double of that size (which is also all the reference expression has)
            y2, p2 = y.copy(), p.copy()
            y2[:, 0, 0, :] = y[:1, 0, 0, :]
            y2[n // 2, 0, 0, :] += np.float32(3e-3) * rng.uniform(0.5, 2, 50).astype(np.float32)
            rep2 = skill_from_sums(*sums_np(y2, p2, [0] * n, 1, None))
            ref2 = np.array([r2_score(y2[:, 0, 0, j].astype(np.float64), p2[:, 0, 0, j].astype(np.float64)) for j in range(50)])
            assert np.all(ref2 < -100) and np.all(np.abs(rep2.r2_spatial[0, 0] - ref2) <= 1e-12 * np.abs(ref2))
