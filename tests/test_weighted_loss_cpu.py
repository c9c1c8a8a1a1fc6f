"""CPU-only checks of the weighted training loss: the three ``_weighted`` entry points at the boundary (declared, exported,
argument checks before any launch), the host helpers of ``nasa_niswan_amd/loss.py`` and the trainer's validator, and the
f64 host model the GPU tests compare against (tests/weighted_loss_model.py) -- itself checked here against torch CPU
autograd and sklearn's weighted r2_score."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import weighted_loss_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nint_loss_mse_l1_crop_weighted", "nint_head_loss_fused_weighted", "nint_head_loss_seq_fused_weighted")
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


def test_weighted_entry_points_are_declared_exported_and_bound():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nint.h")).read(), flags=re.S)
    for name, twin in zip(NEW, ("nint_loss_mse_l1_crop", "nint_head_loss_fused", "nint_head_loss_seq_fused")):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        tres, targs = _lib.SIGNATURES[twin]
        # the twin's signature with (const float* wgt, double wsum) after y
        iy = 1 if twin == "nint_loss_mse_l1_crop" else 8
        assert res is tres and args == targs[:iy + 1] + [C.c_void_p, C.c_double] + targs[iy + 1:]
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)
        names = [re.split(r"[\s*]+", a.strip())[-1] for a in m.split(",")]
        assert names[iy:iy + 3] == ["y", "wgt", "wsum"] and len(names) == len(args)
    assert lib.nint_version() == 113                                # entry points were added, nothing else moved


def test_weighted_entry_points_reject_bad_weights_without_touching_the_gpu():
    """The checks happen before any HIP call, so fake (non-NULL, aligned) addresses exercise them on a CPU-only machine: with
    every other argument valid, a NULL map and a wsum of 0, -1, nan or inf give E_ARG and a map off a 4-byte boundary
    E_ALIGN; the twins' own checks come first / stay (crop outside the grid, Chp > 128, misaligned loss_out)."""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 12, 20, 1) == 0
    a = 4096                                                         # a 16-byte aligned fake address
    bad_wsum = (0.0, -1.0, float("nan"), float("inf"), -float("inf"))

    def crop(wgt, wsum, loss_out=a, oy=1):
        return lib.nint_loss_mse_l1_crop_weighted(a, a, wgt, wsum, None, loss_out, None, 2, 3, 12, 20, oy, 2, 10, 16, None)

    def fused(wgt, wsum, loss_out=a, Chp=16, oy=1):
        return lib.nint_head_loss_fused_weighted(a, 0, 2, 8, Chp, 3, a, a, a, wgt, wsum, a, a, loss_out, None, C.byref(g), oy, 2,
                                                 10, 16, 0, None)

    def seq(wgt, wsum, loss_out=a, Chp=16, oy=1):
        return lib.nint_head_loss_seq_fused_weighted(a, 2, 3, 8, Chp, 3, a, a, a, wgt, wsum, a, a, loss_out, None, C.byref(g), oy,
                                                     2, 10, 16, 0, None)

    for f in (crop, fused, seq):
        assert f(None, 100.0) == E_ARG, f.__name__
        for ws in bad_wsum:
            assert f(a, ws) == E_ARG, (f.__name__, ws)
        for off in (1, 2, 3):
            assert f(a + off, 100.0) == E_ALIGN, (f.__name__, off)
        assert f(a, 100.0, loss_out=a + 4) == E_ALIGN                # the twin's own alignment rule
        assert f(a, 100.0, oy=3) == E_ARG                            # crop outside the grid
        assert f(a + 1, 0.0) == E_ARG                                # argument errors before alignment, as everywhere
    for f in (fused, seq):
        assert f(a, 100.0, Chp=144) == E_SHAPE                       # the Chp limit is unchanged
        assert f(None, 100.0, Chp=144) == E_ARG


def test_cos_latitude_weights_and_grid_latitudes():
    from nasa_niswan_amd.loss import cos_latitude_weights, grid_latitudes
    lat = grid_latitudes(90)
    np.testing.assert_array_equal(lat, -90.0 + (np.arange(90) + 0.5) * (180.0 / 90))     # the expression train.py --test-skill used
    assert lat.dtype == np.float64 and lat[0] == -89.0 and lat[-1] == 89.0
    row = cos_latitude_weights(lat)
    assert row.dtype == np.float32 and row.shape == (90,)
    np.testing.assert_array_equal(row, np.cos(np.deg2rad(lat)).astype(np.float32))
    m = cos_latitude_weights(lat, 144)
    assert m.dtype == np.float32 and m.shape == (90, 144) and m.flags.c_contiguous
    np.testing.assert_array_equal(m, np.repeat(row[:, None], 144, axis=1))
    assert row.max() / row.min() > 40                               # an equatorial row against a polar one on the 2-degree grid
    with pytest.raises(ValueError):
        cos_latitude_weights(np.zeros((3, 4)))


def test_the_trainers_weight_validator():
    from nasa_niswan_amd.loss import validate_loss_weights
    good = WM.wmap(10, 16)
    w, wsum = validate_loss_weights(good, (10, 16))
    assert w.dtype == np.float32 and w.flags.c_contiguous and np.array_equal(w, good) and wsum == WM.wsum_of(good)
    w, wsum = validate_loss_weights(torch.from_numpy(good).double(), (10, 16))
    assert np.array_equal(w, good) and wsum == WM.wsum_of(good)
    # a (Hc,) vector means row weights: kept until the crop is known, then expanded
    rows = np.linspace(0.0, 1.0, 10)
    v, none = validate_loss_weights(rows)
    assert v.shape == (10,) and none is None
    w, wsum = validate_loss_weights(rows, (10, 16))
    assert w.shape == (10, 16) and np.array_equal(w, np.repeat(rows.astype(np.float32)[:, None], 16, axis=1))
    assert wsum == float(w.astype(np.float64).sum())
    for bad, why in ((-good, "negative"), (np.where(good > 0.5, np.nan, good), "NaN"), (np.where(good > 0.5, np.inf, good), "inf"),
                     (np.zeros((10, 16)), "all zero"), (np.full((10, 16), 1e300), "overflows f32"), (np.ones((2, 10, 16)), "3-d"),
                     (np.zeros((0,)), "empty")):
        with pytest.raises(ValueError):
            validate_loss_weights(bad)
    for shape in ((16, 10), (10, 15), (9, 16)):
        with pytest.raises(ValueError):
            validate_loss_weights(np.ones(shape), (10, 16))
    with pytest.raises(ValueError):
        validate_loss_weights(np.ones(9), (10, 16))
    tiny = np.zeros((10, 16)); tiny[4, 4] = 1e-60                    # positive in f64, zero in f32: the map the device sees is all zero
    with pytest.raises(ValueError):
        validate_loss_weights(tiny)


@pytest.mark.parametrize("Hc,Wc", [(10, 16), (9, 11), (90, 144), (4, 5), (5, 9), (4, 7), (140, 212)])
def test_the_test_maps_keep_at_least_half_of_the_cells(Hc, Wc):
    w = WM.wmap(Hc, Wc)
    assert w.dtype == np.float32 and not w[0].any() and not w[:, -1].any() and (w[1:, :-1] > 0).sum() > 0
    assert 2 * (w > 0).sum() >= w.size
    if (Hc, Wc) == (10, 16):
        assert (w == 0).sum() == 40 and not w[3:6, 4:9].any()       # 16 + 9 + 15 of 160: 25 %
    r = w[1:3, :-1] / w[1:3, :1]
    assert np.abs(r[0] - r[1]).max() < 1e-6 and np.ptp(w[1, :-1]) > 0   # rows scale a common, non-constant column profile


@pytest.mark.parametrize("N,O,H,W,oy,ox,Hc,Wc", [(2, 3, 12, 20, 1, 2, 10, 16), (2, 3, 9, 11, 0, 0, 9, 11)])
def test_host_model_against_torch_autograd_and_sklearn(N, O, H, W, oy, ox, Hc, Wc):
    """On f64 inputs the model's loss and dpred equal CPU autograd of the same loss, and its R2 sklearn's weighted r2_score,
    to 1e-9.  (pred and y are f32 values, so d = p - y formed in f32 by the model differs from the f64 difference by one f32
    rounding; the inputs are therefore drawn on a 2^-10 grid, where that subtraction is exact.)"""
    from sklearn.metrics import r2_score
    rng = np.random.default_rng(7)
    q = lambda a: (np.round(a * 1024) / 1024).astype(np.float32)
    pred, y, w = q(rng.standard_normal((N, O, H, W))), q(rng.standard_normal((N, O, Hc, Wc))), WM.wmap(Hc, Wc)
    pred[0, 0, oy + 1, ox] = y[0, 0, 1, 0]                           # sign(0) = 0
    ref = WM.loss(pred, y, w, oy, ox)
    pt = torch.from_numpy(pred).double().requires_grad_(True)
    lt = WM.loss_torch(pt, torch.from_numpy(y).double(), w, oy, ox)
    lt.backward()
    assert abs(float(lt.detach()) - ref["loss"]) <= 1e-9
    g = pt.grad.numpy()
    assert np.abs(g - ref["dpred"].astype(np.float64)).max() <= 2.0 ** -24 * np.abs(g).max()     # the model rounds dpred to f32 once
    cnt = N * O * WM.wsum_of(w)
    inv = 1.0 / cnt
    d = pred[:, :, oy:oy + Hc, ox:ox + Wc].astype(np.float64) - y
    np.testing.assert_allclose(g[:, :, oy:oy + Hc, ox:ox + Wc], (2 * d + np.sign(d)) * inv * w, rtol=1e-9, atol=1e-15)
    outside = np.ones((H, W), bool)
    outside[oy:oy + Hc, ox:ox + Wc] = False
    assert not ref["dpred"][:, :, outside].any() and not ref["dpred"][:, :, oy:oy + Hc, ox:ox + Wc][:, :, w == 0].any()
    assert ref["sums"][4] == cnt
    wb = np.broadcast_to(w, y.shape).astype(np.float64)
    p_crop = pred[:, :, oy:oy + Hc, ox:ox + Wc].astype(np.float64)
    want = r2_score(y.astype(np.float64).ravel(), p_crop.ravel(), sample_weight=wb.ravel())
    assert abs(ref["r2"] - want) <= 1e-9 and abs(WM.r2_weighted(y, p_crop, w) - want) <= 1e-9
    assert 0 < ref["r2_tol"] < 1e-9
    # NaN targets under the mask change nothing
    y_nan = y.copy()
    y_nan[:, :, w == 0] = np.nan
    ref2 = WM.loss(pred, y_nan, w, oy, ox)
    assert np.array_equal(ref2["dpred"], ref["dpred"]) and np.array_equal(ref2["sums"], ref["sums"]) and ref2["r2"] == ref["r2"]
    # unit weights: small_audit's unweighted model, bit for bit
    from oracle import small_audit as SM
    one, plain = WM.loss(pred, y, np.ones((Hc, Wc), np.float32), oy, ox), SM.loss(pred, y, oy, ox)
    assert np.array_equal(one["dpred"], plain["dpred"]) and np.array_equal(one["sums"], plain["sums"]) and one["loss"] == plain["loss"]


def test_train_py_flags_reach_configurations_json(tmp_path):
    from nasa_niswan_amd.train import get_arguments
    args = get_arguments(["--snapshot-dir", str(tmp_path), "--lat-weighted-loss", "--loss-weights", "m.npy"])
    assert args.lat_weighted_loss is True and args.loss_weights == "m.npy"
    import json
    cfg = json.load(open(tmp_path / "configurations.json"))
    assert cfg["lat_weighted_loss"] is True and cfg["loss_weights"] == "m.npy"
    args = get_arguments(["--snapshot-dir", str(tmp_path)])
    assert args.lat_weighted_loss is False and args.loss_weights is None
