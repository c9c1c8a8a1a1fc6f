"""CPU tests of the static-attribute input channels (reference dataset.py:100-122, used at :531-533 / :622-624): the
golden taken from the reference's own __getitem__ against the numpy restatement, the host side of the datasets
(statistics, channel count, refusals), the train.py flag, and the argument checks of the three new C entry points."""
import ctypes as C
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def lib():
    from nasa_niswan_amd import _lib
    return _lib.load()


def restate(window, S, padding, mode="reference"):
    """the reference's static path restated with the oracle: z-score over space, repeat over T, concatenate after the
    dynamic channels, pad"""
    from oracle import preproc_oracle as PO
    Sz = PO.zscore(S[None], S.mean(axis=(1, 2)), S.std(axis=(1, 2)))[0]
    x = np.concatenate([window, np.repeat(Sz[None], window.shape[0], axis=0)], axis=1)
    return PO.padding_data_4d(x, tuple(int(v) for v in padding), mode).astype(np.float32)


@pytest.mark.parametrize("case", ["s3", "s16"])
def test_reference_golden_equals_the_restatement_bit_for_bit(case):
    g = np.load(os.path.join(GOLD, "static_pad4d.npz"))
    window, S, X, padding = g[case + ".window"], g[case + ".S"], g[case + ".X"], g[case + ".padding"]
    T, nS = window.shape[0], S.shape[0]
    assert nS == {"s3": 3, "s16": 16}[case] and X.shape == (T, 5 + nS, padding[0], padding[1])
    assert np.array_equal(restate(window, S, padding), X)
    # the mode-0 quirk runs across the whole C: the top halo row of u (channel 0) is row 1 of the LAST static channel,
    # and the top halo row of the last static channel is row 1 of u
    H, W = S.shape[1:]
    pl, pt = (padding[1] - W) // 2, (padding[0] - H) // 2
    assert pt >= 1
    Sz = (S[-1] - S.mean(axis=(1, 2))[-1]) / S.std(axis=(1, 2))[-1]
    np.testing.assert_array_equal(X[:, 0, 0, pl:pl + W], np.repeat(Sz[None, 1], T, 0))
    np.testing.assert_array_equal(X[:, -1, 0, pl:pl + W], window[:, 0, 1, :])
    np.testing.assert_array_equal(X[:, 5, pt:pt + H, pl:pl + W], np.repeat(((S[0] - S.mean(axis=(1, 2))[0]) / S.std(axis=(1, 2))[0])[None], T, 0))


def _arrays(n, L, H, W, seed=5):
    rng = np.random.default_rng(seed)
    sh = (n, L, H, W) if L > 1 else (n, H, W)
    u, v, w, c = (rng.standard_normal(sh).astype(np.float32) for _ in range(4))
    pr, src = (np.abs(rng.standard_normal((n, H, W))).astype(np.float32) for _ in range(2))
    return u, v, w, pr, src, c


@pytest.mark.parametrize("L", [1, 2])
def test_from_arrays_static_statistics_and_channel_count(L):
    from nasa_niswan_amd.dataset import E33OMA90D_CRNN
    n, H, W = 30, 12, 16
    rng = np.random.default_rng(9)
    S = (rng.uniform(-3, 3, (3, 1, 1)) + rng.uniform(0.1, 50, (3, 1, 1)) * rng.standard_normal((3, H, W))).astype(np.float64)
    arrs = _arrays(n, L, H, W)
    plain = E33OMA90D_CRNN.from_arrays(*arrs, padding=(16, 22), sequence_length=4, device="cpu", pinned=False)
    ds = E33OMA90D_CRNN.from_arrays(*arrs, padding=(16, 22), sequence_length=4, device="cpu", pinned=False, static=S)
    C0 = 3 * L + 2
    assert plain.in_channels == C0 and plain.static is None and plain.X_mean.shape == (C0,)
    assert ds.in_channels == C0 + 3 and ds.X_mean.shape == ds.X_std.shape == (C0 + 3,)
    assert ds.X_mean.dtype == ds.X_std.dtype == np.float32
    S32 = S.astype(np.float32)                             # converted to f32 like the other fields, then the reference's expression
    assert ds.static.dtype == np.float32 and np.array_equal(ds.static, S32)
    assert np.array_equal(ds.X_mean[C0:], S32.mean(axis=(1, 2))) and np.array_equal(ds.X_std[C0:], S32.std(axis=(1, 2)))
    assert np.array_equal(ds.S_mean, ds.X_mean[C0:]) and np.array_equal(ds.S_std, ds.X_std[C0:])
    # the dynamic statistics do not move
    assert np.array_equal(ds.X_mean[:C0], plain.X_mean) and np.array_equal(ds.X_std[:C0], plain.X_std)
    assert len(ds) == len(plain)
    with pytest.raises(ValueError, match="static"):
        E33OMA90D_CRNN.from_arrays(*arrs, padding=(16, 22), sequence_length=4, device="cpu", pinned=False, static=S[:, :-1])
    with pytest.raises(ValueError, match="static"):
        E33OMA90D_CRNN.from_arrays(*arrs, padding=(16, 22), sequence_length=4, device="cpu", pinned=False, static=S[0])
    flat = S.copy()
    flat[2] = 7.0
    with pytest.raises(ValueError, match="static channel 2"):
        E33OMA90D_CRNN.from_arrays(*arrs, padding=(16, 22), sequence_length=4, device="cpu", pinned=False, static=flat)


def test_synthetic_static_channels():
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    kw = dict(padding=(100, 154), sequence_length=6, n_steps=40, device="cpu", seed=3)
    ds = SyntheticE33OMA_CRNN("train", in_channels=8, static_channels=3, **kw)
    base = SyntheticE33OMA_CRNN("train", in_channels=5, **kw)
    assert not ds.generic and ds.in_channels == 8 and ds.static.shape == (3, 90, 144) and ds.static.dtype == np.float32
    assert ds.X_mean.shape == ds.X_std.shape == (8,)
    assert np.array_equal(ds.X_mean[5:], ds.static.mean(axis=(1, 2))) and np.array_equal(ds.X_std[5:], ds.static.std(axis=(1, 2)))
    assert (ds.S_std > 0).all()
    # smooth: neighbouring points differ by far less than the field's spread
    assert (np.abs(np.diff(ds.static, axis=2)).max(axis=(1, 2)) < 0.5 * ds.static.std(axis=(1, 2))).all()
    # seeded, and the dynamic fields of a seed do not depend on S
    again = SyntheticE33OMA_CRNN("val", in_channels=8, static_channels=3, **kw)
    assert np.array_equal(again.static, ds.static)
    assert np.array_equal(ds.u, base.u) and np.array_equal(ds.yraw, base.yraw) and np.array_equal(ds.X_mean[:5], base.X_mean)
    assert not np.array_equal(SyntheticE33OMA_CRNN("train", in_channels=8, static_channels=3, **dict(kw, seed=4)).static, ds.static)
    wide = SyntheticE33OMA_CRNN("train", in_channels=3 * 2 + 2 + 16, static_channels=16, levels=2, **kw)
    assert wide.X_mean.shape == (24,) and wide.static.shape == (16, 90, 144)
    for bad in (7, 9, 5):
        with pytest.raises(ValueError, match="in_channels"):
            SyntheticE33OMA_CRNN("train", in_channels=bad, static_channels=3, **kw)
    with pytest.raises(ValueError):
        SyntheticE33OMA_CRNN("train", in_channels=5, static_channels=-1, **kw)


def test_in_channels_8_without_static_is_still_generic():
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    ds = SyntheticE33OMA_CRNN("train", padding=(100, 154), in_channels=8, sequence_length=4, n_steps=24, device="cpu")
    assert ds.generic and ds.static is None and ds.X_mean.shape == (8,)
    (f,), _ = ds.window(0)
    assert f.shape == (4, 8, 90, 144)


def test_get_arguments_parses_static_channels(tmp_path, monkeypatch):
    import json
    from nasa_niswan_amd.train import get_arguments
    monkeypatch.delenv("RANK", raising=False)
    snap = tmp_path / "snap"
    # the reference launcher's LSTM line (launcher.sh:13-30) plus the static-attribute count it implies
    args = get_arguments(["--model", "LSTM-64K5.32K3.16K3-E33OMA-8C-BCB", "--species", "bcb", "--learning-rate", "1.0E-03",
                          "--dataset", "E33OMA", "--in-channels", "8", "--hidden-channels", "64", "32", "16",
                          "--kernel-size", "5", "3", "3", "--num-layers", "3", "--sequence-length", "48",
                          "--num-epochs", "30", "--input-size", "100", "154", "--batch-size", "8", "--num-workers", "1",
                          "--scheduler-config", "10", "0.9", "--betas", "0.5", "0.999", "--snapshot-dir", str(snap),
                          "--restore-from", str(snap), "--static-channels", "3"])
    assert args.static_channels == 3 and args.in_channels == 8
    assert json.load(open(snap / "configurations.json"))["static_channels"] == 3
    assert get_arguments(["--snapshot-dir", str(snap)]).static_channels == 0


def test_static_entry_points_reject_bad_arguments_without_touching_the_gpu(lib):
    """nstatic outside [0, nsrc] and NULL pointers are refused with NINT_E_ARG before any HIP call; the pointers below are
    never dereferenced (argument validation runs on the host)."""
    from nasa_niswan_amd import _lib
    E_ARG = _lib.NINT_E_ARG
    srcs = (C.c_void_p * 2)(16, 16)
    lev = (C.c_int * 2)(5, 3)
    t0 = (C.c_int * 1)(0)
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 16, 22, 2) == 0
    for ns in (-1, 3, 1 << 20):
        assert lib.nint_preproc_fuse_pad_static(srcs, lev, 2, ns, 16, 16, 16, 2, 12, 16, 16, 22, 0, None) == E_ARG, ns
        assert lib.nint_preproc_fuse_pad_static_batch(srcs, lev, 2, ns, 16, 16, t0, 1, 16, 2, 12, 16, 16, 22, 0, None) == E_ARG, ns
        assert lib.nint_preproc_fuse_pad_static_slab(srcs, lev, 2, ns, 16, 16, t0, 1, 16, 16, 0, 2, 12, 16, C.byref(g), 0, 1,
                                                     None) == E_ARG, ns
    # null pointers
    assert lib.nint_preproc_fuse_pad_static(None, None, 0, 0, None, None, None, 1, 5, 5, 13, 13, 0, None) == E_ARG
    assert lib.nint_preproc_fuse_pad_static_batch(srcs, lev, 2, 1, None, 16, t0, 1, 16, 2, 12, 16, 16, 22, 0, None) == E_ARG
    assert lib.nint_preproc_fuse_pad_static_batch(srcs, lev, 2, 1, 16, 16, None, 1, 16, 2, 12, 16, 16, 22, 0, None) == E_ARG
    assert lib.nint_preproc_fuse_pad_static_slab(srcs, lev, 2, 1, 16, 16, t0, 1, None, 16, 0, 2, 12, 16, C.byref(g), 0, 1,
                                                 None) == E_ARG
    assert lib.nint_preproc_fuse_pad_static_slab(srcs, lev, 2, 1, 16, 16, t0, 1, 16, 16, 0, 2, 12, 16, None, 0, 1, None) == E_ARG
    nul = (C.c_void_p * 2)(16, None)
    assert lib.nint_preproc_fuse_pad_static(nul, lev, 2, 1, 16, 16, 16, 2, 12, 16, 16, 22, 0, None) == E_ARG
    # a static source of 0 levels, and a negative window start
    lev0 = (C.c_int * 2)(5, 0)
    assert lib.nint_preproc_fuse_pad_static_batch(srcs, lev0, 2, 1, 16, 16, t0, 1, 16, 2, 12, 16, 16, 22, 0, None) == E_ARG
    tneg = (C.c_int * 1)(-1)
    assert lib.nint_preproc_fuse_pad_static_batch(srcs, lev, 2, 1, 16, 16, tneg, 1, 16, 2, 12, 16, 16, 22, 0, None) == E_ARG
