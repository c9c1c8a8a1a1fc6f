"""GPU tests of the static-attribute input channels (reference dataset.py:100-122, used at :531-533 / :622-624): the
preproc kernels with time-invariant sources against the golden taken from the reference's own __getitem__, the batch and
slab paths against each other and the numpy restatement, the no-static entry points unchanged, the reference launcher's
canonical shape ConvLSTM(8, [64,32,16], [5,3,3], 3) on 100x154 at T = 48 against the CPU oracle, and train.py with
--static-channels end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    from nasa_niswan_amd import _lib
    return _lib.load()


def _sz(S):
    from oracle import preproc_oracle as PO
    return PO.zscore(S[None], S.mean(axis=(1, 2)), S.std(axis=(1, 2)))[0]


def restate_window(dyn_z, S, padding, mode):
    """dynamic channels already z-scored (T, C0, H, W) + static attributes (S, H, W) -> padded (T, C0+S, Hp, Wp)"""
    from oracle import preproc_oracle as PO
    x = np.concatenate([dyn_z, np.repeat(_sz(S)[None], dyn_z.shape[0], axis=0)], axis=1)
    return PO.padding_data_4d(x, tuple(int(v) for v in padding), mode).astype(np.float32)


def restate_sample(ds, i, mode):
    """sample i of a dataset with static attributes: fuse + z-score (dataset.py:526-528), static appended, pad"""
    from oracle import preproc_oracle as PO
    fields, _ = ds.window(i)
    C0 = len(ds.X_mean) - ds.static.shape[0]
    dyn = PO.zscore(PO.fuse_levels(*fields), ds.X_mean[:C0], ds.X_std[:C0])
    return restate_window(dyn, ds.static, ds.padding, mode)


def _vp(*ts):
    return (C.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _stream():
    from nasa_niswan_amd._lib import stream_ptr
    return stream_ptr()


@pytest.mark.parametrize("case", ["s3", "s16"])
def test_static_kernel_matches_reference_golden(lib, case):
    """nint_preproc_fuse_pad_static on the golden's inputs: the window (already z-scored in the reference: mean 0 / std 1
    here) and the raw static fields with the reference's spatial statistics.  Mode 0 against the reference's own output,
    mode 1 against the restatement."""
    g = np.load(os.path.join(GOLD, "static_pad4d.npz"))
    window, S, X, (Hp, Wp) = g[case + ".window"], g[case + ".S"], g[case + ".X"], (int(v) for v in g[case + ".padding"])
    T, C0, H, W = window.shape
    nS = S.shape[0]
    mean = torch.from_numpy(np.concatenate([np.zeros(C0, np.float32), S.mean(axis=(1, 2))])).cuda()
    std = torch.from_numpy(np.concatenate([np.ones(C0, np.float32), S.std(axis=(1, 2))])).cuda()
    wd, sd = torch.from_numpy(window).cuda(), torch.from_numpy(S).cuda()
    for mode, want in ((0, X), (1, restate_window(window, S, (Hp, Wp), "reflect"))):
        out = torch.full((T, C0 + nS, Hp, Wp), float("nan"), device="cuda")
        assert lib.nint_preproc_fuse_pad_static(_vp(wd, sd), _ints(C0, nS), 2, 1, mean.data_ptr(), std.data_ptr(),
                                                out.data_ptr(), T, H, W, Hp, Wp, mode, _stream()) == 0
        torch.cuda.synchronize()
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-6, atol=1e-6)
    # the static source as several sources of one level each: the same tensor (static sources count as ordinary sources)
    if nS <= 15:
        out2 = torch.empty(T, C0 + nS, Hp, Wp, device="cuda")
        assert lib.nint_preproc_fuse_pad_static(_vp(wd, *[sd[s] for s in range(nS)]), _ints(C0, *[1] * nS), 1 + nS, nS,
                                                mean.data_ptr(), std.data_ptr(), out2.data_ptr(), T, H, W, Hp, Wp, 0,
                                                _stream()) == 0
        out1 = torch.empty_like(out2)
        assert lib.nint_preproc_fuse_pad_static(_vp(wd, sd), _ints(C0, nS), 2, 1, mean.data_ptr(), std.data_ptr(),
                                                out1.data_ptr(), T, H, W, Hp, Wp, 0, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(out1, out2)


def test_static_batch_equals_per_sample_and_restatement(pkg, lib):
    """nint_preproc_fuse_pad_static_batch reads every sample's window at its own t0 and the static source at its only
    step: equal to one single-sample call per window; and through the dataset at L = 20, S = 3 (C = 65, 6 sources)."""
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    rng = np.random.default_rng(4)
    n, C0, nS, H, W, Hp, Wp, T = 20, 5, 3, 24, 40, 30, 48, 4
    rec = torch.from_numpy(rng.standard_normal((n, C0, H, W)).astype(np.float32)).cuda()
    S = (rng.standard_normal((nS, H, W)) * 3 + 1).astype(np.float32)
    sd = torch.from_numpy(S).cuda()
    mean = torch.from_numpy(np.concatenate([rng.standard_normal(C0), S.mean(axis=(1, 2))]).astype(np.float32)).cuda()
    std = torch.from_numpy(np.concatenate([rng.uniform(0.5, 2, C0), S.std(axis=(1, 2))]).astype(np.float32)).cuda()
    t0 = [0, 3, 16, 7, 9]
    for mode in (0, 1):
        out = torch.empty(len(t0), T, C0 + nS, Hp, Wp, device="cuda")
        assert lib.nint_preproc_fuse_pad_static_batch(_vp(rec, sd), _ints(C0, nS), 2, 1, mean.data_ptr(), std.data_ptr(),
                                                      _ints(*t0), len(t0), out.data_ptr(), T, H, W, Hp, Wp, mode, _stream()) == 0
        for b, t in enumerate(t0):
            one = torch.empty(T, C0 + nS, Hp, Wp, device="cuda")
            assert lib.nint_preproc_fuse_pad_static(_vp(rec[t], sd), _ints(C0, nS), 2, 1, mean.data_ptr(), std.data_ptr(),
                                                    one.data_ptr(), T, H, W, Hp, Wp, mode, _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(out[b], one), (mode, b)
    for levels, mode, idx in ((20, "reference", [0, 5]), (1, "reflect", [2, 0, 4])):
        Cin = 3 * levels + 2 + nS
        ds = SyntheticE33OMA_CRNN("train", padding=(100, 154), in_channels=Cin, sequence_length=3, levels=levels, n_steps=16,
                                  pad_mode=mode, device="cuda", static_channels=nS)
        ptrs, lev, nstatic = ds._sources(ds._device_arrays())
        assert nstatic == 1 and len(lev) == 6 and lev[5] == nS
        X, y = ds.device_batch(idx)
        torch.cuda.synchronize()
        assert X.shape == (len(idx), 3, Cin, 100, 154)
        for b, i in enumerate(idx):
            np.testing.assert_allclose(X[b].cpu().numpy(), restate_sample(ds, i, mode), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("fold", [True, False], ids=["xfold", "plain"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_static_slab_is_bit_identical_to_preproc_then_pack(pkg, dtype, fold):
    """The slab path with a static source (plain and horizontally folded input layouts) writes the bytes of device_batch
    followed by nint_pack_btchw[_xfold], at the reference launcher's in_channels 8 (S = 3) and at 21 (S = 16), k = 5;
    the channel padding is zero and the values are the restatement rounded to the slab type."""
    from nasa_niswan_amd import engine
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    engine.XFOLD = fold
    try:
        for nS, mode, idx in ((3, "reference", [3, 0, 9]), (16, "reflect", [1, 5])):
            Cin, k, T = 5 + nS, 5, 3
            ds = SyntheticE33OMA_CRNN("train", padding=(100, 154), in_channels=Cin, sequence_length=T, n_steps=24,
                                      pad_mode=mode, device="cuda", static_channels=nS)
            eng = SeqEngine([LayerCfg(Cin, 16, k)], dtype, "cuda")
            folded = eng.cfgs[0].xfold
            assert folded == fold
            B = len(idx)
            ws_a = eng.acquire(B, T, 100, 154, False, False)
            ws_b = eng.acquire(B, T, 100, 154, False, False)
            sb, y1 = ds.slab_batch(idx)
            eng.pack_input(ws_a, sb)
            X, y2 = ds.device_batch(idx)
            eng.pack_input(ws_b, X)
            torch.cuda.synchronize()
            assert torch.equal(ws_a.xs, ws_b.xs) and torch.equal(y1, y2), (nS, mode)
            g, Cp = ws_a.g, ws_a.Cxp0
            et = torch.float32 if dtype == "f32" else torch.bfloat16
            full = ws_a.xs.view(et).view(T * B, g.Hh, g.Wh, Cp)
            slab = full[:, g.P:g.P + 100, g.P:g.P + 154].float().cpu()
            nch = Cin * k if folded else Cin
            assert float(full[:, :, :, nch:].abs().max()) == 0.0                     # channel padding zero
            for b, i in enumerate(idx):
                want = torch.from_numpy(restate_sample(ds, i, mode)).to(et).float().permute(0, 2, 3, 1)   # (T,Hp,Wp,C)
                if folded:     # channel kx*C + c of pixel x = channel c of pixel x + kx - k//2, zero outside
                    pad = torch.nn.functional.pad(want, (0, 0, k // 2, k // 2))
                    want = torch.cat([pad[:, :, kx:kx + 154] for kx in range(k)], dim=3)
                got = slab[b::B][:, :, :, :nch]
                if dtype == "f32":
                    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-6, atol=1e-6)
                else:   # the f32 value may differ from numpy's in the last bit before rounding: <= 1 bf16 ulp, and rarely
                    d = (got - want).abs()
                    assert float((d > 0).float().mean()) < 1e-3 and float((d / (want.abs() + 1e-6)).max()) <= 2 ** -7
            eng.release(ws_a); eng.release(ws_b)
    finally:
        engine.XFOLD = True


def test_static_entry_points_with_no_static_source_write_the_old_bytes(pkg, lib):
    """nstatic = 0: the _static entry points and the three existing ones write identical bytes on the same inputs."""
    from nasa_niswan_amd import _lib
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    ds = SyntheticE33OMA_CRNN("train", padding=(100, 154), in_channels=14, sequence_length=3, levels=4, n_steps=16,
                              device="cuda")
    dv = ds._device_arrays()
    ptrs, lev, nstatic = ds._sources(dv)
    assert nstatic == 0
    H, W = ds.grid
    Cc, T, t0 = 14, 3, [4, 0, 7]
    m, s = dv["mean"].data_ptr(), dv["std"].data_ptr()
    for mode in (0, 1):
        a = torch.full((T, Cc, 100, 154), float("nan"), device="cuda")
        b = torch.full_like(a, float("nan"))
        one = (C.c_void_p * len(lev))(*[ptrs[i] + 4 * 3 * lev[i] * H * W for i in range(len(lev))])    # windows at step 3
        assert lib.nint_preproc_fuse_pad(one, lev, len(lev), m, s, a.data_ptr(), T, H, W, 100, 154, mode, _stream()) == 0
        assert lib.nint_preproc_fuse_pad_static(one, lev, len(lev), 0, m, s, b.data_ptr(), T, H, W, 100, 154, mode,
                                                _stream()) == 0
        ab = torch.full((3, T, Cc, 100, 154), float("nan"), device="cuda")
        bb = torch.full_like(ab, float("nan"))
        assert lib.nint_preproc_fuse_pad_batch(ptrs, lev, len(lev), m, s, _ints(*t0), 3, ab.data_ptr(), T, H, W, 100, 154,
                                               mode, _stream()) == 0
        assert lib.nint_preproc_fuse_pad_static_batch(ptrs, lev, len(lev), 0, m, s, _ints(*t0), 3, bb.data_ptr(), T, H, W,
                                                      100, 154, mode, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ab.view(torch.int32), bb.view(torch.int32))
        for dt, kf in ((_lib.NINT_BF16, 0), (_lib.NINT_F32, 0), (_lib.NINT_BF16, 5)):
            g = _lib.NintGeom()
            assert lib.nint_geom_make(C.byref(g), 100, 154, 2) == 0
            Cxp = 80 if kf else 16
            nbytes = 3 * T * g.Hh * g.Wh * Cxp * (2 if dt == _lib.NINT_BF16 else 4)
            xa = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
            xb = torch.full_like(xa, 0xA5)
            assert lib.nint_preproc_fuse_pad_slab(ptrs, lev, len(lev), m, s, _ints(*t0), 3, xa.data_ptr(), Cxp, kf, T, H, W,
                                                  C.byref(g), mode, dt, _stream()) == 0
            assert lib.nint_preproc_fuse_pad_static_slab(ptrs, lev, len(lev), 0, m, s, _ints(*t0), 3, xb.data_ptr(), Cxp, kf,
                                                         T, H, W, C.byref(g), mode, dt, _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(xa, xb), (mode, dt, kf)
            assert not torch.equal(xa, torch.full_like(xa, 0xA5))


def _check(res, dtype):
    """the standing tolerances of tests/test_gpu_fullsize.py"""
    for k, (a, b) in res.items():
        a, b = a.double().numpy(), b.double().numpy()
        assert np.isfinite(a).all(), k
        r = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
        if dtype == "f32":
            err, ref = np.abs(a - b).max(), np.abs(b).max()
            print(f"  {k}: max abs err {err:.2e} (ref max {ref:.2e}), rel-L2 {r:.2e}")
            if k == "pred":
                np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)
            elif k == "loss":
                assert err <= 2e-6 * ref, (k, err, ref)
            else:
                assert err <= 1e-3 * ref + 1e-9, (k, err, ref)
        else:
            print(f"  {k}: rel-L2 {r:.2e}")
            assert r <= 2e-2, (k, r)


@pytest.fixture(scope="module")
def canonical(pkg):
    """The reference launcher's run (launcher.sh:13-30, "8C"): a from_arrays record with S = 3 static attributes on the
    90x144 grid padded to 100x154, T = 48, one window; the oracle's fit-loop step on device_batch's X (shared by both
    dtypes: the oracle is the expensive part)."""
    import time
    from nasa_niswan_amd.dataset import E33OMA90D_CRNN
    from oracle import convlstm_oracle as O
    rng = np.random.default_rng(48)
    n, H, W, T = 60, 90, 144, 48
    arrs = [(rng.standard_normal((n, H, W)) * s + m).astype(np.float32)
            for m, s in ((0.2, 6.5), (0.3, 5.3), (0, 6e-5), (2.2, 7.3), (0.2, 2.6), (5.0, 57.0))]
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 2 * np.pi, W), indexing="ij")
    static = np.stack([100 + 40 * np.sin(xx) * yy, np.cos(2 * xx + 3 * yy), 0.01 * (yy - 0.3) ** 2 + 1e-3 * np.cos(xx)])
    ds = E33OMA90D_CRNN.from_arrays(*arrs, period="train", padding=(100, 154), sequence_length=T, device="cuda",
                                    static=static)
    assert ds.in_channels == 8
    idx = [7]
    X, y = ds.device_batch(idx)
    params = O.synth_params(8, [64, 32, 16], [5, 3, 3], 3, seed=48)
    t = time.time()
    _, _, oloss, opred, ograds = O.train_step(params, None, X.cpu(), y.cpu(), lr=1e-3, halo=(5, 5))
    print(f"  oracle fit-loop step at T = 48, 100x154, C = 8: {time.time() - t:.1f} s")
    return ds, idx, params, oloss, opred, ograds


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_canonical_launch_8c_t48_vs_oracle(pkg, canonical, dtype):
    """ConvLSTM(8, [64,32,16], [5,3,3], 3) on 100x154, T = 48, B = 1, fed from slab_batch through the fused fit-loop step:
    prediction, loss and all 8 gradients against the oracle's step on device_batch's X (which the tests above tie to the
    restatement)."""
    from nasa_niswan_amd.trainer import FusedTrainer
    ds, idx, params, oloss, opred, ograds = canonical
    net = pkg.ConvLSTM(8, [64, 32, 16], [5, 3, 3], 3, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=1e-3, halo=(5, 5))
    sb, y = ds.slab_batch(idx)
    eng, ws, pred, _ = tr.forward_loss(sb, y, train=False)
    pred = pred[0, 0, 5:95, 5:149].detach().cpu()
    eng.release(ws)
    loss = float(tr.step(sb, y))
    torch.cuda.synchronize()
    res = {"pred": (pred, opred), "loss": (torch.tensor([loss]), torch.tensor([oloss]))}
    for k, p in net.named_parameters():
        res["grad." + k] = (p.grad.detach().cpu(), ograds[k])
    print(f"  [{dtype}] loss {loss:.7f} (oracle {oloss:.7f})")
    _check(res, dtype)


def test_train_py_static_channels_t48(pkg, tmp_path, monkeypatch):
    """train.py with the reference launcher's --in-channels 8 --sequence-length 48 plus --static-channels 3 (small model,
    short synthetic record): the first step's loss equals the oracle's fit-loop step on the same first batch."""
    from nasa_niswan_amd import train as T
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from nasa_niswan_amd.utils import shard_indices
    from oracle import convlstm_oracle as O
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--model", "LSTM-8C", "--in-channels", "8", "--static-channels", "3", "--hidden-channels", "8", "--kernel-size", "3",
            "--num-layers", "1", "--sequence-length", "48", "--input-size", "32", "32", "--grid", "32", "32", "--batch-size", "2",
            "--num-epochs", "1", "--learning-rate", "1e-4", "--synthetic-steps", "170", "--dtype", "f32",
            "--snapshot-dir", str(tmp_path / "s")]
    logger = T.main(T.get_arguments(argv))
    assert len(logger["MSELoss"]) == 1 and np.isfinite(logger["MSELoss"]).all() and np.isfinite(logger["r2_score_val"]).all()
    ds = SyntheticE33OMA_CRNN("train", padding=(32, 32), in_channels=8, sequence_length=48, n_steps=170, grid=(32, 32),
                              device="cuda", static_channels=3)
    assert not ds.generic and ds.static.shape == (3, 32, 32)
    idx = shard_indices(len(ds), 1, 0, 1, 2)
    X, y = ds.device_batch(idx[0])
    params = O.init_params(8, [8], [3], 1, seed=0)                    # seed(0) then ConvLSTM(...): train.py:32,48
    _, _, oloss, _, _ = O.train_step(params, None, X.cpu(), y.cpu(), lr=1e-4, halo=(0, 0))
    print(f"  first-step loss {logger['first_step_loss']:.7f}, oracle {oloss:.7f}")
    assert abs(logger["first_step_loss"] - oloss) <= 2e-6 * abs(oloss)
    with pytest.raises(ValueError, match="in_channels"):
        T.main(T.get_arguments(argv[:4] + ["--static-channels", "2"] + argv[6:]))
