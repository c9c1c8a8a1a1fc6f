"""GPU tests of the evaluation skill sums: nint_skill_accum against numpy f64, bit-reproducibility under splits of a call,
the fused nint_head_skill_accum against nint_head_fwd + nint_skill_accum bit for bit, and inference.evaluate_skill /
train.py --test-skill end to end against the analysis notebook's expressions (test.ipynb:377-385, :462-485, :796-803)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import small_audit as SM

pytestmark = pytest.mark.gpu

PIXN, SMPN = 5, 8


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as pkg
    return pkg.load_library()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def geom(lib, H, W, Pd):
    from nasa_niswan_amd._lib import NintGeom
    g = NintGeom()
    assert lib.nint_geom_make(C.byref(g), H, W, Pd) == 0
    return g


def i32(v):
    return (C.c_int32 * len(v))(*[int(a) for a in v])


def plain(lib, pred, y, slot, nslots, row_w, pix, halo):
    """one nint_skill_accum call; returns the sample rows"""
    N, O, H, W = pred.shape
    Hc, Wc = y.shape[-2:]
    sample = torch.full((N, O, SMPN), float("nan"), dtype=torch.float64, device="cuda")
    nb = lib.nint_skill_scratch_bytes(N, O, Hc, Wc)
    scratch = torch.empty(nb // 8, dtype=torch.float64, device="cuda")
    assert lib.nint_skill_accum(P(pred), P(y), None if slot is None else i32(slot), nslots, P(row_w), P(pix), P(sample), P(scratch),
                                nb, N, O, H, W, halo[0], halo[1], Hc, Wc, None) == 0
    return sample


def terms_np(pred, y, halo, row_w):
    """per element, f64: the five map terms (5, N, O, Hc, Wc) and the eight sample terms (8, N, O, Hc, Wc)"""
    Hc, Wc = y.shape[-2:]
    p = pred[:, :, halo[0]:halo[0] + Hc, halo[1]:halo[1] + Wc].astype(np.float64)
    t = y.astype(np.float64)
    d = p - t
    w = row_w[None, None, :, None] * np.ones_like(t)
    return np.stack([t, p, t * t, p * p, d * d]), np.stack([d * d, np.abs(d), t, t * t, p, p * p, w * t, w * p])


@pytest.fixture(scope="module")
def small(lib):
    """N = 5, O = 2, 13 x 21 grid, crop 9 x 15 at (2, 3): the data, and ONE call over all five samples"""
    torch.manual_seed(23)
    N, O, H, W, halo, Hc, Wc = 5, 2, 13, 21, (2, 3), 9, 15
    pred = torch.randn(N, O, H, W, device="cuda")
    y = torch.randn(N, O, Hc, Wc, device="cuda")
    row_w = torch.rand(Hc, dtype=torch.float64, device="cuda") + 0.25
    slot = [0, 1, -1, 0, 1]
    pix = torch.zeros(2, PIXN, O, Hc, Wc, dtype=torch.float64, device="cuda")
    sample = plain(lib, pred, y, slot, 2, row_w, pix, halo)
    torch.cuda.synchronize()
    return dict(pred=pred, y=y, row_w=row_w, slot=slot, halo=halo, pix=pix, sample=sample)


def test_plain_entry_matches_numpy_f64(lib, small):
    """Every map cell and every sample row against the exact sum of its f64 addends (math.fsum), within gamma(n - 1) * sum
    |addends| with u = 2^-53 and n the number of addends (at most three samples for a cell, 135 pixels for a row): the bound of
    any summation order, which is the only freedom -- products are single f64 operations (oracle.small_audit.skill_audit)."""
    s = small
    pred_h, y_h, roww_h = s["pred"].cpu().numpy(), s["y"].cpu().numpy(), s["row_w"].cpu().numpy()
    mt, st = terms_np(pred_h, y_h, s["halo"], roww_h)
    pix, sample = s["pix"].cpu().numpy(), s["sample"].cpu().numpy()
    r = SM.skill_audit(pred_h, y_h, s["halo"][0], s["halo"][1], s["slot"], 2, roww_h, np.zeros_like(pix), pix, sample)
    print(f"  largest err / (gamma(n-1) sum|terms|): maps {r[0]:.2e}, sample rows {r[1]:.2e}")
    assert r[0] <= 1.0 and r[1] <= 1.0 and SM.gamma(134, SM.U64) < 1e-12
    # the slot -1 sample (n = 2) is absent from the maps -- adding its terms to either slot would be far outside the bound --
    # and present in `sample`
    assert np.all(np.abs(mt[:, 2]).sum(axis=0) > 0)
    for sl in (0, 1):
        members = [n for n, v in enumerate(s["slot"]) if v == sl]
        assert np.abs(pix[sl] - mt[:, members + [2]].sum(axis=1)).max() > 1e-3
    assert np.all(np.isfinite(sample[2])) and np.all(sample[2, :, 0] > 0)
    # uniform weights and one slot: NULL row_w, NULL slot
    pix1 = torch.zeros(1, PIXN, 2, 9, 15, dtype=torch.float64, device="cuda")
    smp1 = plain(lib, s["pred"], s["y"], None, 1, None, pix1, s["halo"]).cpu().numpy()
    assert np.array_equal(smp1[..., :6], sample[..., :6]) and np.array_equal(smp1[..., 6], smp1[..., 2]) and np.array_equal(smp1[..., 7], smp1[..., 4])
    SM.skill_audit(pred_h, y_h, s["halo"][0], s["halo"][1], None, 1, None, np.zeros((1, PIXN, 2, 9, 15)), pix1.cpu().numpy(), smp1)


def test_splits_of_a_call_change_no_bit(lib, small):
    s = small
    pred, y, slot, halo, row_w = s["pred"], s["y"], s["slot"], s["halo"], s["row_w"]
    # N = 3 then N = 2 against the one call with N = 5
    pix = torch.zeros_like(s["pix"])
    a = plain(lib, pred[:3], y[:3], slot[:3], 2, row_w, pix, halo)
    b = plain(lib, pred[3:], y[3:], slot[3:], 2, row_w, pix, halo)
    torch.cuda.synchronize()
    assert torch.equal(pix, s["pix"]) and torch.equal(torch.cat([a, b]), s["sample"])
    # a second identical run
    pix2 = torch.zeros_like(s["pix"])
    again = plain(lib, pred, y, slot, 2, row_w, pix2, halo)
    assert torch.equal(pix2, s["pix"]) and torch.equal(again, s["sample"])
    # a sample's row depends neither on N nor on its position in the call
    alone = plain(lib, pred[4:5], y[4:5], [1], 2, row_w, torch.zeros_like(pix), halo)
    assert torch.equal(alone[0], s["sample"][4])
    # N = 70 (more than NINT_SKILL_MAX_N = 64: split inside the library) against two calls
    torch.manual_seed(29)
    N = 70
    predL = torch.randn(N, 2, 13, 21, device="cuda")
    yL = torch.randn(N, 2, 9, 15, device="cuda")
    slotL = [(n % 4) - 1 for n in range(N)]
    pixA = torch.zeros(3, PIXN, 2, 9, 15, dtype=torch.float64, device="cuda")
    one = plain(lib, predL, yL, slotL, 3, row_w, pixA, halo)
    pixB = torch.zeros_like(pixA)
    two = torch.cat([plain(lib, predL[:33], yL[:33], slotL[:33], 3, row_w, pixB, halo),
                     plain(lib, predL[33:], yL[33:], slotL[33:], 3, row_w, pixB, halo)])
    torch.cuda.synchronize()
    assert torch.equal(pixA, pixB) and torch.equal(one, two)
    SM.skill_audit(predL.cpu().numpy(), yL.cpu().numpy(), halo[0], halo[1], slotL, 3, row_w.cpu().numpy(), np.zeros((3, PIXN, 2, 9, 15)),
                   pixA.cpu().numpy(), one.cpu().numpy())          # gamma(n - 1) * sum |addends|, n <= 18 samples per cell


# (the three before the last five: the weight image [O][CHV] beyond 64 KiB while the fused head passes still hold the shape; the last
# five: Ch = CHV, so the 12 staged channels the head's dot product leaves unfused hold data, in both storage types)
@pytest.mark.parametrize("dt,Ch,O", [(0, 16, 20), (1, 16, 20), (1, 8, 1), (0, 48, 3), (1, 128, 20), (1, 128, 200), (0, 48, 300), (0, 16, 600),
                                     (0, 32, 3), (1, 32, 3), (0, 64, 3), (1, 64, 3), (0, 128, 3)])
def test_fused_entry_equals_head_fwd_then_plain_entry(lib, dt, Ch, O):
    """nint_head_skill_accum = nint_head_fwd followed by nint_skill_accum, bit for bit: pred_out, pix and sample (the
    relation nint_head_loss_fused has to its three separate launches; the same shapes, all three CHV instances)."""
    N, H, W, Pd, halo = 3, 20, 28, 2, (5, 4)
    torch.manual_seed(19)
    Hc, Wc = H - 2 * halo[0], W - 2 * halo[1]
    g = geom(lib, H, W, Pd)
    kc = lib.nint_kc(dt)
    Chp = (Ch + kc - 1) // kc * kc
    et = torch.bfloat16 if dt else torch.float32
    hsl = torch.zeros(2 * N, g.Hh, g.Wh, Chp, device="cuda", dtype=et)
    hsl[:, Pd:Pd + H, Pd:Pd + W, :Ch] = torch.randn(2 * N, H, W, Ch, device="cuda").to(et)
    w = torch.randn(O, Ch, device="cuda") * 0.3
    b = torch.randn(O, device="cuda")
    y = torch.randn(N, O, Hc, Wc, device="cuda")
    row_w = torch.rand(Hc, dtype=torch.float64, device="cuda") + 0.5
    slot, n0 = [1, -1, 0], N                                      # the head reads images [n0, n0+N)
    pred = torch.empty(N, O, H, W, device="cuda")
    assert lib.nint_head_fwd(P(hsl), n0, N, Ch, Chp, O, P(w), P(b), P(pred), C.byref(g), dt, None) == 0
    pix1 = torch.zeros(2, PIXN, O, Hc, Wc, dtype=torch.float64, device="cuda")
    smp1 = plain(lib, pred, y, slot, 2, row_w, pix1, halo)
    nb = lib.nint_skill_scratch_bytes(N, O, Hc, Wc)
    scratch = torch.empty(nb // 8, dtype=torch.float64, device="cuda")

    def fused(pred_out, Chp_=Chp):
        pix = torch.zeros_like(pix1)
        smp = torch.full_like(smp1, float("nan"))
        rc = lib.nint_head_skill_accum(P(hsl), n0, N, Ch, Chp_, O, P(w), P(b), P(y), i32(slot), 2, P(row_w), P(pix), P(smp),
                                       P(pred_out), P(scratch), nb, C.byref(g), halo[0], halo[1], Hc, Wc, dt, None)
        return rc, pix, smp
    pout = torch.full((N, O, Hc, Wc), float("nan"), device="cuda")
    rc, pix2, smp2 = fused(pout)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(pout, pred[:, :, halo[0]:halo[0] + Hc, halo[1]:halo[1] + Wc])
    assert torch.equal(pix1, pix2) and torch.equal(smp1, smp2)
    rc, pix3, smp3 = fused(None)                                  # without pred_out: the same sums
    assert rc == 0 and torch.equal(pix1, pix3) and torch.equal(smp1, smp3)
    assert fused(None, 192)[0] == -2                              # NINT_E_SHAPE: wider than the fused kernel holds


def test_head_skill_takes_the_fallback_beyond_the_fused_limit(lib):
    """SeqEngine.head_skill: the fused entry where it holds, head_forward + nint_skill_accum beyond it (here 1100 outputs:
    the [O][CHV] weight image of the fused head passes is beyond the LDS) -- the same sums either way."""
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    from nasa_niswan_amd.inference import SkillAccumulator
    torch.manual_seed(31)
    B, T, Cx, Ch, H, W, halo = 3, 2, 4, 8, 20, 28, (5, 4)
    Hc, Wc = H - 2 * halo[0], W - 2 * halo[1]
    eng = SeqEngine([LayerCfg(Cx, Ch, 3)], "f32", "cuda")
    ws = eng.acquire(B, T, H, W, False, False)
    eng.pack_weights([torch.randn(4 * Ch, Cx + Ch, 3, 3, device="cuda") * 0.2], [torch.randn(4 * Ch, device="cuda") * 0.1])
    eng.forward(ws, torch.randn(B, T, Cx, H, W, device="cuda"))
    slots = [1, 0, -1]
    for O in (3, 1100):
        Chp = eng.cfgs[-1].padded(eng.kc)[2]
        assert eng._beyond_fused_head(Chp, O) == (O == 1100)
        w, b = torch.randn(O, Ch, device="cuda") * 0.3, torch.randn(O, device="cuda")
        y = torch.randn(B, O, Hc, Wc, device="cuda")
        acc = SkillAccumulator(O, Hc, Wc, nslots=2, lat=np.linspace(-40, 40, Hc), device="cuda", halo=halo)
        pout = torch.empty(B, O, Hc, Wc, device="cuda")
        smp = eng.head_skill(ws, w, b, y, slots, acc, pred_out=pout)
        pred = eng.head_forward(ws, w, b)
        pix = torch.zeros_like(acc.pix)
        ref = plain(lib, pred, y, slots, 2, acc.row_w, pix, halo)
        torch.cuda.synchronize()
        assert torch.equal(pout, pred[:, :, halo[0]:halo[0] + Hc, halo[1]:halo[1] + Wc])
        assert torch.equal(acc.pix, pix) and torch.equal(smp, ref)
        if O == 1100:
            scratch = acc.scratch_for(B)
            assert lib.nint_head_skill_accum(P(ws.h[-1]), T * B, B, Ch, Chp, O, P(w), P(b), P(y), i32(slots), 2, None, P(pix), P(smp),
                                             None, P(scratch), scratch.numel() * 8, C.byref(ws.g), halo[0], halo[1], Hc, Wc, eng.dt,
                                             None) == -2
    eng.release(ws)


# ------------------------------------------------------------------------------ end to end
def r_squared_spatial_notebook(real_data, model_output):
    """test.ipynb:480-485"""
    ss_res = np.sum((real_data - model_output) ** 2, axis=0)
    ss_tot = np.sum((real_data - np.mean(real_data, axis=0)) ** 2, axis=0)
    return 1 - (ss_res / ss_tot)


def rel_close(a, b, tol=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    err = np.abs(a - b) / np.abs(b)
    print(f"    max rel err {float(err.max()):.2e}")
    return bool(np.all(err <= tol))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_evaluate_skill_matches_the_notebook_on_the_same_predictions(lib, dtype):
    """evaluate_skill over 21 test windows in batches of 8, 8 and 5, three groups, cos-latitude weights: (a) the predictions
    it returns are the crop of net(X) bit for bit; (b) every report field equals the notebook's expression evaluated in f64
    on those predictions and targets, de-normalised in f64 (1e-9 absolute for R2 and r, 1e-9 relative elsewhere), the
    per-group maps against the samples of that group."""
    from sklearn.metrics import r2_score
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from nasa_niswan_amd.inference import evaluate_skill
    ds = SyntheticE33OMA_CRNN("test", padding=(20, 28), sequence_length=4, n_steps=120, grid=(10, 18), levels=2, in_channels=8,
                              seed=0, device="cuda")
    assert len(ds) == 21
    torch.manual_seed(7)
    net = pkg.ConvLSTM(8, [16, 8], [3, 3], 2, out_channels=2, compute_dtype=dtype).cuda()
    halo, lat = (5, 5), np.linspace(-9, 9, 10)
    acc, preds = evaluate_skill(net, ds, batch_size=8, halo=halo, groups=lambda i: i % 3, lat=lat, return_predictions=True)
    assert acc.n_samples == 21 and acc.nslots == 3 and list(acc.counts.cpu().numpy()) == [7.0, 7.0, 7.0]
    # (a) against the model's own forward over the same batches
    net.eval()
    want, ys = [], []
    with torch.no_grad():
        for s in range(0, 21, 8):
            X, y = ds.device_batch(list(range(s, min(s + 8, 21))))
            want.append(net(X)[:, :, 5:15, 5:23])
            ys.append(y)
    want, yz = torch.cat(want), torch.cat(ys)
    assert preds.shape == (21, 2, 10, 18) and torch.equal(preds, want)
    # (b) the notebook's expressions on physical-unit arrays
    mu, sig = float(ds.y_mean), float(ds.y_std)
    G = yz.cpu().numpy().astype(np.float64) * sig + mu
    Pd = preds.cpu().numpy().astype(np.float64) * sig + mu
    N, O, Hc, Wc = G.shape
    assert np.all(np.sum((yz.cpu().numpy().astype(np.float64) - yz.cpu().numpy().astype(np.float64).mean(axis=0)) ** 2, axis=0) > 0)
    w = np.cos(np.deg2rad(lat))
    rep = acc.report(ds.y_mean, ds.y_std)
    r2t = np.array([r2_score(G[n].flatten(), Pd[n].flatten()) for n in range(N)])
    assert np.max(np.abs(rep.r2_temporal - r2t)) <= 1e-9
    r2to = np.array([[r2_score(G[n, o].flatten(), Pd[n, o].flatten()) for o in range(O)] for n in range(N)])
    assert np.max(np.abs(rep.r2_temporal_per_output - r2to)) <= 1e-9
    dz = preds.cpu().numpy().astype(np.float64) - yz.cpu().numpy().astype(np.float64)
    assert rel_close(rep.loss, (dz ** 2).mean(axis=(1, 2, 3)) + np.abs(dz).mean(axis=(1, 2, 3)))
    wm = lambda a: (a * w[None, None, :, None]).sum(axis=(2, 3)) / (w.sum() * Wc)
    assert rel_close(rep.global_mean_gt, wm(G)) and rel_close(rep.global_mean_pd, wm(Pd))
    assert abs(rep.r2 - r2_score(G.flatten(), Pd.flatten())) <= 1e-9

    Z = yz.cpu().numpy().astype(np.float64)
    Pz = preds.cpu().numpy().astype(np.float64)

    def maps(rp, members, all_finite=False):
        g, p = G[members], Pd[members]
        assert rp.count == len(members)
        # grid cells whose target is constant over the members (the tracer is clamped at zero, so a cell can be zero in all seven
        # windows of a group): z-score units decide, where n equal values sum and average exactly
        const = np.sum((Z[members] - Z[members].mean(axis=0)) ** 2, axis=0) == 0
        assert not (all_finite and const.any())
        print(f"    {int(const.sum())} constant-target cells")
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = np.stack([r_squared_spatial_notebook(g[:, o], p[:, o]) for o in range(O)])
        assert np.all(np.isfinite(r2[~const])) and np.max(np.abs(rp.r2_spatial - r2)[~const]) <= 1e-9
        r2s = np.array([[[r2_score(g[:, o, i, j], p[:, o, i, j]) for j in range(Wc)] for i in range(Hc)] for o in range(O)])
        assert np.max(np.abs(rp.r2_spatial - r2s)[~const]) <= 1e-9
        # at a constant target the notebook's vectorised cell divides by zero; the report follows sklearn's convention (in
        # physical units the equal values do not average exactly, so sklearn is asked in z-score units there: R2 is unit-free)
        for o, i, j in zip(*np.nonzero(const)):
            assert rp.r2_spatial[o, i, j] == r2_score(Z[members, o, i, j], Pz[members, o, i, j])
            assert np.isnan(rp.pearson[o, i, j])
        r = np.array([[[np.corrcoef(g[:, o, i, j], p[:, o, i, j])[0, 1] if not const[o, i, j] else np.nan
                        for j in range(Wc)] for i in range(Hc)] for o in range(O)])
        assert np.max(np.abs(rp.pearson - r)[~const]) <= 1e-9
        assert rel_close(rp.mean_gt, g.mean(axis=0)) and rel_close(rp.mean_pd, p.mean(axis=0))
        assert rel_close(rp.rmse, np.sqrt(((p - g) ** 2).mean(axis=0)))
        assert rel_close(rp.bias, (p - g).mean(axis=0))
    maps(rep, list(range(N)), all_finite=True)       # over all 21 windows the notebook's expression is finite everywhere
    for sl in range(3):
        maps(acc.report(ds.y_mean, ds.y_std, slots=[sl]), [n for n in range(N) if n % 3 == sl])
    maps(acc.report(ds.y_mean, ds.y_std, slots=[0, 2]), [n for n in range(N) if n % 3 != 1])
    # the plain entry on predictions that are already in memory: the same report
    acc2 = pkg.SkillAccumulator(O, Hc, Wc, nslots=3, lat=lat, device="cuda")
    with torch.no_grad():
        for s in range(0, 21, 8):
            idx = list(range(s, min(s + 8, 21)))
            X, y = ds.device_batch(idx)
            acc2.update_from_pred(net(X), y, halo, slots=[i % 3 for i in idx])
    assert torch.equal(acc2.pix, acc.pix) and torch.equal(torch.cat(acc2._rows), torch.cat(acc._rows))


def test_train_py_test_skill_writes_the_report(lib, tmp_path, monkeypatch, capsys):
    from nasa_niswan_amd import train as T
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--model", "LSTM-skill", "--in-channels", "4", "--hidden-channels", "8", "--kernel-size", "3", "--num-layers", "1",
            "--sequence-length", "4", "--input-size", "36", "36", "--grid", "32", "32", "--batch-size", "2", "--num-epochs", "1",
            "--learning-rate", "1e-4", "--synthetic-steps", "40", "--dtype", "f32", "--snapshot-dir", str(tmp_path / "s")]
    T.main(T.get_arguments(argv))
    assert not (tmp_path / "s" / "skill.npz").exists()                 # without the flag nothing changes
    capsys.readouterr()
    T.main(T.get_arguments(argv + ["--test-skill"]))
    out = capsys.readouterr().out
    z = np.load(tmp_path / "s" / "skill.npz")
    assert z["r2_temporal"].shape == (5,)                              # 40 steps: windows 32..36 are the test period
    assert z["r2_spatial"].shape == z["mean_pd"].shape == (1, 32, 32) and z["global_mean_gt"].shape == (5, 1)
    assert np.all(np.isfinite(z["r2_temporal"])) and np.all(np.isfinite(z["rmse"])) and "preds" not in z.files
    assert f"mean R2 per window {np.mean(z['r2_temporal']):.5f}" in out and f"mean R2 per grid cell {np.mean(z['r2_spatial']):.5f}" in out
