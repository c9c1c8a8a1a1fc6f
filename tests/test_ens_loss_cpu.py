"""Ensemble training without a device: the model of nint_ens_loss against brute force and finite differences, the
entry's refusals (they come before any HIP call), the scratch arithmetic and the trainer's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ensemble_model as EM
import ens_loss_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_ALIGN = -1, -4
A = 4096         # a "pointer" that is never followed: every call below is refused before a launch


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("M", [2, 3, 8])
def test_alpha_zero_and_one_are_the_plain_and_the_fair_crps(M):
    rng = np.random.default_rng(M)
    N, O, Hc, Wc = 3, 2, 4, 5
    x = rng.standard_normal((N, M, O, Hc, Wc)).astype(np.float32)
    t = rng.standard_normal((N, O, Hc, Wc)).astype(np.float32)
    flat = x.transpose(0, 2, 3, 4, 1).reshape(-1, M)
    ref = EM.brute_stats(flat, t.reshape(-1))
    for alpha, name in ((0.0, "crps"), (1.0, "crps_fair")):
        r = LM.run(x, t, alpha)
        assert r["cnt"] == N * O * Hc * Wc
        assert abs(r["loss"] - ref[name]) <= 1e-12 * max(1.0, abs(ref[name])), (alpha, r["loss"], ref[name])
    mid = LM.run(x, t, 0.5)["loss"]
    assert abs(mid - 0.5 * (ref["crps"] + ref["crps_fair"])) <= 1e-12
    # the statistics are the ensemble mean's: stats[0] / cnt is its MSE, ens_out[2] gives the spread
    r = LM.run(x, t, 1.0)
    assert abs((r["stats"][0] / r["cnt"]) ** 0.5 - ref["rmse_mean"]) <= 1e-12
    assert abs((r["ens"][2] / (M * M * (M - 1)) / r["cnt"]) ** 0.5 - ref["spread"]) <= 1e-12


@pytest.mark.parametrize("M,alpha", [(2, 1.0), (3, 0.5), (5, 0.0)])
def test_dpred_is_the_central_difference_of_the_loss(M, alpha):
    """data with every gap above 1e-2: members and target are distinct multiples of 1/32 plus a small offset, h = 1e-3"""
    rng = np.random.default_rng(10 + M)
    N, O, Hc, Wc = 2, 2, 3, 4
    ranks = np.stack([rng.permutation(M + 1) for _ in range(N * O * Hc * Wc)]).reshape(N, O, Hc, Wc, M + 1)
    vals = (ranks / 32.0 + rng.integers(-3, 4, (N, O, Hc, Wc, 1))).astype(np.float32)
    x = np.ascontiguousarray(np.moveaxis(vals[..., :M], -1, 1))
    t = np.ascontiguousarray(vals[..., M])
    wgt = (1.0 + rng.integers(0, 4, (Hc, Wc))).astype(np.float32) / 4
    ow = np.array([[1.0, 0.5], [0.25, 2.0]], np.float32)
    q, w, cnt = LM.weights(N, O, Hc, Wc, wgt, ow, [1, 0])
    g = LM.cells(x, t, alpha, q, w, cnt)["dpred"]
    h, x64 = 1e-3, x.astype(np.float64)
    for idx in [(0, 0, 0, 0, 0), (1, M - 1, 1, 2, 3), (0, 1, 1, 1, 2), (1, 0, 0, 2, 0)]:
        up, dn = x64.copy(), x64.copy()
        up[idx] += h
        dn[idx] -= h
        fd = (LM.loss_value(up, t, alpha, q, w, cnt) - LM.loss_value(dn, t, alpha, q, w, cnt)) / (2 * h)
        assert abs(fd - float(g[idx])) <= 1e-6 * abs(fd) + 1e-9, (idx, fd, g[idx])


def test_ties_have_sign_zero_and_zero_weights_skip():
    M, alpha = 3, 1.0
    x = np.zeros((1, M, 1, 1, 3), np.float32)
    t = np.zeros((1, 1, 1, 3), np.float32)
    x[0, :, 0, 0, 0] = (2.0, 2.0, 5.0)          # x_0 == x_1
    t[0, 0, 0, 0] = 5.0                         # x_2 == t
    x[0, :, 0, 0, 1] = (1.0, 1.0, 1.0)          # all equal, on the target
    t[0, 0, 0, 1] = 1.0
    x[0, :, 0, 0, 2] = (1.0, 2.0, 3.0)
    t[0, 0, 0, 2] = np.nan                      # under a zero weight: harmless
    wgt = np.array([[1.0, 1.0, 0.0]], np.float32)
    r = LM.run(x, t, alpha, wgt=wgt)
    cnt, kp = r["cnt"], LM.kp_of(M, alpha)
    assert cnt == 2.0
    g = r["dpred"][0, :, 0, 0]
    want0 = [(-1 / 3 - kp * -1) / cnt, (-1 / 3 - kp * -1) / cnt, (0.0 - kp * 2) / cnt]
    assert np.allclose(g[:, 0], want0, rtol=1e-7) and not np.signbit(g[:, 1]).any() and (g[:, 1] == 0).all()
    assert (g[:, 2] == 0).all() and not np.signbit(g[:, 2]).any() and np.isfinite(r["loss"]) and np.isfinite(r["stats"]).all()
    # a NaN member under a live weight: the cell's M gradients and the loss are NaN, no other cell's
    x[0, 1, 0, 0, 0] = np.nan
    r = LM.run(x, t, alpha, wgt=wgt)
    g = r["dpred"][0, :, 0, 0]
    assert np.isnan(g[:, 0]).all() and np.isfinite(g[:, 1:]).all() and np.isnan(r["loss"])


def test_integer_data_sums_are_exact():
    """what the GPU test leans on: with EM.int_data and dyadic weights the model's numpy totals equal the fractions"""
    rng = np.random.default_rng(3)
    N, M, O, Hc, Wc = 2, 3, 2, 4, 5
    _, x, y = EM.int_data(rng, N, M, O, Hc + 2, Wc + 2, 1, 1, Hc, Wc)
    wgt = np.broadcast_to(EM.dyadic_rows(Hc)[:, None], (Hc, Wc)).astype(np.float32)
    ow = np.array([[1.0, 0.0], [0.5, 2.0]], np.float32)
    r = LM.run(x, y, 0.5, wgt=wgt, ow=ow, ow_row=[1, 0])
    q, w, cnt = LM.weights(N, O, Hc, Wc, wgt, ow, [1, 0])
    vals, _, _, n_live = LM.exact_totals(x, y, q, w)
    assert n_live == 3 * Hc * Wc
    for k in (0, 1, 2, 5, 6):                               # SA, SD, SV, Sy, Syy: integers times dyadic weights
        assert float(vals[k]) == r["tot"][k], LM.TERMS[k]


def test_the_histogram_form_for_integer_data_has_the_loops_bits():
    rng = np.random.default_rng(4)
    for M in (2, 3, 8):
        _, x, y = EM.int_data(rng, 3, M, 2, 6, 7, 1, 1, 4, 5)
        a, b = LM.pairs(x, y), LM.pairs_int(x, y)
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (M, k)


def test_the_torch_crps_of_the_training_model_is_the_kernel_models_loss():
    """tests/ens_train_model.crps (what CPU autograd differentiates) against ens_loss_model.run, with step and output weights"""
    import ens_train_model as ETM
    rng = np.random.default_rng(6)
    N, M, T, O, H, W, halo, Hc, Wc = 2, 3, 4, 2, 7, 9, (1, 2), 5, 5
    seq = torch.from_numpy(rng.standard_normal((N * M, T * O, H, W)))
    y = torch.from_numpy(rng.standard_normal((N, T, O, Hc, Wc)).astype(np.float32)).double()
    step_w, out_w = [0.0, 0.5, 1.0, 2.0], [1.0, 0.25]
    got = float(ETM.crps(seq, y, M, 0.75, halo, True, O, step_w, out_w))
    x = seq.numpy().astype(np.float32).reshape(N, M, T, O, H, W)[..., 1:1 + Hc, 2:2 + Wc]
    x = np.stack([x[n, :, t] for n in range(N) for t in range(T)])
    ow = (np.asarray(step_w, np.float32)[:, None] * np.asarray(out_w, np.float32)[None]).astype(np.float32)
    r = LM.run(x, y.numpy().reshape(N * T, O, Hc, Wc), 0.75, ow=ow, ow_row=[t for _ in range(N) for t in range(T)])
    assert abs(got - r["loss"]) <= 1e-6 * abs(r["loss"]), (got, r["loss"])
    last = float(ETM.crps(seq, y[:, T - 1], M, 1.0, halo, False, O))
    r = LM.run(np.stack([seq.numpy().astype(np.float32).reshape(N, M, T, O, H, W)[n, :, T - 1, :, 1:1 + Hc, 2:2 + Wc] for n in range(N)]),
               y[:, T - 1].numpy(), 1.0)
    assert abs(last - r["loss"]) <= 1e-6 * abs(r["loss"])


# ------------------------------------------------------------------ the boundary
def test_entry_is_declared_exported_and_bound():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nint.h")).read(), flags=re.S)
    for name, nargs in (("nint_ens_loss_scratch_bytes", 5), ("nint_ens_loss", 25)):
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", src), name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
        assert len(re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1).split(",")) == nargs
    assert re.search(r"#define\s+NINT_ENS_LOSS_OUT\s+4\b", src) and _lib.NINT_ENS_LOSS_OUT == 4
    S = _lib.NintEnsLossSpec
    assert (C.sizeof(S), S.alpha.offset, S.cnt.offset, S.ow.offset, S.ow_row.offset, S.nrows.offset) == (40, 0, 8, 16, 24, 32)
    assert re.search(r"typedef struct nint_ens_loss_spec \{\s*double alpha;\s*double cnt;\s*const float\* ow;\s*const int32_t\* ow_row;"
                     r"\s*int32_t nrows;\s*\} nint_ens_loss_spec;", src)


def test_scratch_query_is_host_arithmetic():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    # the workgroups' partial rows of one piece (256-pixel blocks of the FULL image), then a row per (sample, output) of the call
    assert lib.nint_ens_loss_scratch_bytes(3, 8, 5, 15, 41) == (3 * 5 * 3 + 3 * 5) * 8 * 8
    assert lib.nint_ens_loss_scratch_bytes(70, 2, 5, 15, 41) == (64 * 5 * 3 + 70 * 5) * 8 * 8
    assert lib.nint_ens_loss_scratch_bytes(1, 2, 1, 1, 1) == 2 * 8 * 8
    assert lib.nint_ens_loss_scratch_bytes(0, 2, 1, 3, 5) == 0 and lib.nint_ens_loss_scratch_bytes(3, 8, 5, 0, 37) == 0


def test_ens_loss_refusals_without_touching_the_gpu():
    from nasa_niswan_amd import _lib
    lib = _lib.load()

    def call(pred=A, poff=(0, 100, 50), pstride=1000, dpred=A, doff=(0, 7, 9), dstride=500, M=4, y=A, wgt=None, wsum=0.0, spec=True,
             alpha=1.0, cnt=10.0, ow=None, ow_row=None, nrows=0, loss=A, stats=A, ens=A, scratch=A, nb=None, N=3, O=5, H=15, W=41,
             oy=1, ox=2, Hc=13, Wc=37):
        po = None if poff is None else (C.c_int64 * len(poff))(*poff)
        do = None if doff is None else (C.c_int64 * len(doff))(*doff)
        sp = _lib.NintEnsLossSpec()
        sp.alpha, sp.cnt, sp.ow, sp.nrows = alpha, cnt, ow, nrows
        rows = None if ow_row is None else (C.c_int32 * len(ow_row))(*ow_row)
        sp.ow_row = rows
        nb = lib.nint_ens_loss_scratch_bytes(N, M, O, H, W) if nb is None else nb
        return lib.nint_ens_loss(pred, po, pstride, dpred, do, dstride, M, y, wgt, wsum, C.byref(sp) if spec else None, loss, stats,
                                 ens, scratch, nb, N, O, H, W, oy, ox, Hc, Wc, None)

    for kw in (dict(pred=None), dict(poff=None), dict(dpred=None), dict(doff=None), dict(y=None), dict(spec=False), dict(loss=None),
               dict(stats=None), dict(ens=None), dict(scratch=None)):
        assert call(**kw) == E_ARG, kw
    inf, nan = float("inf"), float("nan")
    for kw in (dict(M=1), dict(M=0), dict(M=65), dict(N=0), dict(O=0), dict(poff=(0, -1, 5)), dict(doff=(0, 1, -5)), dict(pstride=-1),
               dict(dstride=-1), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan), dict(alpha=inf), dict(cnt=0.0), dict(cnt=-1.0),
               dict(cnt=nan), dict(cnt=inf), dict(wgt=A, wsum=0.0), dict(wgt=A, wsum=nan), dict(wgt=A, wsum=inf),
               dict(ow_row=(0, 0, 0)), dict(nrows=2), dict(ow=A, nrows=0), dict(ow=A, nrows=2, ow_row=(0, 2, 1)),
               dict(ow=A, nrows=2, ow_row=(0, -1, 1)), dict(oy=3), dict(ox=5), dict(oy=-1), dict(ox=-1), dict(Hc=0), dict(Wc=0),
               dict(Hc=16, oy=0), dict(nb=8)):
        assert call(**kw) == E_ARG, kw
    assert call(nb=lib.nint_ens_loss_scratch_bytes(3, 4, 5, 15, 41) - 8) == E_ARG
    # alignment, after every argument check: the f64 buffers 8 bytes, the f32 buffers 4
    for kw in (dict(stats=A + 4), dict(ens=A + 4), dict(scratch=A + 4), dict(pred=A + 2), dict(dpred=A + 2), dict(y=A + 2),
               dict(wgt=A + 2, wsum=3.0), dict(ow=A + 2, nrows=1), dict(loss=A + 2)):
        assert call(**kw) == E_ALIGN, kw
    assert call(stats=A + 4, M=1) == E_ARG and call(pred=A + 2, cnt=0.0) == E_ARG


# ------------------------------------------------------------------ the host layers, without a device
def test_ensemble_loss_validates_on_the_host():
    from nasa_niswan_amd.loss import EnsembleLoss
    for bad in (-0.1, 1.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            EnsembleLoss(alpha=bad)
    with pytest.raises(ValueError, match="output weights"):
        EnsembleLoss(output_weights=[1.0, -1.0])
    with pytest.raises(ValueError, match="all zero"):
        EnsembleLoss(step_weights=[0.0, 0.0])
    e = EnsembleLoss(0.5, output_weights=[1.0, 0.5], step_weights=[0.0, 1.0, 0.25])
    tab = e.host_table(2, 3)
    assert tab.dtype == np.float32 and tab.tolist() == [[0.0, 0.0], [1.0, 0.5], [0.25, 0.125]]
    assert EnsembleLoss().host_table(2, 3) is None and EnsembleLoss(output_weights=[2.0, 1.0]).host_table(2).tolist() == [[2.0, 1.0]]
    with pytest.raises(ValueError, match="output weights for"):
        e.host_table(3, 3)
    with pytest.raises(ValueError, match="step_weights need"):
        e.host_table(2)


def test_trainer_refusals_come_before_any_device():
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.loss import EnsembleLoss, LossSpec
    from nasa_niswan_amd.trainer import FusedTrainer
    fb = pkg.ConvLSTM(4, [8], [3], 1, out_channels=2, feedback=True)
    ok = dict(rollout_from=2, ensemble_members=4, feedback_noise=0.1)
    with pytest.raises(ValueError, match="needs rollout_from"):
        FusedTrainer(fb, ensemble_members=4, feedback_noise=0.1)
    for m in (1, 65, 0, 2.5, True):
        with pytest.raises(ValueError, match=r"\[2, 64\]"):
            FusedTrainer(fb, **{**ok, "ensemble_members": m})
    for kw in (dict(feedback_noise=None), dict(feedback_noise=0.0), dict(feedback_noise=0.0, input_noise=0.0)):
        with pytest.raises(ValueError, match="identical"):
            FusedTrainer(fb, **{**ok, **kw})
    with pytest.raises(ValueError, match="LossSpec"):
        FusedTrainer(fb, loss=LossSpec(0, 1, 0), **ok)
    with pytest.raises(ValueError, match="sampling_prob"):
        FusedTrainer(fb, sampling_prob=0.5, **ok)
    with pytest.raises(ValueError, match="step_weights need"):
        FusedTrainer(fb, ensemble_loss=EnsembleLoss(step_weights=[1.0, 1.0]), **ok)
    with pytest.raises(TypeError, match="EnsembleLoss"):
        FusedTrainer(fb, ensemble_loss=LossSpec(), **ok)
    for kw in (dict(feedback_noise=-1.0), dict(feedback_noise=float("nan")), dict(feedback_noise=(0.1, 0.2, 0.3))):
        with pytest.raises(ValueError, match="std"):
            FusedTrainer(fb, **{**ok, **kw})
    for kw in (dict(feedback_noise=0.1), dict(ensemble_loss=EnsembleLoss())):
        with pytest.raises(ValueError, match="need ensemble_members"):
            FusedTrainer(fb, rollout_from=2, **kw)
    # valid requests get as far as the device check -- input noise alone, feedback noise alone, one value per output
    for kw in (dict(), dict(feedback_noise=None, input_noise=0.05), dict(feedback_noise=(0.1, 0.0)),
               dict(ensemble_loss=EnsembleLoss(0.9, output_weights=[1.0, 2.0])),
               dict(sequence_loss=True, ensemble_loss=EnsembleLoss(step_weights=[0.0, 1.0, 1.0]))):
        with pytest.raises(pkg.NintError, match="MI355X"):
            FusedTrainer(fb, **{**ok, **kw})
    # the autograd route keeps its refusal
    from nasa_niswan_amd.engine import InputNoise
    with pytest.raises(ValueError, match="feedback_grad"):
        fb(torch.zeros(1, 3, 4, 8, 8), free_from=1, feedback_grad=True, feedback_noise=InputNoise(0.1))


def _train_args(*extra):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nint_train_cli", os.path.join(ROOT, "nasa-niswan_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.get_arguments(list(extra))


def test_train_cli_flags(capsys, tmp_path):
    from nasa_niswan_amd.loss import EnsembleLoss
    base = ["--input-size", "20", "28", "--grid", "20", "28", "--snapshot-dir", str(tmp_path), "--tracer-input", "--sequence-length", "4"]
    mod, a = _train_args(*base, "--rollout-from", "2", "--train-ensemble", "4")
    assert (a.train_ensemble, a.train_feedback_noise, a.crps_alpha) == (4, 0.05, 0.95)
    spec = mod.build_loss_spec(a)
    assert isinstance(spec, EnsembleLoss) and spec.alpha == 0.95 and spec.step_weights is None
    mod, a = _train_args(*base, "--rollout-from", "2", "--train-ensemble", "2", "--tracer-noise", "0.1", "--crps-alpha", "1", "--sequence-loss",
                         "--spinup-steps", "2")
    assert (a.train_feedback_noise, a.crps_alpha) == (0.0, 1.0)
    assert mod.build_loss_spec(a).step_weights.tolist() == [0.0, 0.0, 1.0, 1.0]
    _, a = _train_args(*base, "--rollout-from", "2")
    assert a.train_ensemble is None and mod.build_loss_spec(a) is None
    for extra, msg in ((["--train-ensemble", "4"], "needs --rollout-from"), (["--rollout-from", "2", "--crps-alpha", "0.5"], "needs --train-ensemble"),
                       (["--rollout-from", "2", "--train-feedback-noise", "0.1"], "needs --train-ensemble"),
                       (["--rollout-from", "2", "--train-ensemble", "1"], "[2, 64]"), (["--rollout-from", "2", "--train-ensemble", "65"], "[2, 64]"),
                       (["--rollout-from", "2", "--train-ensemble", "4", "--sampling-prob", "0.5"], "--sampling-prob"),
                       (["--rollout-from", "2", "--train-ensemble", "4", "--loss-mix", "0", "1", "0"], "--loss-mix"),
                       (["--rollout-from", "2", "--train-ensemble", "4", "--train-feedback-noise", "-1"], "finite standard deviation"),
                       (["--rollout-from", "2", "--train-ensemble", "4", "--train-feedback-noise", "0"], "identical"),
                       (["--rollout-from", "2", "--train-ensemble", "4", "--crps-alpha", "1.5"], "[0, 1]")):
        with pytest.raises(SystemExit):
            _train_args(*base, *extra)
        assert msg in capsys.readouterr().err, extra
