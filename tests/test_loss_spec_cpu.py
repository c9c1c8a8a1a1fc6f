"""CPU tests of the configurable loss (MSE / L1 / Huber mix, output and step weights): the host model of
tests/loss_spec_model.py against torch's own criteria and autograd in f64, the conditions its case builder asserts for the
seeds the GPU tests use, ``loss.LossSpec``'s validation, the ``_spec`` entries' argument checks (made before any launch, so
they run without a GPU), the layout of ``nint_loss_spec`` against gcc, and ``train.py``'s loss flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_spec_model as LM
import weighted_loss_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


# =========================================================================== the model against torch in f64
def exact_case(rng, N, O, H, W, oy, ox, Hc, Wc):
    """pred and y on a grid of 2^-10 in [-2, 2): their f32 difference is exact, so an f64 expression sees the model's d"""
    pred = (rng.integers(-2048, 2048, (N, O, H, W)) / 1024.0).astype(f32)
    y = (rng.integers(-2048, 2048, (N, O, Hc, Wc)) / 1024.0).astype(f32)
    return pred, y


@pytest.mark.parametrize("with_ow,steps", [(False, 0), (True, 0), (True, 3)], ids=["no-ow", "ow", "steps-x-outputs"])
@pytest.mark.parametrize("with_map", [False, True], ids=["no-map", "map"])
@pytest.mark.parametrize("mix", ["mse", "l1", "huber", "mix"])
def test_model_against_torch_criteria_and_autograd_in_f64(mix, with_map, with_ow, steps):
    """loss = a MSELoss + b L1Loss + c HuberLoss(delta) with reduction='none', the weights applied by hand and the weighted sum
    divided by the weights' total; gradient by autograd.  1e-12 relative: f64 sums of ~1e3 terms in two orders."""
    N, O, H, W, oy, ox, Hc, Wc = (2, 6, 12, 20, 1, 2, 10, 16)
    rng = np.random.default_rng(5)
    pred, y = exact_case(rng, N, O, H, W, oy, ox, Hc, Wc)
    w = WM.wmap(Hc, Wc) if with_map else None
    ow = None
    if with_ow:
        ow = LM.seq_weights(LM.STEP_W, LM.output_weights(O // 3)) if steps else LM.output_weights(O)
    sp = LM.Spec(*LM.MIXES[mix], delta=LM.DELTA, ow=ow)
    ref = LM.loss(pred, y, w, sp, oy, ox)
    pt = torch.from_numpy(pred).double().requires_grad_(True)
    yt = torch.from_numpy(y).double()
    pc = pt[:, :, oy:oy + Hc, ox:ox + Wc]
    Wt = torch.from_numpy(LM.weights_of(sp, w, O, Hc, Wc))[None].expand_as(yt)
    total = Wt.sum()
    terms = [torch.nn.MSELoss(reduction="none"), torch.nn.L1Loss(reduction="none"), torch.nn.HuberLoss(reduction="none", delta=sp.delta)]
    want = sum(co * (Wt * crit(pc, yt)).sum() / total for co, crit in zip((sp.a, sp.b, sp.c), terms) if co != 0)
    want.backward()
    want = want.detach()
    assert abs(ref["loss"] - float(want)) <= 1e-12 * abs(float(want))
    assert abs(LM.cnt_of(N, O, sp, w, Hc, Wc) - float(total)) <= 1e-12 * float(total)
    g = pt.grad.numpy()
    scale = np.abs(g).max()
    assert np.abs(ref["dpred64"] - g).max() <= 1e-12 * scale
    assert np.array_equal(ref["dpred"], ref["dpred64"].astype(f32))
    # the torch twin of the model (what the oracle fit loop minimises) is the same number, with the same gradient
    p2 = torch.from_numpy(pred).double().requires_grad_(True)
    lt = LM.loss_torch(p2, yt, w, sp, oy, ox)
    lt.backward()
    assert abs(float(lt.detach()) - float(want)) <= 1e-12 * abs(float(want)) and (p2.grad - pt.grad).abs().max() <= 1e-12 * scale
    # and the f64 fused twin on a head that is the identity reproduces it
    if not steps:
        h = np.zeros((N, H, W, O)); h[...] = np.moveaxis(pred.astype(np.float64), 1, -1)
        dp, dh, lf = LM.head_loss_fused(h, np.eye(O), None, y, w, sp, oy, ox)
        assert abs(lf - float(want)) <= 1e-12 * abs(float(want)) and np.abs(dp - g).max() <= 1e-12 * scale
        assert np.abs(np.moveaxis(dh, -1, 1) - g).max() <= 1e-12 * scale


def test_a_zero_coefficient_takes_its_term_out_and_nan_survives_the_clamp():
    sp = LM.Spec(0.0, 1.0, 0.0)
    assert LM.mix(sp, np.inf, 2.0, np.nan) == 2.0                  # neither 0 * inf nor 0 * NaN
    assert np.isnan(LM.clamp(np.array([np.nan]), 0.75))[0] and LM.clamp(np.array([np.inf, -np.inf]), 0.75).tolist() == [0.75, -0.75]
    assert LM.sgn(np.array([np.nan, 0.0, -0.0, 2.0, -3.0])).tolist() == [0, 0, 0, 1, -1]
    assert LM.huber(np.array([0.75, 0.75 + 2.0 ** -24, np.inf]), 0.75).tolist() == [0.28125, 0.75 * (0.75 + 2.0 ** -24 - 0.375), np.inf]


@pytest.mark.parametrize("shape,mix,with_map,with_ow,steps", LM.plain_cases())
def test_case_builder_conditions_hold_for_the_gpu_tests_seeds(shape, mix, with_map, with_ow, steps):
    """build_case asserts its three conditions itself; here they are seen to hold for every case the GPU tests build"""
    case = LM.build_case(shape, LM.SEED, with_map, with_ow, mix, steps=steps)
    sp, (N, O, H, W, oy, ox, Hc, Wc) = case["spec"], shape
    assert set(case["where"]) == {"plus", "minus", "zero", "above"}
    if with_ow:
        assert 2 * int((sp.ow > 0).sum()) >= (sp.ow.size if not steps else sp.ow.size // 2)
        assert (sp.ow == 0).any() == (O > 1)
    ref = LM.loss(case["pred"], case["y"], case["w"], sp, oy, ox)
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["dpred"]).all()
    Wd = LM.weights_of(sp, case["w"], O, Hc, Wc)
    dead = np.ones((O, H, W), bool)
    dead[:, oy:oy + Hc, ox:ox + Wc] = Wd == 0
    assert not ref["dpred"].view(np.uint32)[:, dead].any()


# =========================================================================== LossSpec
def test_loss_spec_validation():
    from nasa_niswan_amd.loss import LossSpec
    LossSpec()
    LossSpec(0, 0, 1, delta=0.5)
    LossSpec(1, 0, 0, delta=float("nan"))                           # delta is not read while huber is off
    for bad in (dict(mse=-1.0), dict(l1=float("nan")), dict(huber=float("inf")), dict(mse=0, l1=0, huber=0),
                dict(huber=1.0, delta=0.0), dict(huber=1.0, delta=-1.0), dict(huber=1.0, delta=float("inf")),
                dict(huber=1.0, delta=float("nan")), dict(output_weights=[1.0, -0.5]), dict(output_weights=[1.0, float("nan")]),
                dict(output_weights=[float("inf")]), dict(output_weights=[0.0, 0.0]), dict(step_weights=[0.0]),
                dict(step_weights=[-1.0, 1.0]), dict(step_weights=[[1.0, 1.0]]), dict(output_weights=[1e39])):
        with pytest.raises(ValueError):
            LossSpec(**bad)
    sp = LossSpec(output_weights=[1.0, 0.0, 2.5], step_weights=[0.0, 0.3])
    with pytest.raises(ValueError):
        sp.host_vector(3)                                           # step weights need the sequence loss
    with pytest.raises(ValueError):
        sp.host_vector(4, 2)                                        # lengths: against O ...
    with pytest.raises(ValueError):
        sp.host_vector(3, 3)                                        # ... and T, at the first call that knows them
    vec = sp.host_vector(3, 2)
    assert vec.dtype == f32 and np.array_equal(vec, (np.array([0.0, 0.3], f32)[:, None] * np.array([1.0, 0.0, 2.5], f32)[None]).reshape(-1))
    assert np.array_equal(vec, LM.seq_weights([0.0, 0.3], [1.0, 0.0, 2.5]))
    assert LossSpec().host_vector(3) is None and LossSpec().host_vector(3, 2) is None
    assert np.array_equal(LossSpec(step_weights=[0, 1]).host_vector(2, 2), np.array([0, 0, 1, 1], f32))
    assert np.array_equal(LossSpec(output_weights=[0.1, 0]).host_vector(2), np.array([0.1, 0], f32))


def test_trainer_refuses_step_weights_without_the_sequence_loss_before_touching_a_device():
    from nasa_niswan_amd.loss import CropLoss, LossSpec
    from nasa_niswan_amd.trainer import FusedTrainer
    tr = FusedTrainer.__new__(FusedTrainer)
    tr.sequence_loss = False
    with pytest.raises(ValueError, match="sequence_loss"):
        tr.set_loss(LossSpec(step_weights=[0.0, 1.0]))
    with pytest.raises(TypeError):
        tr.set_loss((1.0, 1.0, 0.0))
    tr.set_loss(None)
    assert tr._spec is None
    tr.sequence_loss = True
    tr.set_loss(LossSpec(step_weights=[0.0, 1.0]))
    with pytest.raises(TypeError):
        CropLoss(spec=(1, 1, 0))


# =========================================================================== the C ABI
def test_loss_spec_struct_layout_matches_header(tmp_path):
    from nasa_niswan_amd import _lib
    prog = tmp_path / "sz.c"
    fields = ["mse", "l1", "huber", "delta", "ow", "now", "osum"]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nint.h"\nint main(){printf("%zu %d' + " %zu" * len(fields) +
                    '\\n",sizeof(nint_loss_spec),NINT_LOSS_SPEC_SCRATCH_FLOATS,' +
                    ",".join(f"offsetof(nint_loss_spec,{f})" for f in fields) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_lib.NintLossSpec), _lib.NINT_LOSS_SPEC_SCRATCH_FLOATS] + [getattr(_lib.NintLossSpec, f).offset for f in fields]
    assert got == want
    assert _lib.NINT_LOSS_SPEC_SCRATCH_FLOATS == 2 + 2 * 5 * ((_lib.NINT_LOSS_SCRATCH_FLOATS - 2) // 8)   # five doubles per workgroup
    assert _lib.NINT_LOSS_SCRATCH_FLOATS == 8194


def spec_c(mse=1.0, l1=1.0, huber=0.0, delta=1.0, ow=None, now=0, osum=0.0):
    from nasa_niswan_amd import _lib
    s = _lib.NintLossSpec()
    s.mse, s.l1, s.huber, s.delta, s.ow, s.now, s.osum = mse, l1, huber, delta, ow, now, osum
    return s


BAD_SPECS = [dict(mse=-1.0), dict(l1=float("nan")), dict(huber=float("inf")), dict(mse=0.0, l1=0.0, huber=0.0),
             dict(huber=1.0, delta=0.0), dict(huber=1.0, delta=float("nan")), dict(huber=1.0, delta=float("inf")),
             dict(ow=16, now=5, osum=3.0), dict(ow=16, now=0, osum=3.0), dict(ow=16, now=3, osum=0.0),
             dict(ow=16, now=3, osum=float("nan")), dict(ow=16, now=3, osum=float("inf")), dict(ow=None, now=3, osum=3.0)]


def test_spec_entries_reject_bad_arguments_without_touching_the_gpu():
    """Every check of the _spec entries is made before any HIP call: NINT_E_ARG for the twins' argument checks, a NULL or
    invalid spec and a bad map total; NINT_E_ALIGN for misaligned loss_out, map and ow; NINT_E_SHAPE where the fused twins
    return it.  (Pointers are small integers: never dereferenced on these paths.)"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 12, 20, 1) == 0
    ok = spec_c()
    okw = spec_c(ow=16, now=3, osum=3.5)
    okw6 = spec_c(ow=16, now=6, osum=3.5)

    def plain(spec, pred=16, y=16, wgt=None, wsum=0.0, loss_out=16, N=2, O=3, H=12, W=20, oy=1, ox=2, Hc=10, Wc=16):
        return lib.nint_loss_crop_spec(pred, y, wgt, wsum, None if spec is None else C.byref(spec), None, loss_out, None,
                                       N, O, H, W, oy, ox, Hc, Wc, None)

    def fused(spec, h=16, wgt=None, wsum=0.0, loss_out=16, Chp=16, O=3, oy=1, Hc=10, dt=0, dpred=16):
        return lib.nint_head_loss_fused_spec(h, 0, 2, 8, Chp, O, 16, None, 16, wgt, wsum, None if spec is None else C.byref(spec),
                                             dpred, 16, loss_out, None, C.byref(g), oy, 2, Hc, 16, dt, None)

    def seq(spec, h=16, wgt=None, wsum=0.0, loss_out=16, Chp=16, O=3, oy=1, Hc=10, dt=0, dh=16):
        return lib.nint_head_loss_seq_fused_spec(h, 2, 2, 8, Chp, O, 16, None, 16, wgt, wsum, None if spec is None else C.byref(spec),
                                                 16, dh, loss_out, None, C.byref(g), oy, 2, Hc, 16, dt, None)

    for call, good in ((plain, okw), (fused, okw), (seq, okw6)):
        assert call(None) == E_ARG                                  # a NULL spec
        for bad in BAD_SPECS:
            assert call(spec_c(**bad)) == E_ARG, (call.__name__, bad)
        assert call(good, wgt=16, wsum=0.0) == E_ARG and call(good, wgt=16, wsum=float("nan")) == E_ARG
        assert call(good, wgt=16, wsum=float("inf")) == E_ARG and call(ok, wgt=16, wsum=-1.0) == E_ARG
        assert call(ok, loss_out=20) == E_ALIGN and call(ok, wgt=18, wsum=5.0) == E_ALIGN
        assert call(spec_c(ow=18, now=good.now, osum=3.5)) == E_ALIGN
        assert call(ok, oy=5) == E_ARG and call(ok, Hc=0) == E_ARG  # the crop outside the grid, an empty crop
    assert plain(okw6) == E_ARG and plain(ok, pred=None) == E_ARG and plain(ok, N=0) == E_ARG    # now is O for the plain entry ...
    assert fused(okw6) == E_ARG and seq(okw) == E_ARG               # ... and the fused one, T*O for the sequence entry
    assert fused(ok, dt=7) == E_ARG and seq(ok, dt=7) == E_ARG and fused(ok, dpred=None) == E_ARG and seq(ok, dh=None) == E_ARG
    # NINT_E_SHAPE exactly where the twins return it: more than 128 padded channels; the weight image beyond the LDS
    assert fused(ok, Chp=144) == E_SHAPE and seq(ok, Chp=144) == E_SHAPE
    assert lib.nint_head_loss_fused(16, 0, 2, 8, 144, 3, 16, None, 16, 16, 16, 16, None, C.byref(g), 1, 2, 10, 16, 0, None) == E_SHAPE
    assert fused(spec_c(), O=1200) == E_SHAPE and seq(spec_c(), O=1200) == E_SHAPE
    assert lib.nint_head_loss_fused(16, 0, 2, 8, 16, 1200, 16, None, 16, 16, 16, 16, None, C.byref(g), 1, 2, 10, 16, 0, None) == E_SHAPE
    assert fused(spec_c(mse=-1.0), Chp=144) == E_ARG                # the argument checks come first
    assert seq(ok, h=24) == E_ALIGN and seq(ok, dh=24) == E_ALIGN   # the twin's 16-byte slab alignment


# =========================================================================== train.py
def train_mod():
    sys.path.insert(0, os.path.join(ROOT, "nasa-niswan_amd"))
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location("nint_train_cli", os.path.join(ROOT, "nasa-niswan_amd", "train.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path.pop(0)


def test_train_py_loss_flags(tmp_path, monkeypatch):
    import json
    monkeypatch.delenv("RANK", raising=False)
    T = train_mod()
    base = ["--snapshot-dir", str(tmp_path), "--sequence-length", "4", "--levels", "3"]
    for bad in (["--spinup-steps", "1"], ["--sequence-loss", "--spinup-steps", "4"], ["--sequence-loss", "--spinup-steps", "9"],
                ["--sequence-loss", "--spinup-steps", "-1"]):
        with pytest.raises(SystemExit):
            T.get_arguments(base + bad)
    args = T.get_arguments(base)
    assert tuple(args.loss_mix) == (1.0, 1.0, 0.0) and args.huber_delta == 1.0 and args.output_weights is None and args.spinup_steps == 0
    assert T.build_loss_spec(args) is None                          # no loss flag: the trainer receives loss=None ...
    assert T.build_loss_spec(T.get_arguments(base + ["--huber-delta", "0.5"])) is None    # (a threshold without a Huber term)
    import inspect
    assert "loss=build_loss_spec(args)" in inspect.getsource(T.main)                       # ... through this one call
    np.save(tmp_path / "ow.npy", np.array([1.0, 0.0, 2.0]))
    args = T.get_arguments(base + ["--loss-mix", "0", "0.5", "2", "--huber-delta", "0.5", "--output-weights", str(tmp_path / "ow.npy"),
                                   "--sequence-loss", "--spinup-steps", "1"])
    sp = T.build_loss_spec(args)
    assert (sp.mse, sp.l1, sp.huber, sp.delta) == (0.0, 0.5, 2.0, 0.5)
    assert sp.output_weights.tolist() == [1.0, 0.0, 2.0] and sp.step_weights.tolist() == [0.0, 1.0, 1.0, 1.0]
    cfg = json.load(open(tmp_path / "configurations.json"))
    assert cfg["loss_mix"] == [0.0, 0.5, 2.0] and cfg["huber_delta"] == 0.5 and cfg["spinup_steps"] == 1
    assert cfg["output_weights"] == str(tmp_path / "ow.npy")
    assert T.build_loss_spec(T.get_arguments(base + ["--sequence-loss", "--spinup-steps", "3"])).step_weights.tolist() == [0, 0, 0, 1]
    with pytest.raises(SystemExit):
        T.build_loss_spec(T.get_arguments(base + ["--loss-mix", "0", "0", "0"]))
    np.save(tmp_path / "ow2.npy", np.ones(2))
    with pytest.raises(SystemExit):
        T.build_loss_spec(T.get_arguments(base + ["--output-weights", str(tmp_path / "ow2.npy")]))
