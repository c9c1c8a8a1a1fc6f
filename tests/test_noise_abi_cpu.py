"""CPU: the input noise's boundary -- nint_input_noise and nint_noise_normal are declared, exported and bound;
every refusal of include/nint.h returns its code before any HIP call (the convention of
tests/test_abi.py::test_entry_points_reject_bad_arguments_without_touching_the_gpu); InputNoise, ConvLSTM, FusedTrainer and
train.py refuse what they say they refuse, without a device."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4
A = 4096          # a made-up aligned address: every call below is refused before it is read


def test_entries_are_declared_exported_and_bound():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nint.h")).read(), flags=re.S)
    for name, nargs in (("nint_input_noise", 18), ("nint_noise_normal", 10)):
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)
        assert len(m.split(",")) == nargs
    assert "noise.hip" in open(os.path.join(ROOT, "nasa-niswan_amd", "build.py")).read()


def test_input_noise_refusals_without_touching_the_gpu():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 13, 37, 2) == 0
    gp = C.byref(g)

    def call(xs=A, x_n0=1, B=2, T=3, Cx=8, Cxp=16, c0=1, n=6, sigma=A, k=0, cyc=0, geom=gp, dt=0):
        return lib.nint_input_noise(xs, x_n0, B, T, Cx, Cxp, c0, n, sigma, k, cyc, 1, 2, 3, 4, geom, dt, None)

    # NULL pointers, counts
    for kw in (dict(xs=None), dict(sigma=None), dict(geom=None), dict(x_n0=-1), dict(B=0), dict(T=0), dict(n=0), dict(n=-1), dict(Cx=0)):
        assert call(**kw) == E_ARG, kw
    # the span
    for kw in (dict(c0=-1), dict(c0=3, n=6), dict(c0=0, n=9)):
        assert call(**kw) == E_ARG, kw
    # the fold
    for kw in (dict(k=-1), dict(k=2), dict(k=4, Cxp=32)):
        assert call(**kw) == E_ARG, kw
    # Cxp too small (plain, folded), or a pixel record that is no multiple of 16 bytes
    for kw in (dict(Cxp=4), dict(k=3, Cxp=16), dict(Cxp=18), dict(Cxp=12, dt=1, Cx=8), dict(Cxp=10, Cx=8, dt=0)):
        assert call(**kw) == E_ARG, kw
    # lon_cyclic
    for kw in (dict(cyc=2), dict(cyc=-1)):
        assert call(**kw) == E_ARG, kw
    narrow = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(narrow), 13, 1, 2) == 0
    assert call(cyc=1, geom=C.byref(narrow)) == E_ARG                            # W < P
    narrow.P, narrow.Hh, narrow.Wh = 0, 13, 1
    assert call(cyc=1, k=5, Cxp=48, geom=C.byref(narrow)) == E_ARG               # W < k/2
    # a bad dtype or geometry
    assert call(dt=2) == E_ARG and call(dt=-1) == E_ARG
    bad = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(bad), 13, 37, 2) == 0
    bad.Wh = 37
    assert call(geom=C.byref(bad)) == E_ARG
    # alignment: the slab 16 bytes, sigma 4 bytes -- after every argument check
    assert call(xs=A + 8) == E_ALIGN and call(sigma=A + 2) == E_ALIGN
    assert call(xs=A + 8, c0=-1) == E_ARG
    # the one bound: a fold no layer has
    assert call(k=4097, Cxp=4097 * 8 + 8) == E_SHAPE


def test_noise_normal_refusals_without_touching_the_gpu():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 13, 37, 2) == 0
    gp = C.byref(g)
    call = lambda out=A, B=2, T=3, n=5, geom=gp: lib.nint_noise_normal(out, B, T, n, 1, 2, 3, 4, geom, None)
    for kw in (dict(out=None), dict(geom=None), dict(B=0), dict(T=0), dict(n=0)):
        assert call(**kw) == E_ARG, kw
    assert call(out=A + 2) == E_ALIGN


def test_input_noise_object_refusals():
    from nasa_niswan_amd.engine import InputNoise
    for bad in (-0.1, float("nan"), float("inf"), (0.1, -1.0), (), "x"):
        with pytest.raises(ValueError, match="std"):
            InputNoise(bad)
    with pytest.raises(ValueError, match="channels"):
        InputNoise(0.1, channels=(1,))
    for name in ("seed", "draw", "step0", "lane0"):
        with pytest.raises(ValueError, match=name):
            InputNoise(0.1, **{name: -1})
    nz = InputNoise(0.5, seed=3)
    assert nz.active and not InputNoise(0.0).active and not InputNoise((0.0, 0.0)).active
    with pytest.raises(Exception):                      # frozen
        nz.seed = 4
    assert nz.span(9, 3) == (6, 3, (0.5, 0.5, 0.5))
    assert InputNoise((0.1, 0.2), channels=(1, 2)).span(4) == (1, 2, (0.1, 0.2))
    with pytest.raises(ValueError, match="feedback=True"):
        nz.span(9, None)
    with pytest.raises(ValueError, match="outside"):
        InputNoise(0.1, channels=(3, 2)).span(4)
    with pytest.raises(ValueError, match="std values"):
        InputNoise((0.1, 0.2, 0.3), channels=(1, 2)).span(4)


def test_module_refusals_come_before_any_device():
    """on CPU tensors: the input_noise refusals raise their own messages, before the module's 'no CPU path'"""
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.engine import InputNoise
    x = torch.zeros(1, 2, 4, 8, 8)
    plain = pkg.ConvLSTM(4, [8], [3], 1)
    with pytest.raises(ValueError, match="feedback=True"):
        plain(x, input_noise=InputNoise(0.1))
    with pytest.raises(ValueError, match="outside"):
        plain(x, input_noise=InputNoise(0.1, channels=(3, 2)))
    with pytest.raises(ValueError, match="InputNoise"):
        plain(x, input_noise=0.1)
    fb = pkg.ConvLSTM(4, [8], [3], 1, out_channels=2, feedback=True)
    with pytest.raises(RuntimeError, match="no CPU path"):          # a valid request gets as far as the device check
        fb(x, input_noise=InputNoise(0.1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        plain(x, input_noise=InputNoise(0.1, channels=(0, 4)))


def test_trainer_refusals_come_before_any_device():
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.trainer import FusedTrainer
    plain = pkg.ConvLSTM(4, [8], [3], 1)
    fb = pkg.ConvLSTM(4, [8], [3], 1, out_channels=2, feedback=True)
    with pytest.raises(ValueError, match="feedback=True"):
        FusedTrainer(plain, input_noise=0.1)
    with pytest.raises(ValueError, match="std"):
        FusedTrainer(fb, input_noise=-0.5)
    with pytest.raises(ValueError, match="std"):
        FusedTrainer(fb, input_noise=float("nan"))
    with pytest.raises(ValueError, match="outside"):
        FusedTrainer(plain, input_noise=0.1, noise_channels=(3, 2))
    with pytest.raises(ValueError, match="seed"):
        FusedTrainer(fb, input_noise=0.1, noise_seed=-1)
    with pytest.raises(Exception, match="MI355X"):                   # valid: it gets as far as asking for the device
        FusedTrainer(fb, input_noise=0.1)


def _train_args(*extra):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nint_train_cli", os.path.join(ROOT, "nasa-niswan_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.get_arguments(list(extra))


def test_train_cli_flags(capsys, tmp_path):
    import json
    base = ["--input-size", "20", "28", "--grid", "20", "28", "--snapshot-dir", str(tmp_path)]
    a = _train_args(*base, "--tracer-input", "--tracer-noise", "0.05", "--noise-seed", "7")
    assert a.tracer_noise == 0.05 and a.noise_seed == 7
    cfg = json.load(open(tmp_path / "configurations.json"))
    assert cfg["tracer_noise"] == 0.05 and cfg["noise_seed"] == 7
    a = _train_args(*base)
    assert a.tracer_noise is None and a.noise_seed == 0
    for extra, msg in ((["--tracer-noise", "0.05"], "needs --tracer-input"), (["--tracer-input", "--tracer-noise", "-1"], "finite standard deviation"),
                       (["--tracer-input", "--tracer-noise", "nan"], "finite standard deviation"), (["--noise-seed", "-2"], "noise-seed")):
        with pytest.raises(SystemExit):
            _train_args(*base, *extra)
        assert msg in capsys.readouterr().err, extra
