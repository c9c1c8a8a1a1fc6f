"""Cyclic longitude (nint_seq.lon_cyclic) without a GPU: the CPU model the GPU tests compare against
(tests/cyclic_model.py), the host surface of the flag, and the launch plan -- nint_debug_seq_plan runs the drivers' own planner
on the host, and the wrap launches show in it as the enqueue indices its conv / pointwise records skip."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cyclic_model as CM
import test_launch_plan_cpu as TLP

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _small3():
    from oracle import convlstm_oracle as O
    g = np.load(os.path.join(GOLD, "small3_train.npz"), allow_pickle=False)
    hidden, ks = [int(v) for v in g["hidden"]], [int(v) for v in g["ks"]]
    params = O.synth_params(int(g["C"]), hidden, ks, len(hidden), seed=int(g["seed"]))
    X, y = O.synth_batch(int(g["B"]), int(g["T"]), int(g["C"]), int(g["Hp"]), int(g["Wp"]), tuple(int(v) for v in g["grid"]),
                         seed=int(g["seed"]))
    return g, params, X, y


def test_model_without_wrapping_is_the_oracle():
    """wrapping off: the helper is oracle/convlstm_oracle (bit for bit: the same torch ops) and reproduces the golden vectors
    of the reference's own model.py -- prediction, loss and every gradient of tests/golden/small3_train.npz"""
    from oracle import convlstm_oracle as O
    g, params, X, y = _small3()
    leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = CM.forward(X, leaf, cyclic=False)
    assert torch.equal(out, O.convlstm_forward(X, params))
    np.testing.assert_allclose(out.detach().numpy(), g["pred_full"], rtol=1e-5, atol=1e-6)
    hy, hx = (int(v) for v in g["halo"])
    pred = out[:, :, hy:hy + y.shape[-2], hx:hx + y.shape[-1]].squeeze()
    loss = O.loss_mse_l1(y, pred)
    assert abs(float(loss.detach()) - float(g["loss1"])) < 1e-6
    loss.backward()
    for k, v in leaf.items():
        ref = g["grad." + k]
        assert float(np.abs(v.grad.numpy() - ref).max()) <= 1e-5 * float(np.abs(ref).max()) + 1e-8, k
    pred2, seq, hs, cs = CM.forward(X, params, cyclic=False, return_sequence=True, return_states=True)
    opred, oseq, ohs, ocs = O.convlstm_forward(X, params, return_sequence=True, return_states=True)
    assert torch.equal(seq, oseq) and all(torch.equal(a, b) for a, b in zip(hs + cs, ohs + ocs))


@pytest.mark.parametrize("case", ["A", "C"])
def test_model_with_wrapping_is_roll_equivariant(case):
    """net(roll(x, s, W)) == roll(net(x), s, W) in f64, states included -- and the zero-padded model is not"""
    from oracle import convlstm_oracle as O
    c = CM.CASES[case]
    params = O.synth_params(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=2, seed=3, dtype=torch.float64)
    rng = np.random.default_rng(5)
    X = torch.from_numpy(rng.standard_normal((c["B"], c["T"], c["C"], c["H"], c["W"])))
    for s in (1, 7, c["W"] - 2):
        a = CM.forward(torch.roll(X, s, -1), params, return_sequence=True, return_states=True)
        b = CM.forward(X, params, return_sequence=True, return_states=True)
        flat = lambda r: [r[0], r[1]] + list(r[2]) + list(r[3])
        for u, v in zip(flat(a), flat(b)):
            assert float((u - torch.roll(v, s, -1)).abs().max()) <= 1e-12
        z = CM.forward(torch.roll(X, s, -1), params, cyclic=False)
        assert float((z - torch.roll(CM.forward(X, params, cyclic=False), s, -1)).abs().max()) > 1e-3


def test_module_takes_the_flag_and_keeps_the_state_dict():
    import nasa_niswan_amd as pkg
    from oracle import convlstm_oracle as O
    ref = O.init_params(5, [16, 8], [5, 3], 2, out_channels=3)          # the keys and shapes of the reference's module tree
    net = pkg.ConvLSTM(5, [16, 8], [5, 3], 2, out_channels=3, lon_cyclic=True)
    plain = pkg.ConvLSTM(5, [16, 8], [5, 3], 2, out_channels=3)
    assert net.lon_cyclic is True and plain.lon_cyclic is False
    sd = net.state_dict()
    assert list(sd) == list(plain.state_dict()) and sorted(sd) == sorted(ref)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    plain.load_state_dict(sd)                                            # a checkpoint loads into either mode
    net.load_state_dict(plain.state_dict())
    with pytest.raises(TypeError):
        pkg.ConvLSTM(5, [16, 8], [5, 3], 2, 1, False, "f32", True)       # keyword-only
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(1, 2, 5, 8, 8))


def _seq(c, **kw):
    """nint_seq of a case as SeqEngine fills it (made-up addresses: the planner reads none)"""
    return TLP._seq_of(c["C"], **{k: v for k, v in c.items() if k != "C"}, **kw)


def test_struct_field_and_its_values():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    # behind probe_mask, in front of the 8-byte aligned probe; dh_seq stays the last field (tests/test_seq_train_cpu.py)
    S = _lib.NintSeq
    assert S.lon_cyclic.offset == S.probe_mask.offset + 4 and S.probe.offset == S.lon_cyclic.offset + 8
    assert S._fields_[-1][0] == "dh_seq" and S().lon_cyclic == 0
    assert lib.nint_version() == 113
    s = _seq(CM.CASES["B"], dtype="f32")
    for bwd in (0, 1):
        s.lon_cyclic = 1
        assert lib.nint_debug_seq_plan(C.byref(s), bwd, None, 0) > 0
        for bad in (-1, 2, 256):
            s.lon_cyclic = bad
            assert lib.nint_debug_seq_plan(C.byref(s), bwd, None, 0) == _lib.NINT_E_ARG
            assert (lib.nint_seq_bwd if bwd else lib.nint_seq_fwd)(C.byref(s), None) == _lib.NINT_E_ARG
    # W >= P: a wrapped halo column must be an interior column
    narrow = TLP._seq_of(3, [16], [7], 1, 2, 8, 2, "f32")
    assert lib.nint_debug_seq_plan(C.byref(narrow), 0, None, 0) > 0
    narrow.lon_cyclic = 1
    assert lib.nint_debug_seq_plan(C.byref(narrow), 0, None, 0) == _lib.NINT_E_ARG
    assert lib.nint_seq_fwd(C.byref(narrow), None) == _lib.NINT_E_ARG
    # the cyclic fold needs k/2 <= W too, before any launch
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 8, 2, 3) == 0
    assert lib.nint_pack_btchw_xfold_cyclic(16, 16, 1, 1, 3, 7, 32, C.byref(g), 0, None) == _lib.NINT_E_ARG
    assert lib.nint_unfold_dx_cyclic(16, 16, 1, 3, 7, 32, 8, 2, 0, None) == _lib.NINT_E_ARG


def _steps(recs):
    """[(index, [launch, ...])] of a plan in enqueue order"""
    out = []
    for idx, launch in recs:
        if not out or out[-1][0] != idx:
            out.append((idx, []))
        out[-1][1].append(launch)
    return out


WAVES_FUSES = [(w, f) for w in range(6) for f in (0, 1, 2)]


@pytest.mark.parametrize("case", ["A", "B", "D"])
@pytest.mark.parametrize("need_dx,has_init", [(False, False), (True, False), (False, True)])
def test_plan_is_the_zero_padded_plan_with_wraps_behind_writers_and_readers(case, need_dx, has_init):
    """Every schedule: the conv / pointwise launches of the cyclic plan are those of the zero-padded plan, record for record,
    and the enqueue indices in between are taken by exactly the wrap launches the rule asks for --
    forward: one at the head (an unfolded xs, a given initial state) and one behind every step (its gate problems' h blocks);
    BPTT: one behind every step with a dgrad (the CLEAR of the block it read, and the WRAP of what its epilogue wrote), and
    behind a step of pointwise passes alone only where a dgrad of the plan reads what it wrote (time 0 of the bottom layer
    from the zero state without an input gradient has none: that dG block must stay unwrapped for the weight gradient)."""
    c = CM.CASES[case]
    for dtype in ("f32", "bf16"):
        for wave, fuse in WAVES_FUSES:
            s = _seq(c, dtype=dtype, wave=wave, fuse=fuse, need_dx=need_dx, has_init=has_init)
            assert bool(s.layer[0].xfold) == CM.FOLDED[case]
            plain = TLP._library_plan(s, True)
            s.lon_cyclic = 1
            cyc = TLP._library_plan(s, True)
            assert [r[1] for r in cyc] == [r[1] for r in plain], (dtype, wave, fuse)
            for pass_ in ("fwd", "bwd"):
                a = _steps([r for r in plain if r[1].pass_ == pass_])
                b = _steps([r for r in cyc if r[1].pass_ == pass_])
                assert [len(x[1]) for x in a] == [len(x[1]) for x in b]
                reads = {(x.layer, x.t) for _, ls in a for x in ls if x.op in ("dgrad", "fused")}
                want, at = [], (1 if pass_ == "fwd" and (has_init or not CM.FOLDED[case]) else 0)
                for _, ls in a:
                    want.append(at)
                    behind = pass_ == "fwd" or any(x.op in ("dgrad", "fused") or (x.layer, x.t) in reads for x in ls)
                    at += 2 if behind else 1
                assert [x[0] for x in b] == want, (dtype, wave, fuse, pass_)
            if not need_dx and not has_init:      # the trap: the bottom layer's pointwise backward of time 0 has no reader
                assert (0, 0) not in {(x.layer, x.t) for _, x in plain if x.op in ("dgrad", "fused")}


def test_train_py_flag_needs_the_width_of_the_grid(tmp_path, capsys):
    """--cyclic-longitude: the model wraps at the edge of its own grid, so --input-size's width must be --grid's; the loss
    crop is then (latitude halo, 0).  Refused on the command line, before anything is written."""
    from nasa_niswan_amd import train as T
    snap = tmp_path / "s"
    argv = ["--model", "LSTM-cfg0", "--input-size", "100", "154", "--grid", "90", "144", "--snapshot-dir", str(snap)]
    with pytest.raises(SystemExit):
        T.get_arguments(argv + ["--cyclic-longitude"])
    assert "--cyclic-longitude" in capsys.readouterr().err and not snap.exists()
    args = T.get_arguments(["--model", "LSTM-cfg0", "--input-size", "100", "144", "--grid", "90", "144", "--cyclic-longitude",
                            "--snapshot-dir", str(snap)])
    assert args.cyclic_longitude is True
    assert T.get_arguments(argv).cyclic_longitude is False
