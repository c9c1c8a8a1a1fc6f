"""CPU: the closed-loop forward as far as it needs no device -- the identities of the CPU model
(tests/closed_loop_model.py), the library's planner through nint_debug_seq_plan_closed, every argument the library refuses
"before any launch" (this machine has no GPU: a launch attempt would return a HIP error code, not NINT_E_ARG), and the
ValueError / RuntimeError paths of the model, the datasets, the inference helpers and train.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_model as CLM
import test_launch_plan_cpu as TLP

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


def _params(c, dtype=torch.float64, seed=3):
    from oracle import convlstm_oracle as O
    return O.synth_params(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=c["O"], seed=seed, dtype=dtype)


def _x(c, T=None, seed=5, dtype=torch.float64):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((c["B"], c["T"] if T is None else T, c["C"], c["H"], c["W"]))).to(dtype)


SMALL = dict(C=4, O=2, hidden=[6, 5], ks=[3, 3], B=2, T=4, H=5, W=7)


# ------------------------------------------------------------------ the model's own identities
@pytest.mark.parametrize("cyclic", [False, True])
def test_free_from_beyond_the_window_is_the_open_loop(cyclic):
    import cyclic_model as CM
    c, p = SMALL, _params(SMALL)
    X = _x(c)
    want_pred, want_seq = CM.forward(X, p, cyclic=cyclic, return_sequence=True)
    for s in (None, c["T"], c["T"] + 3):
        got = CLM.forward(X, p, free_from=s, cyclic=cyclic, storage="bf16")
        assert torch.equal(got["pred"], want_pred) and torch.equal(got["seq"], want_seq) and torch.equal(got["x_fed"], X)


@pytest.mark.parametrize("storage", ["f32", "bf16", None])
@pytest.mark.parametrize("cyclic", [False, True])
def test_closed_loop_is_the_open_loop_on_the_fed_input(cyclic, storage):
    """if the feedback channels of x already hold the rounded predictions, closed loop equals open loop exactly"""
    c, p = SMALL, _params(SMALL)
    X = _x(c)
    O_, Cc = c["O"], c["C"]
    for s in (1, 2):
        a = CLM.forward(X, p, free_from=s, cyclic=cyclic, storage=storage)
        assert torch.equal(a["x_fed"][:, :s], X[:, :s]) and torch.equal(a["x_fed"][:, :, :Cc - O_], X[:, :, :Cc - O_])
        assert not torch.equal(a["x_fed"][:, s:, Cc - O_:], X[:, s:, Cc - O_:])
        # the fed value of step t is the rounded head output of step t-1
        seq = a["seq"].view(c["B"], c["T"], O_, c["H"], c["W"])
        assert torch.equal(a["x_fed"][:, s:, Cc - O_:], CLM.round_et(seq[:, s - 1:-1], storage))
        b = CLM.forward(a["x_fed"], p, free_from=None, cyclic=cyclic, storage=storage)
        for k in ("pred", "seq"):
            assert torch.equal(a[k], b[k]), (s, k)
        assert all(torch.equal(u, v) for u, v in zip(a["hs"] + a["cs"], b["hs"] + b["cs"]))
        # ... and feeding the model its own input again changes nothing
        again = CLM.forward(a["x_fed"], p, free_from=s, cyclic=cyclic, storage=storage)
        assert torch.equal(again["seq"], a["seq"])


@pytest.mark.parametrize("cyclic", [False, True])
def test_two_chunks_with_carried_state_are_one_window(cyclic):
    c, p = SMALL, _params(SMALL)
    X = _x(c, T=6)
    whole = CLM.forward(X, p, free_from=2, cyclic=cyclic, storage="bf16")
    a = CLM.forward(X[:, :3], p, free_from=2, cyclic=cyclic, storage="bf16")
    b = CLM.forward(X[:, 3:], p, free_from=0, cyclic=cyclic, storage="bf16", h0=a["hs"], c0=a["cs"])
    assert torch.equal(torch.cat([a["seq"], b["seq"]], dim=1), whole["seq"]) and torch.equal(b["pred"], whole["pred"])
    assert all(torch.equal(u, v) for u, v in zip(b["hs"] + b["cs"], whole["hs"] + whole["cs"]))
    with pytest.raises(ValueError):
        CLM.forward(X, p, free_from=0)                                 # step 0 has nothing to be fed from


# ------------------------------------------------------------------ the library's planner
STACK3 = dict(hidden=[32, 16, 16], ks=[5, 3, 3], B=2, T=5, H=13, W=37)


def _fb(O, from_step, w=1 << 12, b=None):
    from nasa_niswan_amd import _lib
    fb = _lib.NintFeedback()
    fb.w, fb.b, fb.O, fb.from_step = w, b, O, from_step
    return fb


def _recs(s, fb=None, bwd=0):
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    cap = 8 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    if fb is None:
        n = lib.nint_debug_seq_plan(C.byref(s), bwd, recs, cap)
    else:
        n = lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(fb), bwd, recs, cap)
    assert 0 <= n <= cap, n
    names = [f for f, _ in _lib.NintLaunchRec._fields_]
    return [{f: getattr(r, f) for f in names} for r in recs[:n]]


@pytest.mark.parametrize("has_init", [False, True])
@pytest.mark.parametrize("Cin,O", [(5, 1), (64, 2)], ids=["folded", "plain"])
@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("wave", [0, 4, 5])
def test_plan_of_a_fed_window(wave, cyclic, Cin, O, has_init):
    """3 layers, T = 5, from = 2: steps 0 and 1 are the open-loop plan of a 2-step window record for record; every gate of
    t >= 2 is a launch of its own, time-major, on the tile rows its `wave` gives it; the enqueue indices in between are taken
    by exactly the feedback launches (and, cyclic, the halo wraps: one at the head for an unfolded xs or a given state, one
    behind every gate step, one behind a feedback into an unfolded xs)"""
    F, L, T = 2, 3, STACK3["T"]
    for dtype in ("f32", "bf16"):
        s = TLP._seq_of(Cin, **STACK3, dtype=dtype, wave=wave, has_init=has_init, train=False)
        s.lon_cyclic = int(cyclic)
        folded = bool(s.layer[0].xfold)
        assert folded == (Cin == 5)
        got = _recs(s, _fb(O, F))
        s.T = F
        head = _recs(s)
        s.T = T
        strip = lambda r: {k: v for k, v in r.items() if k != "index"}
        n_open = len(head)
        assert [strip(r) for r in got[:n_open]] == [strip(r) for r in head]
        assert all(r["t"] < F for r in got[:n_open])
        # the indices: walk the rule
        idx = 1 if cyclic and (has_init or not folded) else 0
        want, last = [], None
        for r in head:                                  # the open part: a merged grid's problems share an index
            if last is not None and r["index"] != last:
                idx += 2 if cyclic else 1
            last = r["index"]
            want.append(idx)
        idx += 2 if cyclic else 1
        tail = got[n_open:]
        assert [(r["t"], r["layer"]) for r in tail] == [(t, l) for t in range(F, T) for l in range(L)]
        for t in range(F, T):
            idx += 1 + int(cyclic and not folded)       # the feedback launch (and the wrap of the xs block it wrote)
            for l in range(L):
                want.append(idx)
                idx += 2 if cyclic else 1
        assert [r["index"] for r in got] == want, (dtype, [r["index"] for r in got], want)
        assert all(r["op"] == 0 and r["bwd"] == 0 for r in tail)
        # the tile rows of the open-loop pass under the same wave: 8 rows under wave 2 / 3 / 4, record for record
        s.T = T
        whole = {(r["t"], r["layer"]): strip(r) for r in _recs(s)}
        for r in tail:
            w = dict(whole[(r["t"], r["layer"])])
            if w["kernel"] in (1, 2):                   # a problem of a merged forward grid there: the same body, its own launch here
                w["kernel"] = 0
            assert strip(r) == w, (dtype, r, w)
            if wave == 4:
                assert r["mt"] == 8
        # O = 0, a NULL structure and the open entry give one plan
        assert _recs(s, _fb(0, 0, w=None)) == _recs(s)
        # from >= T: nothing is fed, nothing is planned in between
        assert _recs(s, _fb(O, T)) == _recs(s) and _recs(s, _fb(O, T + 4)) == _recs(s)


def test_single_layer_and_from_zero_plans():
    s = TLP._seq_of(4, [16], [5], 2, 4, 13, 37, "f32", has_init=True, train=False)
    got = _recs(s, _fb(1, 0))
    assert [(r["t"], r["index"]) for r in got] == [(t, 2 * t + 1) for t in range(4)]
    got = _recs(s, _fb(1, 3))
    assert [(r["t"], r["index"]) for r in got] == [(0, 0), (1, 1), (2, 2), (3, 4)]


# ------------------------------------------------------------------ refusals of the library, before any launch
def test_seq_check_refuses_bad_feedback_before_any_launch():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    s = TLP._seq_of(5, **STACK3, dtype="f32", wave=4, has_init=False, train=True)
    T = s.T
    assert lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(_fb(1, 2)), 0, None, 0) > 0
    bad = [_fb(-1, 2), _fb(6, 2), _fb(1, 2, w=None), _fb(1, -1), _fb(1, 0)]
    for fb in bad:
        for bwd in (0, 1):
            assert lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(fb), bwd, None, 0) == E_ARG, (fb.O, fb.from_step)
        assert lib.nint_seq_fwd_closed(C.byref(s), C.byref(fb), None) == E_ARG
        assert lib.nint_seq_bwd_closed(C.byref(s), C.byref(fb), None) == E_ARG
    assert lib.nint_seq_fwd_closed(None, C.byref(_fb(1, 2)), None) == E_ARG
    # O == Cx is the widest feedback; from = 0 is fine from a given state
    assert lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(_fb(5, 1)), 0, None, 0) > 0
    s.has_init_state = 1
    assert lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(_fb(1, 0)), 0, None, 0) > 0
    # the backward pass of a fed window is not defined; a window in which nothing is fed back trains as ever
    for frm in (0, 1, T - 1):
        assert lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(_fb(1, frm)), 1, None, 0) == E_ARG
        assert lib.nint_seq_bwd_closed(C.byref(s), C.byref(_fb(1, frm)), None) == E_ARG
    assert _recs(s, _fb(1, T), bwd=1) == _recs(s, None, bwd=1) and len(_recs(s, None, bwd=1)) > 0
    # a head the staged kernels do not hold: NINT_E_SHAPE from the planner, nothing enqueued
    wide = TLP._seq_of(5, [32, 160], [3, 3], 1, 3, 8, 8, "f32", wave=0, train=False)
    assert lib.nint_debug_seq_plan_closed(C.byref(wide), C.byref(_fb(1, 1)), 0, None, 0) == E_SHAPE
    assert lib.nint_seq_fwd_closed(C.byref(wide), C.byref(_fb(1, 1)), None) == E_SHAPE


def test_head_feedback_refuses_bad_arguments_before_any_launch():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 13, 37, 2) == 0
    # Made-up addresses: none is read before a launch, and NO call below reaches one (this file also runs where there is a GPU).
    # The h slab is misaligned by default: NINT_E_ALIGN is the last check but the shape rule, so a call that returns it has
    # passed every argument check, and NINT_E_ARG can only come from the one argument a case changes.
    H_, W_, X_ = (1 << 12) + 8, 1 << 13, 1 << 14

    def call(h=H_, n0=0, N=2, Ch=8, Chp=32, O=1, w=W_, b=None, xs=X_, x_n0=0, Cx=4, Cxp=32, c0=3, k=5, cyc=0, geom=g, dtype=1):
        return lib.nint_head_feedback(h, n0, N, Ch, Chp, O, w, b, xs, x_n0, Cx, Cxp, c0, k, cyc, C.byref(geom) if geom else None,
                                      dtype, None)
    assert call() == E_ALIGN and call(h=1 << 12, xs=X_ + 4) == E_ALIGN
    for kw in (dict(h=None), dict(w=None), dict(xs=None), dict(geom=None), dict(N=0), dict(O=0), dict(Ch=0), dict(dtype=2),
               dict(Chp=4), dict(Chp=48), dict(c0=-1), dict(c0=4), dict(O=2), dict(k=4), dict(k=2), dict(k=-1),
               dict(Cxp=16), dict(k=0, Cx=40, Cxp=32, c0=37), dict(Cxp=36), dict(cyc=2), dict(cyc=-1), dict(n0=-1), dict(x_n0=-1)):
        assert call(**kw) == E_ARG, kw
    narrow = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(narrow), 8, 2, 3) == 0
    assert call(geom=narrow, k=7, Cxp=32, cyc=0) == E_ALIGN
    assert call(geom=narrow, k=7, Cxp=32, cyc=1) == E_ARG       # W < P: a wrapped column must be an interior one
    # a plain slab, f32, and xfold_k = 1 (a plain slab too) pass the argument checks
    assert call(k=0, dtype=0, Chp=16) == E_ALIGN and call(k=1) == E_ALIGN and call(k=0, Cx=40, Cxp=64, c0=37, O=3) == E_ALIGN
    assert call(cyc=1) == E_ALIGN and call(b=1 << 15) == E_ALIGN
    # shapes the kernel does not hold: NINT_E_SHAPE with everything else in order, before any launch
    A_ = 1 << 12
    assert call(h=A_, Ch=130, Chp=160) == E_SHAPE                # beyond the staged head
    assert call(h=A_, Ch=128, Chp=128, O=400, Cx=400, Cxp=416, c0=0, k=0) == E_SHAPE
    big = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(big), 8, 4000, 2) == 0
    assert call(h=A_, geom=big, O=20, Cx=32, Cxp=32, c0=12, k=0) == E_SHAPE      # a row of predictions beyond the LDS


def test_struct_and_entries():
    from nasa_niswan_amd import _lib
    S = _lib.NintSeq
    assert S._fields_[-1][0] == "dh_seq" and S.dh_seq.offset + 8 == C.sizeof(S)       # nint_seq is what it was
    F = _lib.NintFeedback
    assert (F.w.offset, F.b.offset, F.O.offset, F.from_step.offset, C.sizeof(F)) == (0, 8, 16, 20, 24)
    assert F().O == 0 and _lib.load().nint_version() == 113


# ------------------------------------------------------------------ refusals of the host surface that need no device
def test_module_flag_and_refusals():
    import nasa_niswan_amd as pkg
    plain = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2)
    net = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2, feedback=True)
    assert net.feedback is True and plain.feedback is False
    assert list(net.state_dict()) == list(plain.state_dict())
    plain.load_state_dict(net.state_dict())
    with pytest.raises(TypeError):
        pkg.ConvLSTM(6, [8, 4], [3, 3], 2, 1, False, "f32", False, True)            # keyword-only
    with pytest.raises(ValueError, match="out_channels <= input_channels"):
        pkg.ConvLSTM(2, [8], [3], 1, out_channels=3, feedback=True)
    pkg.ConvLSTM(3, [8], [3], 1, out_channels=3, feedback=True)                      # O == C is the widest
    x = torch.zeros(1, 3, 6, 8, 8)
    with pytest.raises(ValueError, match="feedback=True"):
        plain(x, free_from=1)
    with pytest.raises(ValueError, match="pass a state"):
        net(x, free_from=0)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="free_from"):
            net(x, free_from=bad)
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(x, free_from=1)                                                          # parameters require grad, grad mode is on
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU path"):                       # past the refusals: the device check
            net(x, free_from=1)
    with pytest.raises(RuntimeError, match="no CPU path"):                           # nothing is fed back: trains as ever
        net(x, free_from=3)
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="back-propagation"):
        net(x.clone().requires_grad_(True), free_from=2)
    h = [(torch.zeros(1, 8, 8, 8, requires_grad=True), torch.zeros(1, 8, 8, 8)), (torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8))]
    with pytest.raises(RuntimeError, match="back-propagation"):
        net(x, h, free_from=0)


def test_dataset_tracer_input_on_the_host():
    from nasa_niswan_amd.dataset import E33OMA90D_CRNN, SyntheticE33OMA_CRNN
    kw = dict(sequence_length=4, n_steps=24, grid=(12, 16), device="cpu")
    ds = SyntheticE33OMA_CRNN("train", padding=None, in_channels=6, tracer_input=True, **kw)
    base = SyntheticE33OMA_CRNN("train", padding=None, in_channels=5, **kw)
    assert ds.in_channels == 6 and ds.tracer_input and not ds.generic and int(ds.first[0]) == 1 and len(ds) == len(base) - 1
    assert np.array_equal(ds.yraw, base.yraw) and np.array_equal(ds.u, base.u)           # the record of a seed does not change
    assert np.array_equal(ds.X_mean[:5], base.X_mean) and ds.X_mean[5] == ds.y_mean and ds.X_std[5] == ds.y_std
    same = SyntheticE33OMA_CRNN("val", padding=(12, 16), in_channels=6, tracer_input=True, **kw)
    assert int(same.first[0]) == int(SyntheticE33OMA_CRNN("val", padding=None, in_channels=5, **kw).first[0]) >= 1
    lv = SyntheticE33OMA_CRNN("train", padding=None, in_channels=14, levels=3, tracer_input=True, **kw)
    assert lv.X_mean.shape == (14,) and not lv.generic
    gen = SyntheticE33OMA_CRNN("train", padding=None, in_channels=4, tracer_input=True, **kw)
    assert gen.generic and gen.gen.shape[1] == 3
    with pytest.raises(ValueError, match="lon_cyclic"):
        SyntheticE33OMA_CRNN("train", padding=(14, 16), in_channels=6, tracer_input=True, **kw)
    with pytest.raises(ValueError, match="static"):
        SyntheticE33OMA_CRNN("train", padding=None, in_channels=8, static_channels=2, tracer_input=True, **kw)
    with pytest.raises(ValueError, match="in_channels"):
        SyntheticE33OMA_CRNN("train", padding=None, in_channels=1, tracer_input=True, **kw)
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    arrs = [f(24, 12, 16) for _ in range(6)]
    real = E33OMA90D_CRNN.from_arrays(*arrs, period="train", padding=None, sequence_length=4, device="cpu", pinned=False,
                                      tracer_input=True)
    assert real.in_channels == 6 and int(real.first[0]) == 1
    with pytest.raises(ValueError, match="lon_cyclic"):
        E33OMA90D_CRNN.from_arrays(*arrs, period="train", padding=(22, 26), sequence_length=4, device="cpu", pinned=False,
                                   tracer_input=True)


def test_inference_and_train_py_refusals(tmp_path, capsys):
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd import inference, train as T
    plain = pkg.ConvLSTM(6, [8], [3], 1)
    with pytest.raises(ValueError, match="feedback=True"):
        inference.predict_stream(plain, None, closed_loop=True)
    with pytest.raises(ValueError, match="feedback=True"):
        inference.rollout_skill(plain, None, [1], 4, 2)
    fed = pkg.ConvLSTM(6, [8], [3], 1, feedback=True)
    with pytest.raises(ValueError, match="spinup"):
        inference.predict_stream(fed, None, closed_loop=True, spinup=0)
    with pytest.raises(ValueError, match="horizon and spinup"):
        inference.rollout_skill(fed, None, [1], 0, 2)
    snap = tmp_path / "s"
    base = ["--model", "LSTM-x", "--grid", "28", "32", "--snapshot-dir", str(snap)]
    for extra, word in ((["--tracer-input", "--input-size", "32", "32"], "--tracer-input"),
                        (["--test-rollout", "4", "--input-size", "28", "32"], "--test-rollout"),
                        (["--tracer-input", "--input-size", "28", "32", "--static-channels", "2", "--in-channels", "7"], "--static-channels")):
        with pytest.raises(SystemExit):
            T.get_arguments(base + extra)
        assert word in capsys.readouterr().err and not snap.exists()
    args = T.get_arguments(base + ["--tracer-input", "--cyclic-longitude", "--input-size", "28", "32", "--test-rollout", "6",
                                   "--sequence-length", "5"])
    assert args.tracer_input and args.test_rollout == 6 and args.rollout_spinup == 5


# ------------------------------------------------------------------ the random-shape screen's closed-loop mode
def test_closed_loop_fuzz_seeds_contain_what_the_mode_exists_for():
    import importlib.util
    import os
    from nasa_niswan_amd import _lib
    import test_gpu_fuzz_closed_loop as FZ
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fuzz_shapes_cl", os.path.join(root, "tools", "fuzz_shapes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse(FZ.RUN)
    assert args.mode == "closed_loop"
    cases = tool.draw_cases(args.seed, args.n, args.mode)
    lib = _lib.load()
    fed = [c for c in cases if c["fb_from"] < c["T"]]
    folded = lambda c: c["fold"] and bool(lib.nint_xfold_pays(c["C"], c["ks"][0], 1 if c["dtype"] == "bf16" else 0))
    assert any(folded(c) for c in fed), "a folded input"
    assert any(not folded(c) for c in fed), "a plain input"
    assert any(c["cyclic"] and folded(c) for c in fed) and any(c["cyclic"] and not folded(c) for c in fed), "cyclic, both layouts"
    assert any(c["with_state"] for c in fed) and any(c["fb_from"] == 0 for c in fed), "with a state, and fed from step 0"
    assert any(c["out"] > 1 for c in fed) and any(c["fb_from"] > 1 for c in fed)
    assert any(c["fb_from"] >= c["T"] for c in cases), "nothing fed back"
    assert {c["dtype"] for c in fed} == {"f32", "bf16"} and any(c["L"] == 1 for c in fed) and any(c["L"] > 1 for c in fed)
    assert all(1 <= c["out"] <= c["C"] and (c["fb_from"] > 0 or c["with_state"]) for c in cases)
    # the mode has a stream of its own; the modes before it keep theirs (tests/test_fuzz_draw_cpu.py pins their draws)
    assert tool.STREAM_MODES[:len(tool.NEW_MODES)] == tool.NEW_MODES and tool.STREAM_MODES[-1] == "closed_loop"
    assert tool.draw_case(tool.case_rng(811, "closed_loop", 5), 5, "closed_loop") == cases[5]
