"""CPU: roll-out training as far as it needs no device -- the identities of the CPU model
(tests/rollout_model.py), the planner of the roll-out backward through nint_debug_seq_plan_rollout, every argument that
nint_seq_bwd_rollout and nint_head_feedback_bwd refuse "before any launch" (no call below reaches one), that the closed
entries keep refusing, and the ValueError / RuntimeError paths of the module and the trainer."""
import ctypes as C

import pytest
import torch

import closed_loop_model as CLM
import rollout_model as RM
import test_closed_loop_cpu as TCL
import test_launch_plan_cpu as TLP

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4
SMALL, STACK3 = TCL.SMALL, TCL.STACK3


# ------------------------------------------------------------------ the model's own identities
@pytest.mark.parametrize("storage", ["f32", "bf16", None])
@pytest.mark.parametrize("cyclic", [False, True])
def test_forward_is_the_closed_loop_model_bit_for_bit(cyclic, storage):
    c, p = SMALL, TCL._params(SMALL)
    X = TCL._x(c)
    for s in (1, 2, c["T"] - 1, c["T"], None):
        a = RM.forward(X, p, free_from=s, cyclic=cyclic, storage=storage)
        b = CLM.forward(X, p, free_from=s, cyclic=cyclic, storage=storage)
        for k in ("pred", "seq", "x_fed"):
            assert torch.equal(a[k], b[k]), (s, k)
        assert all(torch.equal(u, v) for u, v in zip(a["hs"] + a["cs"], b["hs"] + b["cs"]))


@pytest.mark.parametrize("cyclic", [False, True])
def test_gradients_open_loop_when_nothing_is_fed_and_different_when_something_is(cyclic):
    c, p = SMALL, TCL._params(SMALL)
    X = TCL._x(c)
    g = torch.Generator().manual_seed(2)
    dpred = torch.randn(c["B"], c["O"], c["H"], c["W"], generator=g, dtype=torch.float64)
    dseq = torch.randn(c["B"], c["T"] * c["O"], c["H"], c["W"], generator=g, dtype=torch.float64)
    opn = RM.grads(X, p, None, cyclic, "bf16", dpred, dseq)
    for s in (c["T"], c["T"] + 2):
        got = RM.grads(X, p, s, cyclic, "bf16", dpred, dseq)
        assert torch.equal(got["dx"], opn["dx"]) and all(torch.equal(got["params"][k], opn["params"][k]) for k in p)
    for s in (1, 2, c["T"] - 1):
        fed = RM.grads(X, p, s, cyclic, "bf16", dpred, dseq)
        # the caller's x never reached the fed channels of the fed steps
        assert not fed["dx"][:, s:, c["C"] - c["O"]:].any() and fed["dx"][:, :s].any()
        # teacher forcing on the very same input is another gradient: the fed term is there
        tf = RM.grads(fed["x_fed"], p, None, cyclic, "bf16", dpred, dseq)
        assert torch.equal(tf["seq"], fed["seq"])
        for k in p:             # (f64: a structural difference, ten orders above the arithmetic's noise)
            d = (fed["params"][k] - tf["params"][k]).norm() / tf["params"][k].norm()
            assert d > 1e-4, (s, k, float(d))
        # straight-through: the gradient is that of the unrounded model at the same forward values, up to the rounding of the values
        exact = RM.grads(X, p, s, cyclic, None, dpred, dseq)
        for k in p:
            assert (fed["params"][k] - exact["params"][k]).norm() <= 5e-2 * exact["params"][k].norm(), (s, k)


# ------------------------------------------------------------------ the library's planner
def _recs_rollout(s, fb):
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    cap = 8 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    n = lib.nint_debug_seq_plan_rollout(C.byref(s), C.byref(fb) if fb is not None else None, recs, cap)
    assert 0 <= n <= cap, n
    names = [f for f, _ in _lib.NintLaunchRec._fields_]
    return [{f: getattr(r, f) for f in names} for r in recs[:n]]


def _train_seq(Cin=5, wave=4, cyclic=False, has_init=False, need_dx=False, dtype="f32", fuse=None, **kw):
    s = TLP._seq_of(Cin, **{**STACK3, **kw}, dtype=dtype, wave=wave, has_init=has_init, need_dx=need_dx, fuse=fuse)
    s.lon_cyclic = int(cyclic)
    s.dh_seq = 1 << 31
    return s


@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("wave", [0, 4, 5])
def test_nothing_fed_is_the_plan_of_nint_seq_bwd(wave, need_dx):
    for dtype in ("f32", "bf16"):
        s = _train_seq(wave=wave, need_dx=need_dx, dtype=dtype)
        want = TCL._recs(s, None, bwd=1)
        assert len(want) > 0
        for fb in (None, TCL._fb(0, 0, w=None), TCL._fb(1, s.T), TCL._fb(1, s.T + 3)):
            assert _recs_rollout(s, fb) == want
        s.dh_seq = None                                   # ... which needs no per-step cotangents
        assert _recs_rollout(s, TCL._fb(1, s.T)) == TCL._recs(s, None, bwd=1)


@pytest.mark.parametrize("has_init", [False, True])
@pytest.mark.parametrize("Cin,O", [(5, 1), (64, 2)], ids=["folded", "plain"])
@pytest.mark.parametrize("cyclic", [False, True])
def test_plan_of_a_fed_window_is_time_major_classic_with_one_launch_per_fed_step(cyclic, Cin, O, has_init):
    """3 layers, T = 4, from = 1, whatever wave and fuse_bwd say: for u = T-1 ... 0, for l = L-1 ... 0 a pointwise backward
    and a dgrad, each its own launch -- record for record the plan of nint_seq_bwd under fuse_bwd = 1, wave = 0 with need_dx
    (the x columns of the fed steps are stored) -- and in the enqueue indices exactly one extra launch behind layer 0's dgrad
    of u = 1, 2, 3, none at u = 0."""
    L, T, F = 3, 4, 1
    OP_DGRAD, OP_PW = 1, 3
    strip = lambda r: {k: v for k, v in r.items() if k != "index"}
    for dtype in ("f32", "bf16"):
        for need_dx in (False, True):
            for wave, fuse in ((4, None), (0, 1), (5, 2)):
                s = _train_seq(Cin, wave, cyclic, has_init, need_dx, dtype, fuse, T=T)
                got = _recs_rollout(s, TCL._fb(O, F))
                seqn = [(r["op"], r["layer"], r["t"]) for r in got]
                want = []
                for u in range(T - 1, -1, -1):
                    for l in range(L - 1, -1, -1):
                        want.append((OP_PW, l, u))
                        if not (u == 0 and l == 0 and not has_init and not need_dx):    # nobody wants that launch's results
                            want.append((OP_DGRAD, l, u))
                assert seqn == want, (dtype, need_dx, wave)
                assert all(r["kernel"] in (0, 8) and r["bwd"] == 1 for r in got)         # no merged grid, no fused step
                # the classic time-major plan of the open-loop pass
                ref = _train_seq(Cin, 0, cyclic, has_init, True, dtype, 1, T=T)
                open_ = TCL._recs(ref, None, bwd=1)
                if not need_dx:         # the stored x columns of step 0 are the only launch that differs
                    open_ = [r for r in open_ if has_init or (r["op"], r["layer"], r["t"]) != (OP_DGRAD, 0, 0)]
                    assert [strip(r) for r in got if r["t"] >= F] == [strip(r) for r in open_ if r["t"] >= F]
                else:
                    assert [strip(r) for r in got] == [strip(r) for r in open_]
                # the indices: both plans hold the same launches and (cyclic) the same wraps in between, so a record's index
                # exceeds its twin's by the feedback launches enqueued before it -- one behind layer 0's dgrad of every fed
                # step u > t: T-1-t of them for t >= F-1, and none behind u = 0
                assert len(got) == len(open_)
                assert [g["index"] - o["index"] for g, o in zip(got, open_)] == [min(T - 1 - r["t"], T - F) for r in got]


def test_single_layer_plan():
    s = TLP._seq_of(4, [16], [5], 2, 4, 13, 37, "f32", need_dx=False)
    s.dh_seq = 1 << 31
    got = _recs_rollout(s, TCL._fb(1, 2))
    # pw(3) dgrad(3) FB pw(2) dgrad(2) FB pw(1) dgrad(1) pw(0)
    assert [(r["op"], r["t"], r["index"]) for r in got] == [(3, 3, 0), (1, 3, 1), (3, 2, 3), (1, 2, 4), (3, 1, 6), (1, 1, 7), (3, 0, 8)]


# ------------------------------------------------------------------ refusals of the library, before any launch
def test_rollout_refusals_before_any_launch():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    T = STACK3["T"]
    fb = TCL._fb(1, 2)

    def rg(dpred=1 << 28, dx_step=1 << 29):
        r = _lib.NintFeedbackGrad()
        r.dpred, r.dx_step = dpred, dx_step
        return r

    def both(s, f, r=None):
        """the plan entry (which makes up its own nint_feedback_grad) and the driver with made-up pointers"""
        a = lib.nint_debug_seq_plan_rollout(C.byref(s), C.byref(f), None, 0)
        b = lib.nint_seq_bwd_rollout(C.byref(s), C.byref(f), C.byref(r if r is not None else rg()), None)
        assert a == b, (a, b)
        return a

    s = _train_seq()
    assert lib.nint_debug_seq_plan_rollout(C.byref(s), C.byref(fb), None, 0) > 0
    for frm in (1, 2, T - 1):            # the closed entries are not touched: they refuse what they refused
        assert lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(TCL._fb(1, frm)), 1, None, 0) == E_ARG
        assert lib.nint_seq_bwd_closed(C.byref(s), C.byref(TCL._fb(1, frm)), None) == E_ARG
    assert both(s, TCL._fb(1, 0)) == E_ARG                                   # a step-0 feedback has no slot in the per-step slabs
    s.has_init_state = 1
    assert both(s, TCL._fb(1, 0)) == E_ARG                                   # ... from a given state either
    s.has_init_state = 0
    for bad in (TCL._fb(-1, 2), TCL._fb(6, 2), TCL._fb(1, 2, w=None), TCL._fb(1, -1)):
        assert both(s, bad) == E_ARG
    for field, val in (("train_from", 1), ("bwd_parts", 1), ("bwd_parts", 2), ("dh_seq", None), ("accumulate", 2), ("lon_cyclic", 2)):
        s = _train_seq()
        setattr(s, field, val)
        assert both(s, fb) == E_ARG, field
    s = _train_seq()
    s.dh_seq = (1 << 31) + 8
    assert both(s, fb) == E_ALIGN
    s = _train_seq()
    assert lib.nint_seq_bwd_rollout(C.byref(s), C.byref(fb), None, None) == E_ARG
    assert lib.nint_seq_bwd_rollout(C.byref(s), C.byref(fb), C.byref(rg(dpred=None)), None) == E_ARG
    assert lib.nint_seq_bwd_rollout(C.byref(s), C.byref(fb), C.byref(rg(dx_step=None)), None) == E_ARG      # need_dx = 0: the scratch
    assert lib.nint_seq_bwd_rollout(C.byref(s), C.byref(fb), C.byref(rg(dpred=(1 << 28) + 2)), None) == E_ALIGN
    assert lib.nint_seq_bwd_rollout(C.byref(s), C.byref(fb), C.byref(rg(dx_step=(1 << 29) + 8)), None) == E_ALIGN
    assert lib.nint_seq_bwd_rollout(None, C.byref(fb), C.byref(rg()), None) == E_ARG
    s = _train_seq(need_dx=True)
    s.dx = None
    assert both(s, fb) == E_ARG
    # a head the kernel does not hold: NINT_E_SHAPE from the planner, nothing enqueued
    wide = TLP._seq_of(5, [32, 160], [3, 3], 1, 3, 8, 8, "f32", wave=0, need_dx=False)
    wide.dh_seq = 1 << 31
    assert both(wide, TCL._fb(1, 1)) == E_SHAPE


def test_head_feedback_bwd_refuses_bad_arguments_before_any_launch():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 13, 37, 2) == 0
    # Made-up addresses: none is read before a launch, and NO call below reaches one.  dx is misaligned by default: NINT_E_ALIGN
    # is the last check but the shape rule, so a call that returns it has passed every argument check.
    DX, DP, DH, W_ = (1 << 12) + 8, 1 << 13, 1 << 14, 1 << 15

    def call(dx=DX, dx_n0=0, dp=DP, p_n0=0, dh=DH, dh_n0=0, N=2, Ch=8, Chp=32, O=1, w=W_, Cx=4, Cxp=32, c0=3, k=5, cyc=0, geom=g, dtype=1):
        return lib.nint_head_feedback_bwd(dx, dx_n0, dp, p_n0, dh, dh_n0, N, Ch, Chp, O, w, Cx, Cxp, c0, k, cyc,
                                          C.byref(geom) if geom else None, dtype, None)
    A_ = 1 << 12
    assert call() == E_ALIGN and call(dx=A_, dh=DH + 8) == E_ALIGN and call(dx=A_, dp=DP + 2) == E_ALIGN
    for kw in (dict(dx=None), dict(dp=None), dict(dh=None), dict(w=None), dict(geom=None), dict(N=0), dict(O=0), dict(Ch=0),
               dict(dtype=2), dict(Chp=4), dict(Chp=48), dict(c0=-1), dict(c0=4), dict(O=2), dict(k=4), dict(k=2), dict(k=-1),
               dict(Cxp=16), dict(k=0, Cx=40, Cxp=32, c0=37), dict(Cxp=36), dict(cyc=2), dict(cyc=-1), dict(dx_n0=-1), dict(p_n0=-1),
               dict(dh_n0=-1)):
        assert call(**kw) == E_ARG, kw
    narrow = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(narrow), 8, 2, 3) == 0
    assert call(geom=narrow, k=7, Cxp=32, cyc=0) == E_ALIGN and call(geom=narrow, k=7, Cxp=32, cyc=1) == E_ARG
    assert call(k=0, dtype=0, Chp=16) == E_ALIGN and call(k=1) == E_ALIGN and call(k=0, Cx=40, Cxp=64, c0=37, O=3) == E_ALIGN
    # exactly the shapes nint_head_feedback holds
    assert call(dx=A_, Ch=130, Chp=160) == E_SHAPE
    assert call(dx=A_, Ch=128, Chp=128, O=400, Cx=400, Cxp=416, c0=0, k=0) == E_SHAPE
    big = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(big), 8, 4000, 2) == 0
    assert call(dx=A_, geom=big, O=20, Cx=32, Cxp=32, c0=12, k=0) == E_SHAPE


def test_structs_and_version():
    from nasa_niswan_amd import _lib
    S, F, G = _lib.NintSeq, _lib.NintFeedback, _lib.NintFeedbackGrad
    assert S._fields_[-1][0] == "dh_seq" and S.dh_seq.offset + 8 == C.sizeof(S)        # nint_seq is what it was
    assert (F.w.offset, F.b.offset, F.O.offset, F.from_step.offset, C.sizeof(F)) == (0, 8, 16, 20, 24)
    assert (G.dpred.offset, G.dx_step.offset, C.sizeof(G)) == (0, 8, 16)
    assert _lib.load().nint_version() == 113


# ------------------------------------------------------------------ the host surface, where it needs no device
def test_module_keyword_and_refusals():
    import nasa_niswan_amd as pkg
    net = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2, feedback=True)
    x = torch.zeros(1, 3, 6, 8, 8)
    with pytest.raises(TypeError):
        net(x, None, False, 1, True)                                                 # keyword-only
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(x, free_from=1)                                                          # without the keyword: today's refusal
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(x, free_from=1, feedback_grad=False)
    for s in (1, 2):
        with pytest.raises(RuntimeError, match="no CPU path"):                       # past the refusals: the device check
            net(x, free_from=s, feedback_grad=True)
    h = [(torch.zeros(1, 8, 8, 8, requires_grad=True), torch.zeros(1, 8, 8, 8)), (torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8))]
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(x, h, free_from=0, feedback_grad=True)                                   # a step-0 feedback stays refused
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(x, h, free_from=1, feedback_grad=True)
    plain = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2)
    with pytest.raises(ValueError, match="feedback=True"):
        plain(x, free_from=1, feedback_grad=True)


@pytest.mark.parametrize("case", ["all", "thin"])
def test_the_gpu_cases_separate_rollout_from_teacher_forcing(case):
    """what tests/test_gpu_rollout.py relies on: in its cases the roll-out gradient is far from the teacher-forced gradient on the
    same input in the gates' own measures, so a backward pass that dropped the fed term cannot pass them"""
    T = CLM.CASES[case]["T"]
    for F_ in (1, 2, T - 1):
        ro, tf = RM.reference(case, False, F_, False)
        assert torch.equal(ro["seq"], tf["seq"])
        sep = RM.separation(ro, tf)
        assert min(a for a, _ in sep.values()) > 2, (F_, sep)           # every parameter: more than two f32 gates
        if F_ < T - 1:          # (one fed step moves the gradients by less: 1.9 bf16 gates at most in `thin`)
            assert max(b for _, b in sep.values()) > 2, (F_, sep)       # some parameter: more than two bf16 gates


def test_trainer_and_train_py_refusals(tmp_path, capsys):
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd import train as T
    from nasa_niswan_amd._lib import NintError
    from nasa_niswan_amd.trainer import FusedTrainer
    net = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2, feedback=True)
    for bad in (0, -1, True, 1.5):
        with pytest.raises(ValueError, match="rollout_from must be a step index >= 1"):
            FusedTrainer(net, rollout_from=bad)
    for kw, word in ((dict(bptt_segments=2), "bptt_segments"), (dict(stateful=True), "stateful"), (dict(freeze_layers=1), "freeze_layers"),
                     (dict(overlap_allreduce=True), "overlap_allreduce")):
        with pytest.raises(ValueError, match=f"rollout_from with {word}"):
            FusedTrainer(net, rollout_from=1, **kw)
    with pytest.raises(ValueError, match="feedback=True"):
        FusedTrainer(pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2), rollout_from=1)
    for kw in (dict(rollout_from=1), dict(rollout_from=2, bptt_segments=1, sequence_loss=True, accumulate_steps=2, max_grad_norm=1.0),
               dict(rollout_from=None)):
        with pytest.raises(NintError, match="needs the model on the MI355X"):        # past the refusals: the device check
            FusedTrainer(net, **kw)
    snap = tmp_path / "s"
    base = ["--model", "LSTM-x", "--grid", "28", "32", "--input-size", "28", "32", "--snapshot-dir", str(snap)]
    for extra in (["--rollout-from", "1"], ["--tracer-input", "--rollout-from", "0"], ["--tracer-input", "--rollout-from", "1", "--stateful"],
                  ["--tracer-input", "--rollout-from", "1", "--bptt-segments", "2"],
                  ["--tracer-input", "--rollout-from", "1", "--freeze-layers", "1"]):
        with pytest.raises(SystemExit):
            T.get_arguments(base + extra)
        assert "--rollout-from" in capsys.readouterr().err and not snap.exists()
    args = T.get_arguments(base + ["--tracer-input", "--cyclic-longitude", "--rollout-from", "2"])
    assert args.rollout_from == 2
    assert T.get_arguments(base + ["--tracer-input"]).rollout_from is None


# ------------------------------------------------------------------ the random-shape screen's roll-out mode
def _fuzz_tool():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fuzz_shapes_ro", os.path.join(root, "tools", "fuzz_shapes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_rollout_fuzz_seeds_contain_what_the_mode_exists_for():
    from nasa_niswan_amd import _lib
    import test_gpu_fuzz_rollout as FZ
    tool = _fuzz_tool()
    args = tool.parse(FZ.RUN)
    assert args.mode == "rollout"
    cases = tool.draw_cases(args.seed, args.n, args.mode)
    lib = _lib.load()
    fed = [c for c in cases if c["fb_from"] < c["T"]]
    folded = lambda c: c["fold"] and bool(lib.nint_xfold_pays(c["C"], c["ks"][0], 1 if c["dtype"] == "bf16" else 0))
    assert any(folded(c) for c in fed) and any(not folded(c) for c in fed), "folded and plain inputs"
    assert any(c["cyclic"] for c in fed) and any(not c["cyclic"] for c in fed), "both boundaries"
    assert {c["dtype"] for c in fed} == {"f32", "bf16"}
    assert all(c["fb_from"] >= 1 and 1 <= c["out"] <= c["C"] for c in cases)
    kinds = {"first" if c["fb_from"] == 1 else "last" if c["fb_from"] == c["T"] - 1 else "none" if c["fb_from"] == c["T"] else "middle"
             for c in cases}
    assert kinds == {"first", "middle", "last", "none"}, kinds
    assert {c["cot"] for c in fed} == {"seq", "last", "both"}
    # the mode continues the stream numbering behind the pinned list: no earlier mode's draws move
    assert tool.ALL_STREAM_MODES == tool.STREAM_MODES + ("rollout",) and tool.STREAM_MODES[-1] == "closed_loop"
    assert tool.draw_case(tool.case_rng(1913, "rollout", 5), 5, "rollout") == cases[5]


# sha256 (first 16 hex digits) of json.dumps(draw_cases(5, 4, mode), sort_keys=True), taken from the tool as it stood before the
# roll-out mode was added: what `--list --seed 5 --n 4` of each older mode prints
OLDER_MODE_DRAWS = {"plain": "5f0d984e1fda6e30", "trainer": "a0e704fc505c6569", "cell": "cd920130566d3032", "dataset": "6fec11e41a834020",
                    "state": "4f0a2cd8de726165", "train_opts": "9a45bd1fabab7a0c", "stateful": "4da2b95060f43a14",
                    "finetune": "72ca00d1c7da3391", "closed_loop": "ca721dbd63f3e766"}


def test_list_of_the_older_modes_is_unchanged():
    """every older mode draws the cases it drew: the recorded digests of its --list output, and the stream key of the modes that
    have one -- (seed, position in STREAM_MODES, iteration)"""
    import hashlib
    import json
    tool = _fuzz_tool()
    import numpy as np
    assert set(OLDER_MODE_DRAWS) == {"plain", "trainer", "cell", "dataset"} | set(tool.STREAM_MODES)
    for mode, want in OLDER_MODE_DRAWS.items():
        got = hashlib.sha256(json.dumps(tool.draw_cases(5, 4, mode), sort_keys=True).encode()).hexdigest()[:16]
        assert got == want, mode
    for pos, mode in enumerate(tool.STREAM_MODES):
        a = tool.case_rng(7, mode, 3).standard_normal(4)
        b = np.random.default_rng([7, 1 + pos, 3]).standard_normal(4)
        assert np.array_equal(a, b), mode
