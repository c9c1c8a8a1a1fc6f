"""CPU: scheduled sampling as far as it needs no device -- the planner under a feed mask through
nint_debug_seq_plan_sampled (a suffix mask IS ``from = s``, record for record), every argument the _sampled entries and the two
_sel kernels' entries refuse "before any launch" (no call below reaches one), the identities of the CPU model
(tests/sampled_model.py), the trainer's draw, and the ValueError / RuntimeError paths of the module and the trainer."""
import ctypes as C

import numpy as np
import pytest
import torch

import rollout_model as RM
import sampled_model as SM
import test_closed_loop_cpu as TCL
import test_rollout_cpu as TRO

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4
FWD, BWD, ROLLOUT = 0, 1, 2
SMALL, STACK3 = TCL.SMALL, TCL.STACK3


def _mask(tb):
    """(T, B) array of 0 / 1 -> (nint_feedback_mask, the bytes it points at: keep them alive)"""
    from nasa_niswan_amd import _lib
    a = np.ascontiguousarray(np.asarray(tb, dtype=np.uint8))
    fm = _lib.NintFeedbackMask()
    fm.fed = a.ctypes.data
    return fm, a


def _suffix(T, B, s):
    return (np.arange(T)[:, None] >= s) * np.ones((1, B), np.uint8)


def _plan(s, fb, tb, direction):
    """(return code or number of records, records) of nint_debug_seq_plan_sampled; tb None: a NULL mask"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    cap = 8 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    fm, keep = _mask(tb) if tb is not None else (None, None)
    n = lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(fb) if fb is not None else None, C.byref(fm) if fm is not None else None,
                                        direction, recs, cap)
    assert n <= cap, n
    names = [f for f, _ in _lib.NintLaunchRec._fields_]
    return n, [{f: getattr(r, f) for f in names} for r in recs[:max(n, 0)]]


def _plan_from(s, fb, direction):
    """the same of the entries the mask extends: nint_debug_seq_plan_closed (forward, refused backward) / _rollout"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    cap = 8 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    if direction == ROLLOUT:
        n = lib.nint_debug_seq_plan_rollout(C.byref(s), C.byref(fb), recs, cap)
    else:
        n = lib.nint_debug_seq_plan_closed(C.byref(s), C.byref(fb), direction, recs, cap)
    names = [f for f, _ in _lib.NintLaunchRec._fields_]
    return n, [{f: getattr(r, f) for f in names} for r in recs[:max(n, 0)]]


# ------------------------------------------------------------------ the library's planner
@pytest.mark.parametrize("has_init", [False, True])
@pytest.mark.parametrize("Cin,O", [(5, 1), (64, 2)], ids=["folded", "plain"])
@pytest.mark.parametrize("cyclic", [False, True])
def test_a_suffix_mask_and_a_null_mask_give_the_plan_of_from(cyclic, Cin, O, has_init):
    """T in {1, 4, 5}, B in {1, 3}, every s in [0, T]: forward, refused backward and roll-out alike -- the return code and every
    field of every record; a NULL mask (a NULL structure, a NULL pointer in it) leaves the entry it extends"""
    from nasa_niswan_amd import _lib
    seen = set()
    for T in (1, 4, 5):
        for B in (1, 3):
            s = TRO._train_seq(Cin, 4, cyclic, has_init, False, "bf16", None, T=T, B=B)
            assert bool(s.layer[0].xfold) == (Cin == 5)
            for frm in range(T + 1):
                for direction in (FWD, BWD, ROLLOUT):
                    want = _plan_from(s, TCL._fb(O, frm), direction)
                    # (fb->from is ignored under a mask: a value that would be refused by itself)
                    got = _plan(s, TCL._fb(O, -7), _suffix(T, B, frm), direction)
                    assert got == want, (T, B, frm, direction, got[0], want[0])
                    assert _plan(s, TCL._fb(O, frm), None, direction) == want
                    null = _lib.NintFeedbackMask()
                    lib = _lib.load()
                    assert lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(TCL._fb(O, frm)), C.byref(null), direction, None, 0) == want[0]
                    seen.add((direction, "ok" if want[0] >= 0 else want[0]))
    # what the sweep met: plans in every direction, the refused backward of a fed window, the refused step-0 feeds
    assert {(FWD, "ok"), (BWD, "ok"), (ROLLOUT, "ok"), (BWD, E_ARG), (ROLLOUT, E_ARG)} <= seen
    assert ((FWD, E_ARG) in seen) == (not has_init)


@pytest.mark.parametrize("Cin,O", [(5, 1), (64, 2)], ids=["folded", "plain"])
@pytest.mark.parametrize("cyclic", [False, True])
def test_a_step_without_a_fed_image_has_no_feedback_launch_but_keeps_its_adjoint(cyclic, Cin, O):
    """T = 5, B = 3, F = 1 and step F+1 = 2 all zero.  Forward: the records are those of from = 1, and the enqueue indices of
    steps >= 2 lie lower by the one feedback launch (cyclic with a plain slab: and the xs wrap behind it) that is not there.
    Roll-out: the plan is the plan of from = 1, index for index -- the adjoint of step 2 goes out whatever its mask word."""
    T, B, L = 5, 3, 3
    tb = np.zeros((T, B), np.uint8)
    tb[1] = (1, 0, 1)
    tb[3] = (0, 0, 1)
    tb[4] = (1, 1, 1)
    strip = lambda r: {k: v for k, v in r.items() if k != "index"}
    s = TRO._train_seq(Cin, 4, cyclic, False, False, "f32", None, T=T, B=B)
    folded = bool(s.layer[0].xfold)
    n, got = _plan(s, TCL._fb(O, 0), tb, FWD)
    m, full = _plan_from(s, TCL._fb(O, 1), FWD)
    assert n == m > 0 and [strip(r) for r in got] == [strip(r) for r in full]
    gap = 1 + int(cyclic and not folded)
    assert [f["index"] - g["index"] for f, g in zip(full, got)] == [gap if r["t"] >= 2 else 0 for r in got]
    # inside the masked plan: between the last gate of step 1 and the first of step 2 nothing but (cyclic) the h wrap
    last1 = max(r["index"] for r in got if r["t"] == 1)
    first2 = min(r["index"] for r in got if r["t"] == 2)
    first3 = min(r["index"] for r in got if r["t"] == 3)
    last2 = max(r["index"] for r in got if r["t"] == 2)
    assert first2 - last1 == (2 if cyclic else 1) and first3 - last2 == (2 if cyclic else 1) + gap
    assert _plan(s, TCL._fb(O, 0), tb, ROLLOUT) == _plan_from(s, TCL._fb(O, 1), ROLLOUT)
    assert _plan(s, TCL._fb(O, 0), tb, BWD)[0] == E_ARG
    # an all-zero mask is the open loop, in every direction
    zero = np.zeros((T, B), np.uint8)
    assert _plan(s, TCL._fb(O, 0), zero, FWD) == _plan_from(s, TCL._fb(O, T), FWD)
    assert _plan(s, TCL._fb(O, 0), zero, BWD) == _plan_from(s, TCL._fb(O, T), BWD)
    assert _plan(s, TCL._fb(O, 0), zero, ROLLOUT) == _plan_from(s, TCL._fb(O, T), ROLLOUT)
    # F is the first step with a fed image: steps [0, 3) of a mask that starts at 3 are the open-loop plan of from = 3
    late = np.zeros((T, B), np.uint8)
    late[3, 1] = 1
    n, got = _plan(s, TCL._fb(O, 0), late, FWD)
    m, full = _plan_from(s, TCL._fb(O, 3), FWD)
    assert [r for r in got if r["t"] <= 3] == [r for r in full if r["t"] <= 3]
    assert [strip(r) for r in got] == [strip(r) for r in full]


# ------------------------------------------------------------------ refusals of the library, before any launch
def test_mask_refusals_before_any_launch():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    T, B = STACK3["T"], STACK3["B"]
    fb = TCL._fb(1, 2)

    def rg():
        r = _lib.NintFeedbackGrad()
        r.dpred, r.dx_step = 1 << 28, 1 << 29
        return r

    def all_of(s, tb, direction):
        """the plan entry and the driver of a direction agree (made-up pointers: no call reaches a launch)"""
        fm, keep = _mask(tb)
        a = lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(fb), C.byref(fm), direction, None, 0)
        if a >= 0:              # (a pass that is in order would be enqueued: the plan entry alone)
            return a
        if direction == FWD:
            b = lib.nint_seq_fwd_sampled(C.byref(s), C.byref(fb), C.byref(fm), None)
        elif direction == ROLLOUT:
            b = lib.nint_seq_bwd_rollout_sampled(C.byref(s), C.byref(fb), C.byref(fm), C.byref(rg()), None)
        else:
            return a
        assert a == b, (a, b)
        return a

    ok = _suffix(T, B, 2)
    s = TRO._train_seq()
    assert lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(fb), C.byref(_mask(ok)[0]), FWD, None, 0) > 0
    assert lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(fb), C.byref(_mask(ok)[0]), ROLLOUT, None, 0) > 0
    for direction in (-1, 3):
        assert lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(fb), C.byref(_mask(ok)[0]), direction, None, 0) == E_ARG
    # a byte other than 0 or 1 -- wherever it stands, also in a step that would otherwise be unfed
    for t, b in ((0, 0), (1, 1), (T - 1, B - 1)):
        bad = ok.copy()
        bad[t, b] = 2
        for direction in (FWD, BWD, ROLLOUT):
            assert all_of(s, bad, direction) == E_ARG, (t, b, direction)
    # step 0 fed without a state; with one the forward pass takes it and the roll-out still refuses (today's from == 0)
    zero = ok.copy()
    zero[0, 1] = 1
    assert all_of(s, zero, FWD) == E_ARG and all_of(s, zero, ROLLOUT) == E_ARG
    s.has_init_state = 1
    assert all_of(s, zero, FWD) > 0 and all_of(s, zero, ROLLOUT) == E_ARG and all_of(s, zero, BWD) == E_ARG
    # the feedback's own refusals come first, the backward fields' before the feedback's in the roll-out
    s = TRO._train_seq()
    for badfb in (TCL._fb(-1, 2), TCL._fb(6, 2), TCL._fb(1, 2, w=None)):
        fm, keep = _mask(ok)
        for direction in (FWD, ROLLOUT):
            assert lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(badfb), C.byref(fm), direction, None, 0) == E_ARG
    s.dh_seq = (1 << 31) + 8
    bad = ok.copy()
    bad[1, 0] = 2
    assert all_of(s, bad, ROLLOUT) == E_ALIGN and all_of(s, bad, FWD) == E_ARG
    # B = 65: NINT_E_SHAPE with a mask, with everything else in order; unlimited without one
    big = TRO._train_seq(B=65)
    assert all_of(big, _suffix(T, 65, 2), FWD) == E_SHAPE and all_of(big, _suffix(T, 65, 2), ROLLOUT) == E_SHAPE
    assert all_of(big, _suffix(T, 65, T), FWD) == E_SHAPE            # (nothing fed: the mask is still one of 65 images)
    wrong = _suffix(T, 65, 2)
    wrong[2, 64] = 3
    assert all_of(big, wrong, FWD) == E_ARG                          # ... and the argument checks come first
    assert lib.nint_debug_seq_plan_sampled(C.byref(big), C.byref(fb), None, FWD, None, 0) > 0
    assert lib.nint_seq_fwd_sampled(None, C.byref(fb), C.byref(_mask(ok)[0]), None) == E_ARG
    ok64 = TRO._train_seq(B=64)
    assert all_of(ok64, _suffix(T, 64, 2), FWD) > 0 and all_of(ok64, _suffix(T, 64, 2), ROLLOUT) > 0
    # a mask beside a head of no outputs says nothing: the open loop
    assert lib.nint_debug_seq_plan_sampled(C.byref(s), C.byref(TCL._fb(0, 0, w=None)), C.byref(_mask(bad)[0]), FWD, None, 0) > 0


def test_sel_entries_refuse_bad_arguments_before_any_launch():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 13, 37, 2) == 0
    # made-up addresses, the first slab misaligned by default: NINT_E_ALIGN is the last check of the unmasked entries but the
    # shape rule, so a call that returns it has passed their argument checks -- and the mask is looked at after all of them
    A_, DP, DH, W_, XS = 1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 16
    fed = np.array([1, 0, 1], np.uint8)

    def bwd(dx=A_ + 8, N=3, O=1, mask=fed, Ch=8, Chp=32):
        return lib.nint_head_feedback_bwd_sel(dx, 0, DP, 0, DH, 0, N, Ch, Chp, O, W_, 4, 32, 3, 5, 0,
                                              None if mask is None else mask.ctypes.data, C.byref(g), 1, None)

    def fwd(h=A_ + 8, N=3, O=1, mask=fed, Ch=8, Chp=32):
        return lib.nint_head_feedback_sel(h, 0, N, Ch, Chp, O, W_, None, XS, 0, 4, 32, 3, 5, 0,
                                          None if mask is None else mask.ctypes.data, C.byref(g), 1, None)

    for call in (fwd, bwd):
        assert call() == E_ALIGN and call(mask=None) == E_ALIGN and call(mask=np.array([1, 2, 0], np.uint8)) == E_ALIGN
        assert call(O=0) == E_ARG and call(N=0) == E_ARG
        assert call(A_, mask=None) == E_ARG
        assert call(A_, mask=np.array([1, 2, 0], np.uint8)) == E_ARG and call(A_, mask=np.array([0, 0, 255], np.uint8)) == E_ARG
        assert call(A_, Ch=130, Chp=160) == E_SHAPE                              # the kernels' own shape rule
        assert call(A_, N=65, mask=np.ones(65, np.uint8)) == E_SHAPE             # more images than the word has bits
        many = np.ones(65, np.uint8)
        many[64] = 2
        assert call(A_, N=65, mask=many) == E_ARG
    # no image fed: the forward entry has nothing to launch (the backward one would launch the plain head backward)
    assert fwd(A_, mask=np.zeros(3, np.uint8)) == 0


def test_structs_entries_and_version():
    from nasa_niswan_amd import _lib
    M = _lib.NintFeedbackMask
    assert (M.fed.offset, C.sizeof(M)) == (0, 8)
    lib = _lib.load()
    assert lib.nint_version() == 113
    for name in ("nint_seq_fwd_sampled", "nint_seq_bwd_rollout_sampled", "nint_debug_seq_plan_sampled", "nint_head_feedback_sel",
                 "nint_head_feedback_bwd_sel"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    TRO.test_structs_and_version()              # nint_seq, nint_feedback and nint_feedback_grad are what they were


# ------------------------------------------------------------------ the CPU model
@pytest.mark.parametrize("storage", ["f32", "bf16", None])
@pytest.mark.parametrize("cyclic", [False, True])
def test_a_suffix_mask_is_the_rollout_model_exactly(cyclic, storage):
    c, p = SMALL, TCL._params(SMALL)
    X = TCL._x(c)
    g = torch.Generator().manual_seed(2)
    dpred = torch.randn(c["B"], c["O"], c["H"], c["W"], generator=g, dtype=torch.float64)
    dseq = torch.randn(c["B"], c["T"] * c["O"], c["H"], c["W"], generator=g, dtype=torch.float64)
    for s in (1, 2, c["T"] - 1, c["T"]):
        a = SM.grads(X, p, SM.suffix(c["B"], c["T"], s), cyclic, storage, dpred, dseq)
        b = RM.grads(X, p, s, cyclic, storage, dpred, dseq)
        for k in ("pred", "seq", "x_fed", "dx"):
            assert torch.equal(a[k], b[k]), (s, k)
        assert all(torch.equal(a["params"][k], b["params"][k]) for k in p), s
    a = SM.grads(X, p, None, cyclic, storage, dpred, dseq)
    b = RM.grads(X, p, None, cyclic, storage, dpred, dseq)
    assert torch.equal(a["dx"], b["dx"]) and all(torch.equal(a["params"][k], b["params"][k]) for k in p)
    with pytest.raises(ValueError):
        SM.forward(X, p, SM.suffix(c["B"], c["T"], 0))


def test_a_masked_pass_is_the_open_loop_on_its_fed_input_and_dx_is_zero_where_fed():
    c, p = SMALL, TCL._params(SMALL)
    X = TCL._x(c)
    fed = torch.tensor([[0, 1, 0, 1], [0, 0, 1, 0]], dtype=torch.bool)
    g = torch.Generator().manual_seed(2)
    dseq = torch.randn(c["B"], c["T"] * c["O"], c["H"], c["W"], generator=g, dtype=torch.float64)
    a = SM.grads(X, p, fed, True, "bf16", None, dseq)
    b = SM.forward(a["x_fed"], p, None, True, "bf16")
    assert torch.equal(a["seq"], b["seq"])
    c0 = c["C"] - c["O"]
    sub = a["dx"][:, :, c0:]
    assert not bool(sub[fed].any()) and bool(sub[~fed].flatten(1).any(dim=1).all())
    keep = ~fed.view(c["B"], c["T"], 1, 1, 1).expand_as(X[:, :, c0:])
    assert torch.equal(a["x_fed"][:, :, :c0], X[:, :, :c0]) and torch.equal(a["x_fed"][:, :, c0:][keep], X[:, :, c0:][keep])


@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("case", sorted(SM.CASES))
def test_the_gpu_cases_separate_the_mask_from_both_neighbours(case, cyclic):
    """what tests/test_gpu_sampled.py relies on: under its mask every parameter's gradient is more than two f32 gates from the
    teacher-forced gradient on the same input AND from the full roll-out gradient (from = 1), so a device that fed nothing, or
    every image, or dropped or kept a fed term it should not, cannot pass"""
    sm, tf, ro = SM.reference(case, cyclic)
    assert torch.equal(sm["seq"], tf["seq"]) and not torch.equal(sm["seq"], ro["seq"])
    for other, name in ((tf, "teacher-forced"), (ro, "roll-out")):
        sep = RM.separation(sm, other)
        assert min(a for a, _ in sep.values()) > 2, (name, sep)


# ------------------------------------------------------------------ the host surface, where it needs no device
def test_the_trainers_draw():
    from nasa_niswan_amd.trainer import FusedTrainer as FT
    T, B, s = 6, 5, 2
    a = [FT.draw_mask(g, T, B, s, 0.5) for g in [FT.sampler(7, 0)] for _ in range(3)]
    b = [FT.draw_mask(g, T, B, s, 0.5) for g in [FT.sampler(7, 0)] for _ in range(3)]
    other = [FT.draw_mask(g, T, B, s, 0.5) for g in [FT.sampler(7, 1)] for _ in range(3)]
    assert all(torch.equal(u, v) for u, v in zip(a, b)), "reproducible"
    assert any(not torch.equal(u, v) for u, v in zip(a, other)), "another rank, another draw"
    assert all(torch.equal(u, v) for u, v in zip(other, [FT.draw_mask(g, T, B, s, 0.5) for g in [FT.sampler(8, 0)] for _ in range(3)]))
    for m in a + other:
        assert m.dtype == torch.bool and tuple(m.shape) == (T, B) and not bool(m[:s].any())
    assert not torch.equal(a[0], a[1]) and any(bool(m[s:].any()) and not bool(m[s:].all()) for m in a)
    # the draw is rand((T, B)) < p of that generator: p = 1 is the suffix, p = 0 feeds nothing
    g = FT.sampler(7, 0)
    want = torch.rand((T, B), generator=FT.sampler(7, 0)) < 0.5
    want[:s] = False
    assert torch.equal(FT.draw_mask(g, T, B, s, 0.5), want)
    assert torch.equal(FT.draw_mask(g, T, B, s, 1.0), SM.suffix(B, T, s).t()) and not bool(FT.draw_mask(g, T, B, s, 0.0).any())


def test_module_keyword_and_refusals():
    import nasa_niswan_amd as pkg
    net = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2, feedback=True)
    x = torch.zeros(2, 3, 6, 8, 8)
    M = torch.tensor([[0, 1, 0], [0, 0, 1]], dtype=torch.bool)
    with pytest.raises(TypeError):
        net(x, None, False, None, True, M)                                           # keyword-only
    with pytest.raises(ValueError, match="exclusive"):
        net(x, free_from=1, free_mask=M)
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(x, free_mask=M)                                                          # grad without feedback_grad
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(x, free_mask=M.numpy().astype(np.uint8), feedback_grad=False)
    with pytest.raises(RuntimeError, match="no CPU path"):                           # past the refusals: the device check
        net(x, free_mask=M, feedback_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):                           # an all-zero mask is the open loop
        net(x, free_mask=torch.zeros(2, 3, dtype=torch.bool))
    M0 = torch.tensor([[0, 1, 0], [1, 0, 1]], dtype=torch.bool)
    with pytest.raises(ValueError, match="pass a state"):
        net(x, free_mask=M0, feedback_grad=True)                                     # column 0 set without a state
    h = [(torch.zeros(2, 8, 8, 8, requires_grad=True), torch.zeros(2, 8, 8, 8)), (torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8))]
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(x, h, free_mask=M0, feedback_grad=True)                                  # column 0 set under grad stays refused
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        net(x, h, free_mask=M0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(x, h, free_mask=M, feedback_grad=True)
    for bad in (M.t(), M.float(), M[:1], torch.tensor([[0, 2, 0], [0, 0, 1]], dtype=torch.uint8)):
        with pytest.raises(ValueError, match="feed mask"):
            net(x, free_mask=bad, feedback_grad=True)
    plain = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2)
    with pytest.raises(ValueError, match="feedback=True"):
        plain(x, free_mask=M, feedback_grad=True)
    with torch.no_grad(), pytest.raises(ValueError, match="at most 64 images"):
        net(torch.zeros(65, 3, 6, 8, 8), free_mask=torch.ones(65, 3, dtype=torch.bool)[:, :].logical_and(torch.arange(3) >= 1))


def test_trainer_and_train_py_refusals(tmp_path, capsys):
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd import train as T
    from nasa_niswan_amd._lib import NintError
    from nasa_niswan_amd.trainer import FusedTrainer
    net = pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2, feedback=True)
    with pytest.raises(ValueError, match="sampling_prob needs rollout_from"):
        FusedTrainer(net, sampling_prob=0.5)
    for bad in (-0.1, 1.5, True, float("nan")):
        with pytest.raises(ValueError, match="sampling_prob must be a probability"):
            FusedTrainer(net, rollout_from=1, sampling_prob=bad)
    with pytest.raises(ValueError, match="rollout_from must be a step index >= 1"):   # the other refusals are rollout_from's
        FusedTrainer(net, rollout_from=0, sampling_prob=0.5)
    with pytest.raises(ValueError, match="rollout_from with stateful"):
        FusedTrainer(net, rollout_from=1, sampling_prob=0.5, stateful=True)
    with pytest.raises(ValueError, match="feedback=True"):
        FusedTrainer(pkg.ConvLSTM(6, [8, 4], [3, 3], 2, out_channels=2), rollout_from=1, sampling_prob=0.5)
    for kw in (dict(rollout_from=1, sampling_prob=0.5), dict(rollout_from=2, sampling_prob=0.0, sampling_seed=3),
               dict(rollout_from=1, sampling_prob=1.0), dict(rollout_from=1, sampling_prob=None)):
        with pytest.raises(NintError, match="needs the model on the MI355X"):         # past the refusals: the device check
            FusedTrainer(net, **kw)
    snap = tmp_path / "s"
    base = ["--model", "LSTM-x", "--grid", "28", "32", "--input-size", "28", "32", "--snapshot-dir", str(snap), "--tracer-input"]
    for extra, flag in ((["--sampling-prob", "0.5"], "--sampling-prob"), (["--rollout-from", "1", "--sampling-prob", "1.5"], "--sampling-prob"),
                        (["--rollout-from", "1", "--sampling-ramp-epochs", "2"], "--sampling-ramp-epochs"),
                        (["--rollout-from", "1", "--sampling-prob", "0.5", "--sampling-ramp-epochs", "-1"], "--sampling-ramp-epochs")):
        with pytest.raises(SystemExit):
            T.get_arguments(base + extra)
        assert flag in capsys.readouterr().err and not snap.exists()
    args = T.get_arguments(base + ["--rollout-from", "2", "--sampling-prob", "0.8", "--sampling-ramp-epochs", "4"])
    assert (args.rollout_from, args.sampling_prob, args.sampling_ramp_epochs) == (2, 0.8, 4)
    assert T.get_arguments(base + ["--rollout-from", "2"]).sampling_prob is None
    # the ramp: linear from 0 to P over the first E epochs, P from then on; no ramp: P from the first epoch
    assert [T.sampling_prob_of(e, 0.8, 4) for e in range(6)] == pytest.approx([0.0, 0.2, 0.4, 0.6, 0.8, 0.8])
    assert [T.sampling_prob_of(e, 0.8, 0) for e in range(2)] == [0.8, 0.8] and T.sampling_prob_of(3, None, 0) is None


# ------------------------------------------------------------------ the random-shape screen's scheduled-sampling mode
def test_sampled_fuzz_seeds_contain_what_the_mode_exists_for():
    from nasa_niswan_amd import _lib
    import test_gpu_fuzz_sampled as FZ
    tool = TRO._fuzz_tool()
    args = tool.parse(FZ.RUN)
    assert args.mode == "sampled"
    cases = tool.draw_cases(args.seed, args.n, args.mode)
    lib = _lib.load()
    folded = lambda c: c["fold"] and bool(lib.nint_xfold_pays(c["C"], c["ks"][0], 1 if c["dtype"] == "bf16" else 0))
    masks = {c["it"]: np.array(c["mask"], bool) for c in cases}
    assert all(masks[c["it"]].shape == (c["B"], c["T"]) and 1 <= c["out"] <= c["C"] for c in cases)
    assert all(c["with_state"] or not masks[c["it"]][:, 0].any() for c in cases), "step 0 is fed only from a state"
    grad = [c for c in cases if masks[c["it"]].any() and not masks[c["it"]][:, 0].any()]      # checked through the backward pass
    any_t = lambda c: masks[c["it"]].any(axis=0)
    assert any((any_t(c) & ~masks[c["it"]].all(axis=0)).any() for c in grad), "a mixed step"
    assert any((~any_t(c)[int(any_t(c).argmax()):]).any() for c in grad), "an empty step behind F"
    assert any((~masks[c["it"]].any(axis=1)).any() for c in grad), "an image that is never fed"
    assert any(folded(c) for c in grad) and any(not folded(c) for c in grad), "folded and plain inputs"
    assert any(c["cyclic"] for c in grad) and any(not c["cyclic"] for c in grad), "both boundaries"
    assert {c["dtype"] for c in grad} == {"f32", "bf16"} and {c["cot"] for c in grad} == {"seq", "last"}
    assert any(c["with_state"] for c in grad), "gradients from a given state"
    assert any(masks[c["it"]][:, 0].any() for c in cases), "step 0 fed from a state (forward only)"
    assert any(not masks[c["it"]].any() for c in cases), "nothing fed"
    # the mode has a tuple and a stream key of its own: the pinned lists are what they were, and a case replays alone
    assert tool.ALL_STREAM_MODES == tool.STREAM_MODES + ("rollout",) and "sampled" not in tool.ALL_STREAM_MODES
    assert tool.SAMPLED_MODES == ("sampled",)
    assert tool.draw_case(tool.case_rng(2008, "sampled", 5), 5, "sampled") == cases[5]
    a = tool.case_rng(7, "sampled", 3).standard_normal(4)
    assert np.array_equal(a, np.random.default_rng([7, tool.SAMPLED_KEY, 3]).standard_normal(4))
    for pos, mode in enumerate(tool.ALL_STREAM_MODES):
        assert np.array_equal(tool.case_rng(7, mode, 3).standard_normal(4), np.random.default_rng([7, 1 + pos, 3]).standard_normal(4))
    # --self-check is a mode of --sampled, --list needs no device
    assert tool.parse(FZ.RUN + ["--self-check"]).self_check
