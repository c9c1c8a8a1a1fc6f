"""The residual head without a GPU: the CPU model (tests/residual_model.py) against itself -- closed loop = open
loop over the fed input, the written-out g recursion = CPU autograd, and the SEPARATION that makes the device's gradient tests
mean something --, the C ABI of the new structure and entries, and every refusal that needs no device."""
import ctypes as C
import json
import os
import subprocess

import pytest
import torch

import closed_loop_model as CLM
import residual_model as RES
import rollout_model as RM
import sampled_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEDS = {"from-1": 1, "from-2": 2, "mask": RES.MASK}


def _inputs(case, dtype=torch.float32):
    c = RES.CASES[case]
    return c, RES.case_data(c), RES.case_params(c, dtype)


# ------------------------------------------------------------------ the model against itself
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(RES.CASES))
def test_closed_pass_equals_open_pass_over_the_fed_input(case, storage):
    """the contract of 4.18 carries over: the base of a fed step is the fed value, so the residual closed loop equals, bit for
    bit, the residual open loop over x_fed -- outputs, states, and x_fed itself; and a head of zeros stands still"""
    c, d, p = _inputs(case)
    T = c["T"]
    for fed in (1, T - 1, RES.MASK[:, :T] if c["B"] == 2 else 1):
        a = RES.forward(d["X"], p, fed, False, storage)
        o = RES.forward(a["x_fed"], p, None, False, storage)
        for k in ("pred", "seq", "x_fed"):
            assert torch.equal(a[k], o[k]), (case, storage, k)
        assert all(torch.equal(u, v) for u, v in zip(a["hs"] + a["cs"], o["hs"] + o["cs"]))
        assert not torch.equal(a["x_fed"], d["X"])
    z = {k: (torch.zeros_like(v) if k.startswith("conv.") else v) for k, v in p.items()}
    r = RES.forward(d["X"], z, 1, False, storage)
    O_, C_ = c["O"], c["C"]
    first = CLM.round_et(d["X"][:, 0, C_ - O_:], storage)      # p_0 = x_0's tracer; every later step is fed its rounding
    assert torch.equal(r["seq"].view(c["B"], T, O_, c["H"], c["W"])[:, 1:], first.unsqueeze(1).expand(-1, T - 1, -1, -1, -1))


def test_a_fed_step_0_is_refused_by_the_model():
    c, d, p = _inputs("thin")
    with pytest.raises(ValueError, match="step 0 is never fed"):
        RES.forward(d["X"], p, 0)


@pytest.mark.parametrize("cyclic", [False, True], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("fed", sorted(FEDS))
@pytest.mark.parametrize("case", ["thin", "wide", "single", "all"])
def test_the_g_recursion_reproduces_autograd(case, fed, cyclic):
    """g_{u-1} = l_{u-1} + fed[u] * (xi_u + g_u), every step differentiated by itself and the steps tied by hand, gives CPU
    autograd's gradients of the whole model to f64 rounding: parameters, and dx with + g_t on the unfed feedback channels and
    zeros on the fed ones.  Without the g_u term it does not (the separation test below says by how much)."""
    c, d, p = _inputs(case, torch.float64)
    f = FEDS[fed]
    X = d["X"].double()
    want = RES.grads(X, p, f, cyclic, "f32", dpred=d["dpred"], dseq=d["dseq"])
    got = RES.recursion(X, p, f, cyclic, "f32", dpred=d["dpred"], dseq=d["dseq"])
    tol = lambda ref: 1e-11 * float(ref.abs().max()) + 1e-13
    for k, g in want["params"].items():
        assert float((got["params"][k] - g).abs().max()) <= tol(g), (case, fed, k)
    assert float((got["dx"] - want["dx"]).abs().max()) <= tol(want["dx"])
    m = RES.fed_mask(f, c["B"], c["T"])
    c0 = c["C"] - c["O"]
    assert not bool(want["dx"][:, :, c0:][m].any())                                  # fed (b, t): exact zeros
    # the skip add is what the unfed feedback channels hold beyond the stack's own d/dx: take it away and they differ
    g_bt = got["g"].transpose(0, 1)
    assert float(g_bt[~m].abs().max()) > 0
    # the non-residual model's dx has no such term
    nr = SM.grads(X, p, m, cyclic, "f32", dpred=d["dpred"], dseq=d["dseq"])
    assert float((nr["dx"] - want["dx"])[:, :, c0:][~m].abs().max()) > 1e-3 * float(want["dx"].abs().max())


@pytest.mark.parametrize("fed", sorted(FEDS))
@pytest.mark.parametrize("case", sorted(CLM.CASES))
def test_separation_of_the_three_gradients(case, fed):
    """SEPARATION: with the cases' weights and cotangents the residual roll-out gradient of EVERY parameter is more than two of
    the standing gates (f32: 1e-3 * max|g| + 1e-6 max-abs; bf16: rel-L2 2e-2 -- tests/rollout_model.py) away from the gradient
    with the `+ g_u` skip term dropped and from the non-residual model's gradient, in both measures.  A device backward that
    forgot the skip term, or ran the non-residual kernels, therefore cannot pass tests/test_gpu_residual.py.  Asserted for every
    case of closed_loop_model.CASES (the issue asks for one per storage type; the CPU reference is the f32 model for both)."""
    res, noskip, nonres = RES.reference(case, False, FEDS[fed])
    for name, other in (("without the skip term", noskip), ("non-residual", nonres)):
        sep = RES.separation(res, other)
        worst = {k: min(v) for k, v in sep.items()}
        print(f"  {case} {fed} {name}: min over parameters {min(worst.values()):.1f} gates "
              f"(f32 {min(v[0] for v in sep.values()):.1f}, bf16 {min(v[1] for v in sep.values()):.1f})")
        for k, (f32_gates, bf16_gates) in sep.items():
            assert f32_gates > 2 and bf16_gates > 2, (case, fed, name, k, f32_gates, bf16_gates)


# ------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ["nint_head_fwd_res", "nint_head_fwd_seq_res", "nint_head_loss_fused_res", "nint_head_loss_seq_fused_res",
               "nint_head_feedback_res", "nint_head_feedback_bwd_res", "nint_seq_fwd_residual", "nint_seq_bwd_rollout_residual"]


def test_head_base_layout_and_the_new_symbols(tmp_path):
    """nint_head_base against a compiled C snippet, as tests/test_abi.py does for the other structures; the eight entries are
    exported, bound, and declared; no existing structure moved"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    prog = tmp_path / "sz.c"
    fields = ["xs", "x_n0", "Cx", "Cxp", "c0", "xfold_k"]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nint.h"\nint main(){printf("%zu %zu %zu %zu'
                    + " %zu" * len(fields) + '\\n",sizeof(nint_head_base),sizeof(nint_feedback),sizeof(nint_feedback_grad),'
                    'sizeof(nint_feedback_mask),' + ",".join(f"offsetof(nint_head_base,{f})" for f in fields) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_lib.NintHeadBase), C.sizeof(_lib.NintFeedback), C.sizeof(_lib.NintFeedbackGrad), C.sizeof(_lib.NintFeedbackMask)]
    want += [getattr(_lib.NintHeadBase, f).offset for f in fields]
    assert got == want and got[0] == 32


def _base(xs=16, x_n0=0, Cx=4, Cxp=16, c0=3, k=0):
    from nasa_niswan_amd import _lib
    hb = _lib.NintHeadBase()
    hb.xs, hb.x_n0, hb.Cx, hb.Cxp, hb.c0, hb.xfold_k = xs, x_n0, Cx, Cxp, c0, k
    return hb


def test_the_base_checks_come_before_any_launch():
    """argument validation needs no device: the twin's checks first, then the base's -- every code on made-up pointers"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 13, 37, 2) == 0
    E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4
    fwd = lambda hb, h=16, Chp=16, O_=1, dt=0: lib.nint_head_fwd_res(h, 0, 2, 8, Chp, O_, 16, None, 16, C.byref(g), dt, C.byref(hb), None)
    seq = lambda hb, h=16: lib.nint_head_fwd_seq_res(h, 2, 3, 8, 16, 1, 16, None, 16, C.byref(g), 0, C.byref(hb), None)
    for call in (fwd, seq):
        assert call(_base(x_n0=-1)) == E_ARG
        assert call(_base(Cx=0)) == E_ARG
        assert call(_base(c0=4)) == E_ARG                    # c0 + O > Cx
        assert call(_base(c0=-1)) == E_ARG
        assert call(_base(k=2)) == E_ARG and call(_base(k=-1)) == E_ARG
        assert call(_base(k=5)) == E_ARG                     # Cxp < k * Cx
        assert call(_base(Cxp=18)) == E_ARG                  # 72 bytes per pixel
        assert call(_base(xs=24)) == E_ALIGN
    assert lib.nint_head_fwd_res(None, 0, 2, 8, 16, 1, 16, None, 16, C.byref(g), 0, C.byref(_base(c0=9)), None) == E_ARG   # the twin's first
    assert seq(_base(xs=24), h=24) == E_ALIGN                # (the twin's alignment check)
    assert fwd(_base(), Chp=144) == E_SHAPE                  # beyond the staged rule: the wide kernels have no residual form
    # the fused twins: the spec entry's checks in its order, then the base's
    sp = _lib.NintLossSpec()
    sp.mse, sp.l1, sp.huber, sp.delta = 1.0, 1.0, 0.0, 1.0
    fused = lambda hb, spec=sp, Chp=16, lo=16: lib.nint_head_loss_fused_res(16, 0, 2, 8, Chp, 1, 16, None, 16, None, 0.0, C.byref(spec), 16, 16, lo,
                                                                            None, C.byref(g), 2, 3, 9, 31, 0, C.byref(hb), None)
    fseq = lambda hb, spec=sp, Chp=16, lo=16: lib.nint_head_loss_seq_fused_res(16, 2, 3, 8, Chp, 1, 16, None, 16, None, 0.0, C.byref(spec), 16, 16,
                                                                               lo, None, C.byref(g), 2, 3, 9, 31, 0, C.byref(hb), None)
    bad = _lib.NintLossSpec()
    for call in (fused, fseq):
        assert call(_base(c0=4)) == E_ARG and call(_base(xs=24)) == E_ALIGN
        assert call(_base(c0=4), spec=bad) == E_ARG          # all coefficients zero
        assert call(_base(c0=4), Chp=160) in (E_SHAPE, E_ARG) and call(_base(xs=24), lo=20) == E_ALIGN
    assert fused(_base(c0=4), Chp=160) == E_SHAPE            # (the twin's shape check stands before the base's)
    # the feedback launch and its adjoint: the ranges read and written lie apart
    fb = lambda x_n0, base_n0, fed=None, N=2: lib.nint_head_feedback_res(16, 0, N, 8, 16, 1, 16, None, 32, x_n0, 4, 16, 3, 0, 0, base_n0, fed,
                                                                        C.byref(g), 0, None)
    assert fb(2, 1) == E_ARG and fb(2, 3) == E_ARG and fb(0, 1) == E_ARG
    two = (C.c_uint8 * 2)(1, 2)
    assert fb(2, 0, two) == E_ARG                            # a mask byte other than 0 / 1
    assert fb(70, 0, (C.c_uint8 * 65)(), 65) == E_SHAPE
    fbb = lambda p_n0, pn, fed=None: lib.nint_head_feedback_bwd_res(16, 0, 16, p_n0, 16, 0, 2, 8, 16, 1, 16, 4, 16, 3, 0, 0, pn, fed, C.byref(g), 0, None)
    assert fbb(0, 1) == E_ARG and fbb(2, 1) == E_ARG and fbb(2, 3) == E_ARG
    assert fbb(0, 2, two) == E_ARG


def test_a_fed_step_0_is_refused_by_the_library():
    """nint_seq_fwd_residual: NINT_E_ARG for a fed image at step 0, with an initial state too -- where nint_seq_fwd_sampled gets
    as far as the first launch's own checks (the structure of tests/test_abi.py: a valid k = 1 layer on a misaligned x slab)"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    seq = _lib.NintSeq()
    seq.L, seq.B, seq.T, seq.dtype, seq.xs, seq.h[0], seq.c[0] = 1, 2, 3, 0, 8, 16, 16
    seq.layer[0].k, seq.layer[0].Cx, seq.layer[0].Cxp, seq.layer[0].Ch, seq.layer[0].Ch16, seq.layer[0].Chp = 1, 4, 16, 8, 16, 16
    assert lib.nint_geom_make(C.byref(seq.g), 13, 37, 0) == 0
    seq.has_init_state = 1
    fb = _lib.NintFeedback()
    fb.w, fb.O, fb.from_step = 16, 1, 0
    E_ARG = -1
    first = lib.nint_seq_fwd_sampled(C.byref(seq), C.byref(fb), None, None)
    assert first != 0 and lib.nint_seq_fwd_residual(C.byref(seq), C.byref(fb), None, None) == E_ARG
    fb.from_step = 1
    assert lib.nint_seq_fwd_residual(C.byref(seq), C.byref(fb), None, None) == lib.nint_seq_fwd_sampled(C.byref(seq), C.byref(fb), None, None) != E_ARG
    fm = _lib.NintFeedbackMask()
    bytes_ = (C.c_uint8 * 6)(0, 1, 0, 0, 1, 1)              # (t, b) = (0, 1) fed
    fm.fed = C.addressof(bytes_)
    assert lib.nint_seq_fwd_residual(C.byref(seq), C.byref(fb), C.byref(fm), None) == E_ARG
    bytes_[1] = 0
    assert lib.nint_seq_fwd_residual(C.byref(seq), C.byref(fb), C.byref(fm), None) != E_ARG


# ------------------------------------------------------------------ host layers
def test_module_refusals_need_no_device():
    import nasa_niswan_amd as pkg
    with pytest.raises(ValueError, match="needs feedback=True"):
        pkg.ConvLSTM(4, [8], [3], 1, residual=True)
    net = pkg.ConvLSTM(4, [8], [3], 1, out_channels=1, feedback=True, residual=True)
    plain = pkg.ConvLSTM(4, [8], [3], 1, out_channels=1, feedback=True)
    assert list(net.state_dict()) == list(plain.state_dict()) and net.residual and not plain.residual
    x = torch.zeros(2, 3, 4, 8, 8)
    st = [(torch.zeros(2, 8, 8, 8), torch.zeros(2, 8, 8, 8))]
    with pytest.raises(ValueError, match="step 0 cannot be fed"):
        net(x, st, free_from=0)
    with pytest.raises(ValueError, match="no input precedes the window"):
        net(x, st, free_mask=torch.tensor([[1, 0, 0], [0, 0, 0]], dtype=torch.bool))
    with pytest.raises(ValueError, match="pass a state"):
        plain(x, free_from=0)                               # (the non-residual module keeps its own message)


def test_train_py_flag_and_the_resume_rule(tmp_path, monkeypatch):
    from nasa_niswan_amd import train as T
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    base = ["--model", "LSTM-r", "--in-channels", "5", "--hidden-channels", "8", "--kernel-size", "3", "--num-layers", "1",
            "--sequence-length", "4", "--input-size", "12", "16", "--grid", "12", "16"]
    with pytest.raises(SystemExit):
        T.get_arguments(base + ["--residual-head", "--snapshot-dir", str(tmp_path / "a")])        # needs --tracer-input
    args = T.get_arguments(base + ["--tracer-input", "--residual-head", "--snapshot-dir", str(tmp_path / "b")])
    assert args.residual_head and json.load(open(tmp_path / "b" / "configurations.json"))["residual_head"] is True
    assert T.checkpoint_residual_head(str(tmp_path / "b")) is True and T.checkpoint_residual_head(str(tmp_path / "b" / "epoch-010")) is True
    old = T.get_arguments(base + ["--tracer-input", "--snapshot-dir", str(tmp_path / "c")])
    assert not old.residual_head and T.checkpoint_residual_head(str(tmp_path / "c" / "epoch-010")) is False
    assert T.checkpoint_residual_head(str(tmp_path / "nowhere" / "epoch-010")) is None
    resume = base + ["--tracer-input", "--residual-head", "--use-checkpoint", "--restore-from", str(tmp_path / "c" / "epoch-010"),
                     "--snapshot-dir", str(tmp_path / "d")]
    with pytest.raises(SystemExit):
        T.get_arguments(resume)                             # trained without it
    assert T.get_arguments(resume + ["--reset-optimizer"]).residual_head
    ok = [a if a != str(tmp_path / "c" / "epoch-010") else str(tmp_path / "b" / "epoch-010") for a in resume]
    assert T.get_arguments(ok).residual_head                # trained with it: resumes


def test_fuzz_seeds_cover_the_branches():
    """the fixed seeds of tests/test_gpu_fuzz_residual.py hold a folded, a plain, a cyclic and a masked case (and an f32 and a
    bf16 one): drawn on the host, no device asked for"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_shapes as FZ
    from nasa_niswan_amd import _lib
    from test_gpu_fuzz_residual import RUN, SELF_CHECK
    lib = _lib.load()
    assert RUN[-1] == "--residual" and SELF_CHECK[-2:] == ["--residual", "--self-check"] and RUN[3] == SELF_CHECK[3]
    cfgs = FZ.draw_cases(int(RUN[3]), int(RUN[1]), "residual")
    assert cfgs[:1] == FZ.draw_cases(int(SELF_CHECK[3]), int(SELF_CHECK[1]), "residual")       # a case replays by itself
    folded = [bool(c["fold"] and lib.nint_xfold_pays(c["C"], c["ks"][0], 0 if c["dtype"] == "f32" else 1)) for c in cfgs]
    assert any(folded) and not all(folded)
    assert any(c["cyclic"] for c in cfgs) and any(not c["cyclic"] for c in cfgs)
    masked = [c for c in cfgs if c["mask"] is not None]
    assert masked and len(masked) < len(cfgs)
    assert all(not any(row[0] for row in c["mask"]) for c in masked)                          # step 0 is never fed
    # a mixed step (some images fed, some not) and a window fed in full are both there, with and without a state
    assert any(any(0 < sum(col) < c["B"] for col in zip(*c["mask"])) for c in masked)
    assert any(c["mask"] is None and c["fb_from"] < c["T"] for c in cfgs)
    assert any(c["with_state"] for c in cfgs) and any(not c["with_state"] for c in cfgs)
    assert {c["dtype"] for c in cfgs} == {"f32", "bf16"}
    assert FZ.RESIDUAL_MODES == ("residual",) and FZ.SAMPLED_MODES == ("sampled",)            # (no earlier mode's stream moved)
