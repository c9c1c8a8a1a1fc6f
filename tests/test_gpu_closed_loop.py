"""GPU: the closed-loop forward -- ``ConvLSTM(feedback=True)(x, free_from=s)``, nint_seq_fwd_closed,
nint_head_feedback: from step s on the last O input channels are the head of the top layer's hidden state of the step
before, rounded once to the storage type, written on the device between two gate launches.

Shapes: closed_loop_model.CASES -- B = 2, T = 4 on a ragged 13 x 37 grid, in f32 and bf16, zero padding and cyclic longitude.
References: the open-loop pass of the library itself (bit for bit), tests/closed_loop_model.py in f64 at the tolerances of
tests/test_gpu_parity.py (f32 outputs rtol 1e-4 / atol 1e-5; bf16 rel-L2 <= 2e-2), the pack entries (bit for bit), numpy."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_model as CLM
import test_gpu_memory_contract as MC
from test_gpu_parity import assert_bf16, assert_close_out

pytestmark = pytest.mark.gpu
BOTH = ("f32", "bf16")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


def params_of(c, dtype=torch.float32, seed=3):
    from oracle import convlstm_oracle as O
    return O.synth_params(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=c["O"], seed=seed, dtype=dtype)


def data_of(c, seed=11, T=None):
    rng = np.random.default_rng(seed)
    B, T, H, W = c["B"], c["T"] if T is None else T, c["H"], c["W"]
    f = lambda *s, scale=1.0: torch.from_numpy((scale * rng.standard_normal(s)).astype(np.float32))
    return dict(X=f(B, T, c["C"], H, W), h0=[f(B, ch, H, W, scale=0.5) for ch in c["hidden"]],
                c0=[f(B, ch, H, W, scale=0.5) for ch in c["hidden"]])


def make_net(pkg, case, dtype, cyclic, gt=None, **kw):
    """the module of a case with its engine built (the plain-input case with folding off: 40 channels under k = 5 would fold)"""
    c = CLM.CASES[case]
    net = pkg.ConvLSTM(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=c["O"], compute_dtype=dtype, lon_cyclic=cyclic,
                       feedback=True, **kw).cuda()
    net.load_state_dict(params_of(c))
    if gt is not None:
        gt.guard_module(net)
    with MC.knobs(XFOLD=CLM.FOLDED[case]):
        eng = net._engine(torch.device("cuda", torch.cuda.current_device()))
    assert bool(eng.cfgs[0].xfold) == CLM.FOLDED[case]
    if gt is not None:
        MC._fill_unused_weight_tail(eng, gt.fill)
    return net, eng


def engine_run(net, eng, X, free_from, state=None, wave=None):
    """one forward pass driven through the engine, every slab kept: xs, h and c of every layer, the per-step head, pred"""
    B, T, _, H, W = X.shape
    with MC.knobs(FORCE_WAVE=wave):
        ws = eng.acquire(B, T, H, W, False, state is not None)
        try:
            net._pack_weights(eng)
            if state is not None:
                eng.load_state(ws, state)
            fb = None if free_from is None else (net.conv.weight, net.conv.bias, free_from)
            eng.forward(ws, X, feedback=fb)
            assert wave is None or ws.seq.wave == (wave if len(eng.cfgs) > 1 else 0)
            res = dict(xs=ws.xs.clone(), seq=eng.head_forward_seq(ws, net.conv.weight, net.conv.bias),
                       pred=eng.head_forward(ws, net.conv.weight, net.conv.bias), geom=(ws.g.P, ws.g.Hh, ws.g.Wh, ws.Cxp0))
            for l in range(len(eng.cfgs)):
                res[f"h{l}"], res[f"c{l}"] = ws.h[l].clone(), ws.c[l].clone()
        finally:
            eng.release(ws)
    torch.cuda.synchronize()
    return res


def substituted(c, X, seq, s):
    """X with the feedback channels of steps >= s replaced by the (f32) predictions of the step before"""
    B, T, O_ = c["B"], X.shape[1], c["O"]
    X2 = X.clone()
    X2[:, s:, c["C"] - O_:] = seq.view(B, T, O_, c["H"], c["W"])[:, s - 1:T - 1]
    return X2


# ------------------------------------------------------------------ 1. the bit contract
@pytest.mark.parametrize("cyclic", [False, True], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(CLM.CASES))
def test_closed_loop_is_the_open_loop_on_the_fed_input_bit_for_bit(pkg, case, dtype, cyclic):
    """closed loop from s = 1 and 2; then the open-loop pass over the input with the per-step predictions substituted: every
    byte of xs, every h and c slab slot of every layer and the predictions are identical -- under the engine's own wave mode,
    the merged mode 4 and the time-major mode 0"""
    c = CLM.CASES[case]
    net, eng = make_net(pkg, case, dtype, cyclic)
    X = data_of(c)["X"].cuda()
    with torch.no_grad():
        for s in (1, 2):
            for wave in (None, 4, 0):
                a = engine_run(net, eng, X, s, wave=wave)
                b = engine_run(net, eng, substituted(c, X, a["seq"], s), None, wave=wave)
                plain = engine_run(net, eng, X, None, wave=wave)
                for k in a:
                    if k != "geom":
                        assert torch.equal(a[k], b[k]), (case, dtype, cyclic, s, wave, k)
                assert not torch.equal(a["seq"], plain["seq"])                    # the loop is in fact closed
                B, O_ = c["B"], c["O"]
                assert torch.equal(a["seq"][:, :s * O_], plain["seq"][:, :s * O_])    # ... from step s on: the head of step t <= s-1 saw x alone
            # the module: the same predictions, return_state and return_sequence as in open loop
            pred = net(X, free_from=s)
            assert torch.equal(pred, engine_run(net, eng, X, s)["pred"])
        assert torch.equal(net(X, free_from=c["T"]), net(X)) and torch.equal(net(X, free_from=c["T"] + 2), net(X))


@pytest.mark.parametrize("dtype", BOTH)
def test_module_options_work_as_in_open_loop(pkg, dtype):
    c = CLM.CASES["thin"]
    net, eng = make_net(pkg, "thin", dtype, True, return_sequence=True)
    X = data_of(c)["X"].cuda()
    with torch.no_grad():
        pred, seq, st = net(X, free_from=1, return_state="device")
        a = engine_run(net, eng, X, 1)
        assert torch.equal(pred, a["pred"]) and torch.equal(seq, a["seq"])
        pred2, seq2, pairs = net(X, free_from=1, return_state=True)
        for (h, cc), (h2, c2) in zip(st.tensors(), pairs):
            assert torch.equal(h, h2) and torch.equal(cc, c2)
    # without free_from the module is the module it was, bit for bit, and it trains
    ref = pkg.ConvLSTM(c["C"], c["hidden"], c["ks"], 2, out_channels=c["O"], compute_dtype=dtype, lon_cyclic=True,
                       return_sequence=True).cuda()
    ref.load_state_dict(net.state_dict())
    outs = []
    for m in (net, ref):
        Xg = X.clone().requires_grad_(True)
        p, sq = m(Xg)
        (p.sum() + (sq * sq).sum()).backward()
        outs.append([p.detach(), sq.detach(), Xg.grad] + [q.grad for q in m.parameters()])
    assert all(torch.equal(u, v) for u, v in zip(*outs))
    # nothing fed back (free_from >= T): trains as ever
    Xg = X.clone().requires_grad_(True)
    p, sq = net(Xg, free_from=c["T"])
    (p.sum() + (sq * sq).sum()).backward()
    assert torch.equal(Xg.grad, outs[0][2])


# ------------------------------------------------------------------ 2. against the CPU model
_REF = {}


def reference(case, cyclic, s, dtype, with_state=False):
    key = (case, cyclic, s, dtype, with_state)
    if key not in _REF:
        c = CLM.CASES[case]
        d = data_of(c)
        st = dict(h0=[t.double() for t in d["h0"]], c0=[t.double() for t in d["c0"]]) if with_state else {}
        r = CLM.forward(d["X"].double(), params_of(c, torch.float64), free_from=s, cyclic=cyclic, storage=dtype, **st)
        _REF[key] = r["seq"].float()
    return _REF[key]


@pytest.mark.parametrize("cyclic", [False, True], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(CLM.CASES))
def test_predictions_of_every_step_against_the_cpu_model(pkg, case, dtype, cyclic):
    c = CLM.CASES[case]
    net, eng = make_net(pkg, case, dtype, cyclic)
    X = data_of(c)["X"].cuda()
    for s in (1, 2):
        with torch.no_grad():
            got = engine_run(net, eng, X, s)["seq"]
        want = reference(case, cyclic, s, dtype)
        assert torch.isfinite(got).all()
        if dtype == "bf16":
            assert_bf16(got, want, f"{case} from {s} seq", 2e-2)
        else:
            assert_close_out(got, want, f"{case} from {s} seq")


@pytest.mark.parametrize("cyclic", [False, True], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dtype", BOTH)
def test_from_step_zero_from_a_device_state(pkg, dtype, cyclic):
    """free_from = 0 from a non-zero device state: step 0 sees the head of the state it was handed -- against the CPU model,
    and bit for bit against the open-loop pass on the substituted input"""
    c = CLM.CASES["thin"]
    net, eng = make_net(pkg, "thin", dtype, cyclic)
    d = data_of(c)
    X = d["X"].cuda()
    with torch.no_grad():
        state = eng.state_from_tensors([(h.cuda(), cc.cuda()) for h, cc in zip(d["h0"], d["c0"])])
        a = engine_run(net, eng, X, 0, state=state)
        # the prediction fed into step 0 is the head of the handed state: slot 0 of the top layer's slab
        B, T, H, W = c["B"], c["T"], c["H"], c["W"]
        ws = eng.acquire(B, T, H, W, False, True)
        eng.load_state(ws, state)
        p0 = eng.head_forward(ws, net.conv.weight, net.conv.bias, slot=0)
        eng.release(ws)
        X2 = substituted(c, X, a["seq"], 1)
        X2[:, 0, c["C"] - c["O"]:] = p0
        b = engine_run(net, eng, X2, None, state=state)
        for k in a:
            if k != "geom":
                assert torch.equal(a[k], b[k]), (dtype, cyclic, k)
        pred, _ = net(X, state, free_from=0, return_state="device")
        assert torch.equal(pred, a["pred"])
    want = reference("thin", cyclic, 0, dtype, with_state=True)
    if dtype == "bf16":
        assert_bf16(a["seq"], want, "from 0 seq", 2e-2)
    else:
        assert_close_out(a["seq"], want, "from 0 seq")


# ------------------------------------------------------------------ 3. untouched bytes
@pytest.mark.parametrize("cyclic", [False, True], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(CLM.CASES))
def test_the_pass_writes_the_feedback_channels_and_nothing_else(pkg, case, dtype, cyclic):
    """the raw xs slab after a closed-loop pass against the one after the open-loop pass on the same input: they differ only
    in the feedback channels (folded: in each of the k copies) of interior pixels of steps >= s, and in those channels of the
    halo columns of these blocks' interior rows when a cyclic engine wraps a plain slab"""
    c = CLM.CASES[case]
    net, eng = make_net(pkg, case, dtype, cyclic)
    X = data_of(c)["X"].cuda()
    B, T, H, W, Cx, O_ = c["B"], c["T"], c["H"], c["W"], c["C"], c["O"]
    et = torch.int16 if dtype == "bf16" else torch.int32
    for s in (1, 2):
        with torch.no_grad():
            a, b = engine_run(net, eng, X, s), engine_run(net, eng, X, None)
        P, Hh, Wh, Cxp = a["geom"]
        va, vb = (r["xs"].view(et).view(T * B, Hh, Wh, Cxp) for r in (a, b))
        allowed = torch.zeros_like(va, dtype=torch.bool)
        kf = c["ks"][0] if CLM.FOLDED[case] else 1
        chans = [kx * Cx + Cx - O_ + o for kx in range(kf) for o in range(O_)]
        cols = slice(0, P + W + P) if (cyclic and kf == 1) else slice(P, P + W)
        for ch in chans:
            allowed[s * B:, P:P + H, cols, ch] = True
        diff = va != vb
        assert not bool((diff & ~allowed).any()), (case, dtype, cyclic, s)
        assert bool(diff[s * B:, P:P + H, P:P + W][..., chans].any())
        if cyclic and kf == 1:         # the wrapped halo columns of the fed blocks hold the fed values
            rows = va[s * B:, P:P + H]
            assert torch.equal(rows[:, :, :P], rows[:, :, W:W + P]) and torch.equal(rows[:, :, P + W:P + W + P], rows[:, :, P:2 * P])


@pytest.mark.parametrize("cyclic", [False, True], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", ["thin", "wide"])
def test_closed_loop_under_the_guarded_allocator(pkg, case, dtype, cyclic):
    """tests/test_gpu_memory_contract.py's three runs (plain torch, guarded zero-filled, guarded poisoned): no store outside an
    extent, no result from a byte the library did not write"""
    c = CLM.CASES[case]

    def scenario(gt):
        G = (lambda t: t) if gt is None else gt.guard_copy
        net, _ = make_net(pkg, case, dtype, cyclic, gt=gt, return_sequence=True)
        d = data_of(c)
        with torch.no_grad():
            pred, seq, st = net(G(d["X"].cuda()), free_from=1, return_state="device")
            pred0, seq0 = net(G(d["X"].cuda()), st, free_from=0)
        return dict(pred=pred, seq=seq, pred0=pred0, seq0=seq0)

    stack = (c["C"], c["hidden"], c["ks"])
    assert MC.three_runs(f"closed-loop-{case}-{dtype}-{cyclic}", scenario, MC.row_stride(stack, (c["H"], c["W"]))) > 0


# ------------------------------------------------------------------ 4. nint_head_feedback alone
def _feedback_alone(lib, ex, dt, Cx, O_, Ch, k, cyc, H=13, W=37, N=3, seed=7):
    """pack(src) then the feedback entry, against pack(src with the head's f32 output in the feedback channels)"""
    from nasa_niswan_amd._lib import stream_ptr
    es, et = (2, torch.bfloat16) if dt == 1 else (4, torch.float32)
    kc = lib.nint_kc(dt)
    rup = lambda a, b: (a + b - 1) // b * b
    Pd = 2
    g = MC._geom(lib, H, W, Pd)
    Chp, Cxp, c0 = rup(Ch, kc), rup((k or 1) * Cx, kc), Cx - O_
    gen = torch.Generator().manual_seed(seed)
    n0 = 1                                                     # the slab holds one image in front of the N that are read
    h = ex.copy((torch.randn((n0 + N) * g.Hh * g.Wh * Chp, generator=gen)).to(et))      # junk in halo and pad channels too
    w = ex.copy(torch.randn(O_, Ch, generator=gen))
    b = ex.copy(torch.randn(O_, generator=gen))
    src = torch.randn(N, 1, Cx, H, W, generator=gen)
    pred = ex.empty(N * O_ * H * W, torch.float32, slack=0)
    st = stream_ptr()
    assert lib.nint_head_fwd(MC.P(h), n0, N, Ch, Chp, O_, MC.P(w), MC.P(b), MC.P(pred), C.byref(g), dt, st) == 0
    src2 = src.cuda().clone()
    src2[:, 0, c0:] = pred[:N * O_ * H * W].view(N, O_, H, W)
    slabs = []
    for s_ in (src.cuda(), src2):
        x = ex.copy(s_.contiguous())
        slab = ex.zeros((N + 1) * g.Hh * g.Wh * Cxp * es, torch.uint8)          # one image in front here too (x_n0 = 1)
        dst = C.c_void_p(slab.data_ptr() + g.Hh * g.Wh * Cxp * es)
        if k:
            fn = lib.nint_pack_btchw_xfold_cyclic if cyc else lib.nint_pack_btchw_xfold
            assert fn(MC.P(x), dst, N, 1, Cx, k, Cxp, C.byref(g), dt, st) == 0
        else:
            assert lib.nint_pack_btchw(MC.P(x), dst, N, 1, Cx, Cxp, C.byref(g), dt, st) == 0
        slabs.append(slab)
    got, want = slabs
    assert lib.nint_head_feedback(MC.P(h), n0, N, Ch, Chp, O_, MC.P(w), MC.P(b), MC.P(got), 1, Cx, Cxp, c0, k, cyc, C.byref(g), dt,
                                  st) == 0
    torch.cuda.synchronize()
    return dict(got=got, want=want)


FB_ALONE = [("thin-folded", 4, 1, 8, 5), ("plain-straddle", 40, 3, 8, 0), ("all-folded", 3, 3, 8, 5), ("all-plain", 32, 32, 40, 0),
            ("tail-channels-64", 6, 2, 64, 3), ("chv-128", 5, 1, 72, 5)]


@pytest.mark.parametrize("cyc", [0, 1], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dt", [0, 1], ids=BOTH)
@pytest.mark.parametrize("name,Cx,O_,Ch,k", FB_ALONE, ids=[f[0] for f in FB_ALONE])
def test_head_feedback_alone_is_head_fwd_then_pack_bit_for_bit(pkg, name, Cx, O_, Ch, k, dt, cyc):
    """the stored value equals nint_head_fwd's f32 output packed by nint_pack_btchw / _xfold / _xfold_cyclic, in each layout --
    every byte of the slab, so also: nothing but the feedback channels of interior pixels moved -- on generous buffers and on
    buffers of exactly their sizes under the poisoning allocator"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    seen = {}

    def call(ex):
        r = _feedback_alone(lib, ex, dt, Cx, O_, Ch, k, cyc)
        assert torch.equal(r["got"], r["want"]), name
        seen["n"] = seen.get("n", 0) + 1
        return r
    MC.both_ways(f"head_feedback {name}", call)
    assert seen["n"] == 2


# ------------------------------------------------------------------ 5. chunking, roll-out skill, the dataset
def _tracer_dataset(period="train", n_steps=17, T=4, grid=(12, 20), **kw):
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    return SyntheticE33OMA_CRNN(period, padding=None, in_channels=6, sequence_length=T, levels=1, n_steps=n_steps, grid=grid,
                                device="cuda", tracer_input=True, **kw)


def _tracer_net(pkg, dtype, seed=5):
    from oracle import convlstm_oracle as O
    net = pkg.ConvLSTM(6, [16, 8], [5, 3], 2, out_channels=1, compute_dtype=dtype, lon_cyclic=True, feedback=True).cuda()
    net.load_state_dict(O.synth_params(6, [16, 8], [5, 3], 2, out_channels=1, seed=seed))
    return net


@pytest.mark.parametrize("dtype", BOTH)
def test_predict_stream_closed_loop_over_three_chunks_is_one_window(pkg, dtype):
    from nasa_niswan_amd.dataset import SlabBatch
    from nasa_niswan_amd.inference import predict_stream
    ds = _tracer_dataset()
    T = ds.seq_len
    net = _tracer_net(pkg, dtype)
    pred, steps, dropped = predict_stream(net, ds, lanes=1, halo=(0, 0), closed_loop=True, spinup=2)
    assert pred.shape[0] == 3 * T and int(steps[0]) == 1 and dropped == len(ds) + T - 1 - 3 * T
    eng = net._engine(pred.device)
    X = SlabBatch(ds, np.asarray([int(ds.first[0])]), 3 * T)
    H, W = ds.grid
    with torch.no_grad(), eng.window(1, 3 * T, H, W, False, False) as ws:
        net._pack_weights(eng)
        eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 2))
        whole = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(3 * T, 1, H, W)
        eng.forward(ws, X)
        open_ = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(3 * T, 1, H, W)
    assert torch.equal(pred, whole) and not torch.equal(pred[3:], open_[3:]) and torch.equal(pred[:2], open_[:2])
    # two lanes: every lane spins up on its own first chunk -- each equals its own one-lane run
    ds2 = _tracer_dataset(n_steps=30)
    two, steps2, _ = predict_stream(net, ds2, lanes=2, halo=(0, 0), closed_loop=True, spinup=2)
    K = two.shape[0] // (2 * T)
    assert K >= 2
    for lane in range(2):
        t0 = int(steps2[lane * K * T])
        Xl = SlabBatch(ds2, np.asarray([t0]), K * T)
        with torch.no_grad(), eng.window(1, K * T, H, W, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, Xl, feedback=(net.conv.weight, net.conv.bias, 2))
            one = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(K * T, 1, H, W)
        assert_close_out(two[lane * K * T:(lane + 1) * K * T], one, f"lane {lane}") if dtype == "f32" else \
            assert_bf16(two[lane * K * T:(lane + 1) * K * T], one, f"lane {lane}", 2e-2)


def test_rollout_skill_slots_are_lead_times(pkg):
    """the accumulator of rollout_skill against f64 sums over the same predictions (oracle.small_audit.skill_audit: every map
    cell and sample row within gamma(n - 1) * sum |addends|, the bound tests/test_gpu_skill.py applies), slot = lead time"""
    from oracle import small_audit as SM
    from nasa_niswan_amd.dataset import SlabBatch
    from nasa_niswan_amd.inference import lead_time_r2, rollout_skill
    ds = _tracer_dataset(n_steps=30)
    net = _tracer_net(pkg, "f32")
    H, W = ds.grid
    starts, horizon, spinup, bs = [1, 4, 9, 16, 20], 3, 2, 2
    lat = np.linspace(-80, 80, H)
    acc = rollout_skill(net, ds, starts, horizon, spinup, bs, lat=lat)
    pix, counts, sample = acc.sums()
    assert list(counts) == [len(starts)] * horizon
    eng = net._engine(torch.device("cuda", torch.cuda.current_device()))
    preds, ys, slots = [], [], []
    T = spinup + horizon
    from nasa_niswan_amd.inference import _step_targets
    for i in range(0, len(starts), bs):                   # the same batches: the same launches, the same bits
        t0s = starts[i:i + bs]
        with torch.no_grad(), eng.window(len(t0s), T, H, W, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, SlabBatch(ds, np.asarray(t0s), T), feedback=(net.conv.weight, net.conv.bias, spinup))
            seq = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(len(t0s), T, 1, H, W)
        y = _step_targets(ds, ds._device_arrays(), t0s, T)                         # (B, T, 1, H, W): the z-scored tracer
        # ... which is the record's, step for step
        want_y = np.stack([(ds.yraw[t0:t0 + T] - ds.y_mean) / ds.y_std for t0 in t0s]).astype(np.float32)
        np.testing.assert_allclose(y.cpu().numpy(), want_y, rtol=1e-6, atol=1e-6)
        preds.append(seq[:, spinup:].reshape(-1, 1, H, W).cpu().numpy())
        ys.append(y[:, spinup:].reshape(-1, 1, H, W).cpu().numpy())
        slots += list(range(horizon)) * len(t0s)
    pred_h, y_h = np.concatenate(preds), np.concatenate(ys)
    r = SM.skill_audit(pred_h, y_h, 0, 0, slots, horizon, np.cos(np.deg2rad(lat)), np.zeros_like(pix), pix, sample)
    print(f"  largest err / bound: maps {r[0]:.2e}, sample rows {r[1]:.2e}")
    assert r[0] <= 1.0 and r[1] <= 1.0
    r2 = lead_time_r2(acc)
    for j in range(horizon):
        sel = [i for i, v in enumerate(slots) if v == j]
        y = y_h[sel].astype(np.float64)
        d = pred_h[sel].astype(np.float64) - y           # (the kernel's d: one f64 subtraction)
        want = 1.0 - (d * d).sum() / ((y - y.mean()) ** 2).sum()
        assert abs(r2[j] - want) <= 1e-9 * max(1.0, abs(want)), (j, r2[j], want)
        assert acc.report(ds.y_mean, ds.y_std, slots=[j]).count == len(starts)
    with pytest.raises(ValueError, match="every start"):
        rollout_skill(net, ds, [0], horizon, spinup, bs)
    with pytest.raises(ValueError, match="every start"):
        rollout_skill(net, ds, [30 - T + 1], horizon, spinup, bs)


@pytest.mark.parametrize("dtype", BOTH)
def test_tracer_input_batches_equal_the_numpy_restatement(pkg, dtype):
    """device_batch against numpy (the tracer of step t-1, z-scored with the target statistics, as last channels: rtol / atol
    1e-6 as tests/test_gpu_static_channels.py compares its channels), slab_batch against the packed device_batch bit for bit,
    and the last channel of step t against the target of step t-1 bit for bit"""
    from oracle import preproc_oracle as PO
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    for levels, cin in ((1, 6), (2, 10)):
        from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
        T, H, W, idx = 4, 12, 20, [3, 0, 5]
        ds = SyntheticE33OMA_CRNN("train", padding=None, in_channels=cin, sequence_length=T, levels=levels, n_steps=24, grid=(H, W),
                                  device="cuda", tracer_input=True, sequence_targets=True)
        X, y = ds.device_batch(idx)
        assert X.shape == (len(idx), T, cin, H, W)
        for n, i in enumerate(idx):
            fields, _ = ds.window(i)
            t0 = int(ds.first[i])
            dyn = PO.zscore(PO.fuse_levels(*fields), ds.X_mean[:cin - levels], ds.X_std[:cin - levels])
            tr = ((ds.yraw[t0 - 1:t0 - 1 + T] - ds.y_mean) / ds.y_std).astype(np.float32)
            want = np.concatenate([dyn, tr], axis=1).astype(np.float32)
            np.testing.assert_allclose(X[n].cpu().numpy(), want, rtol=1e-6, atol=1e-6)
        yy = y if levels > 1 else y[:, :, None]
        assert torch.equal(X[:, 1:, cin - levels:], yy[:, :-1])
        eng = SeqEngine([LayerCfg(cin, 16, 5)], dtype, "cuda", lon_cyclic=True)
        B = len(idx)
        ws_a, ws_b = eng.acquire(B, T, H, W, False, False), eng.acquire(B, T, H, W, False, False)
        sb, _ = ds.slab_batch(idx)
        eng.pack_input(ws_a, sb)
        eng.pack_input(ws_b, X)
        torch.cuda.synchronize()
        assert torch.equal(ws_a.xs, ws_b.xs)
        # fill_slab of a segment: steps [1, 3) of every window
        ws_c = eng.acquire(B, 2, H, W, False, False)
        eng.pack_input(ws_c, sb.segment(1, 2))
        ws_d = eng.acquire(B, 2, H, W, False, False)
        eng.pack_input(ws_d, X[:, 1:3].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(ws_c.xs, ws_d.xs)


# ------------------------------------------------------------------ 6. refusals on the device path
def test_refusals_on_the_device(pkg):
    from nasa_niswan_amd._lib import NintError
    c = CLM.CASES["thin"]
    net, eng = make_net(pkg, "thin", "f32", False)
    X = data_of(c)["X"].cuda()
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    # backward after a fed forward: refused by the library before any launch; after an open-loop forward it runs
    ws = eng.acquire(B, T, H, W, True, False)
    net._pack_weights(eng)
    eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 1))
    eng.head_backward(ws, net.conv.weight, torch.ones(B, c["O"], H, W, device="cuda"))
    with pytest.raises(NintError, match="invalid argument"):
        eng.backward(ws, False, zero_state_grads=(0, 1))
    eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, T))          # nothing fed back
    eng.head_backward(ws, net.conv.weight, torch.ones(B, c["O"], H, W, device="cuda"))
    eng.backward(ws, False, zero_state_grads=(0, 1))
    eng.forward(ws, X)
    eng.head_backward(ws, net.conv.weight, torch.ones(B, c["O"], H, W, device="cuda"))
    eng.backward(ws, False, zero_state_grads=(0, 1))
    # step 0 without a state
    with pytest.raises(ValueError, match="needs a state"):
        eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 0))
    eng.release(ws)
    with pytest.raises(ValueError, match="pass a state"):
        net(X, free_from=0)
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(X, free_from=1)
    with pytest.raises(RuntimeError, match="back-propagation"):
        with torch.enable_grad():
            net(X.clone().requires_grad_(True), free_from=T - 1)
    torch.cuda.synchronize()
    # a head the feedback kernel does not hold: refused before anything is enqueued (the workspace's slabs stay as they were)
    big = pkg.ConvLSTM(8, [16, 160], [3, 3], 2, out_channels=2, feedback=True).cuda()
    with torch.no_grad():
        with pytest.raises(NintError, match="beyond the staged head"):
            big(torch.randn(1, 3, 8, 8, 8, device="cuda"), free_from=1)


# ------------------------------------------------------------------ 7. train.py
def test_train_py_tracer_input_and_rollout_end_to_end(pkg, tmp_path, monkeypatch, capsys):
    from nasa_niswan_amd import train as T
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    snap = tmp_path / "s"
    argv = ["--model", "LSTM-cl", "--in-channels", "5", "--hidden-channels", "8", "4", "--kernel-size", "3", "3", "--num-layers", "2",
            "--sequence-length", "4", "--input-size", "12", "16", "--grid", "12", "16", "--batch-size", "2", "--num-epochs", "1",
            "--learning-rate", "1e-4", "--synthetic-steps", "60", "--dtype", "f32", "--snapshot-dir", str(snap),
            "--cyclic-longitude", "--tracer-input", "--test-rollout", "5", "--rollout-spinup", "3"]
    logger = T.main(T.get_arguments(argv))
    out = capsys.readouterr().out
    assert "R2 per lead time" in out and len(logger["rollout_r2"]) == 5 and np.isfinite(logger["rollout_r2"]).all()
    assert np.isfinite(logger["MSELoss"]).all() and np.load(snap / "rollout_r2.npy").shape == (5,)
