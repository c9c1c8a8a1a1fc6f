"""GPU: cyclic longitude in the ConvLSTM (``ConvLSTM(lon_cyclic=True)``, nint_seq.lon_cyclic) -- the halo
columns of the slabs the conv, dgrad and weight-gradient kernels read hold the wrapped interior columns.

Reference: tests/cyclic_model.py (the reference's cell and stack with a circular pad in x), in f64 under torch autograd.
Tolerances: the standing ones of tests/test_gpu_parity.py --
  f32 outputs rtol 1e-4 / atol 1e-5; f32 gradients max-abs error <= 1e-3 * max|grad| + 1e-6; bf16 rel-L2 <= 2e-2.
Shapes: cyclic_model.CASES, the smallest at which the wrap can go wrong (B = 2, T = 3; E: the production width, B = 1, T = 2)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import cyclic_model as CM
from test_gpu_parity import assert_bf16, assert_close_grad, assert_close_out

pytestmark = pytest.mark.gpu
OUT = 2


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


@contextlib.contextmanager
def knobs(**kw):
    """the schedule hooks of nasa_niswan_amd.engine (FORCE_WAVE, FUSE_BWD, FORCE_TILE_ROWS), as tests/test_gpu_fused_bwd.py sets them"""
    from nasa_niswan_amd import engine
    old = {k: getattr(engine, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(engine, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(engine, k, v)


def params_of(c, seed=3, dtype=torch.float32):
    from oracle import convlstm_oracle as O
    return O.synth_params(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=OUT, seed=seed, dtype=dtype)


def data_of(c, seed=11, T=None):
    """X, the cotangents of pred and seq, and a tensor state (h0, c0) with its own scale"""
    rng = np.random.default_rng(seed)
    B, T, H, W = c["B"], c["T"] if T is None else T, c["H"], c["W"]
    f = lambda *s, scale=1.0: torch.from_numpy((scale * rng.standard_normal(s)).astype(np.float32))
    return dict(X=f(B, T, c["C"], H, W), R=f(B, OUT, H, W), RS=f(B, T * OUT, H, W),
                h0=[f(B, ch, H, W, scale=0.5) for ch in c["hidden"]], c0=[f(B, ch, H, W, scale=0.5) for ch in c["hidden"]])


def make_net(pkg, c, dtype, cyclic=True, seed=3, **kw):
    net = pkg.ConvLSTM(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=OUT, compute_dtype=dtype, lon_cyclic=cyclic,
                       **kw).cuda()
    net.load_state_dict(params_of(c, seed))
    return net


_REF = {}


def reference(case, with_state):
    """pred, seq and every gradient of loss = sum(pred * R) + sum(seq * RS) from the CPU model, f64, computed once"""
    key = (case, with_state)
    if key not in _REF:
        c = CM.CASES[case]
        d = data_of(c)
        p = {k: v.double().requires_grad_(True) for k, v in params_of(c).items()}
        X = d["X"].double().requires_grad_(True)
        h0 = [t.double().requires_grad_(True) for t in d["h0"]] if with_state else None
        c0 = [t.double().requires_grad_(True) for t in d["c0"]] if with_state else None
        pred, seq = CM.forward(X, p, cyclic=True, return_sequence=True, h0=h0, c0=c0)
        ((pred * d["R"].double()).sum() + (seq * d["RS"].double()).sum()).backward()
        res = {"pred": pred.detach(), "seq": seq.detach(), "dX": X.grad}
        res.update({"grad." + k: v.grad for k, v in p.items()})
        if with_state:
            for l in range(len(h0)):
                res[f"dh0.{l}"], res[f"dc0.{l}"] = h0[l].grad, c0[l].grad
        _REF[key] = {k: v.float() for k, v in res.items()}
    return _REF[key]


def run_gpu(pkg, case, dtype, with_state=False, cyclic=True, data=None):
    c = CM.CASES[case]
    d = data if data is not None else data_of(c)
    net = make_net(pkg, c, dtype, cyclic, return_sequence=True)
    X = d["X"].cuda().requires_grad_(True)
    st = None
    if with_state:
        st = [(h.cuda().requires_grad_(True), cc.cuda().requires_grad_(True)) for h, cc in zip(d["h0"], d["c0"])]
    pred, seq = net(X, st) if with_state else net(X)
    ((pred * d["R"].cuda()).sum() + (seq * d["RS"].cuda()).sum()).backward()
    torch.cuda.synchronize()
    res = {"pred": pred.detach(), "seq": seq.detach(), "dX": X.grad}
    res.update({"grad." + k: p.grad for k, p in net.named_parameters()})
    if with_state:
        for l, (h, cc) in enumerate(st):
            res[f"dh0.{l}"], res[f"dc0.{l}"] = h.grad, cc.grad
    return {k: v.detach().clone() for k, v in res.items()}, net


def compare(got, want, dtype, tag=""):
    assert set(got) == set(want)
    for k in sorted(want):
        assert torch.isfinite(got[k]).all(), (tag, k)
        if dtype == "bf16":
            assert_bf16(got[k], want[k], f"{tag}{k}", 2e-2)
        elif k in ("pred", "seq"):
            assert_close_out(got[k], want[k], f"{tag}{k}")
        else:
            assert_close_grad(got[k], want[k], f"{tag}{k}")


# ------------------------------------------------------------------ 1. against the CPU reference
@pytest.mark.parametrize("with_state", [False, True], ids=["zero-state", "tensor-state"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(CM.CASES))
def test_against_the_cpu_reference(pkg, case, dtype, with_state):
    """pred, the per-step seq, every dW and db, the head's gradients, dx and (tensor states) dh0, dc0"""
    got, net = run_gpu(pkg, case, dtype, with_state)
    (eng,) = net._engines.values()
    assert eng.lon_cyclic and bool(eng.cfgs[0].xfold) == CM.FOLDED[case]
    assert all(ws.seq.lon_cyclic == 1 for pool in eng.pool.values() for ws in pool)
    compare(got, reference(case, with_state), dtype)


def test_the_zero_padded_net_is_not_the_cyclic_one(pkg):
    """the tests above can tell the two apart: at the stated tolerance the zero-padded net misses the cyclic reference"""
    got, _ = run_gpu(pkg, "A", "f32", cyclic=False)
    with pytest.raises(AssertionError):
        compare(got, reference("A", False), "f32")


# ------------------------------------------------------------------ 2. every schedule
_SCHED = {}


def schedule_run(pkg, wave, fuse, rows, dtype, cyclic=True):
    key = (wave, fuse, rows, dtype, cyclic)
    if key not in _SCHED:
        with knobs(FORCE_WAVE=wave, FUSE_BWD=fuse, FORCE_TILE_ROWS=rows):
            got, net = run_gpu(pkg, "B", dtype, cyclic=cyclic)
            (eng,) = net._engines.values()
            assert {ws.seq.wave for pool in eng.pool.values() for ws in pool} == {wave}
            assert {ws.seq.fuse_bwd for pool in eng.pool.values() for ws in pool} == {fuse}
        _SCHED[key] = got
    return _SCHED[key]


@pytest.mark.parametrize("fuse", [0, 1, 2])
@pytest.mark.parametrize("wave", range(6))
def test_every_schedule_against_the_reference(pkg, wave, fuse):
    """case B (three layers: the forward wavefront and the BPTT merges are live) under nint_seq.wave 0 .. 5 and
    nint_seq.fuse_bwd 0, 1, 2: a wrap right behind its writer serves every order of the launches"""
    for dtype in ("f32", "bf16"):
        compare(schedule_run(pkg, wave, fuse, 0, dtype), reference("B", False), dtype, f"wave {wave} fuse {fuse} {dtype} ")


@pytest.mark.parametrize("fuse", [0, 1, 2])
def test_schedules_that_agree_bit_for_bit_still_do(pkg, fuse):
    """f32, include/nint.h: wave = 1 is the time-major order (wave = 0) bit for bit, and the forward pass of wave = 2 is the
    time-major order with tile_rows pinned to 8 (the pin also moves the dgrad launches to 8-row tiles, which wave = 2 does
    not: the gradients of that pair differ in their rounding today).  Whatever agrees bit for bit in the zero-padded net
    agrees bit for bit with the wraps in between."""
    runs = {cyclic: dict(base=schedule_run(pkg, 0, fuse, 0, "f32", cyclic), pinned=schedule_run(pkg, 0, fuse, 8, "f32", cyclic),
                         w1=schedule_run(pkg, 1, fuse, 0, "f32", cyclic), w2=schedule_run(pkg, 2, fuse, 0, "f32", cyclic))
            for cyclic in (False, True)}
    for a, b in (("w1", "base"), ("w2", "pinned")):
        today = {k for k in runs[False][a] if torch.equal(runs[False][a][k], runs[False][b][k])}
        assert today >= ({"pred", "seq"} if a == "w2" else set(runs[False][a])), (a, b, sorted(today))
        for k in sorted(today):
            assert torch.equal(runs[True][a][k], runs[True][b][k]), ("cyclic", a, b, k)


# ------------------------------------------------------------------ 3. roll equivariance on the device
@pytest.mark.parametrize("case", ["A", "C"])
def test_roll_equivariance_on_the_device(pkg, case):
    """f32: net(roll(x, s)) == roll(net(x), s) along W, and the weight gradients of the rolled problem (input and cotangents
    rolled together) are those of the original -- at the f32 output tolerance.  Prints whether it is in fact bitwise."""
    c = CM.CASES[case]
    d = data_of(c)
    base, _ = run_gpu(pkg, case, "f32", data=d)
    for s in (1, c["W"] - 3):
        r = dict(d, X=torch.roll(d["X"], s, -1), R=torch.roll(d["R"], s, -1), RS=torch.roll(d["RS"], s, -1))
        got, _ = run_gpu(pkg, case, "f32", data=r)
        bitwise = {}
        for k in ("pred", "seq", "dX"):
            want = torch.roll(base[k], s, -1)
            bitwise[k] = torch.equal(got[k], want)
            assert_close_out(got[k], want, f"shift {s}: {k}")
        for k in base:
            if k.startswith("grad."):
                bitwise[k] = torch.equal(got[k], base[k])
                assert_close_out(got[k], base[k], f"shift {s}: {k}")
        print(f"  case {case} shift {s}: bitwise {bitwise}")


# ------------------------------------------------------------------ 4. against the existing zero-padded kernels
@pytest.mark.parametrize("dtype_cin", [3, 32], ids=["folded", "unfolded"])
def test_against_the_zero_padded_kernels_on_a_cyclic_padded_input(pkg, dtype_cin):
    """No CPU code: L = 2, k = [3, 3], T = 2.  The cyclic net on W columns against today's net on the input cyclic-padded by 8
    columns a side -- wider than the T * L * 1 = 4 columns the seam's zero padding can travel -- with the loss on the
    W-column crop: pred on the crop and every weight gradient agree; as functions of the weights the two are the same map."""
    c = dict(C=dtype_cin, hidden=[16, 8], ks=[3, 3], B=2, T=2, H=9, W=20)
    pad = 8
    d = data_of(c, seed=21)
    Xp = torch.cat([d["X"][..., -pad:], d["X"], d["X"][..., :pad]], dim=-1)
    cyc, plain = make_net(pkg, c, "f32", True), make_net(pkg, c, "f32", False)
    R = d["R"].cuda()
    pc = cyc(d["X"].cuda())
    (pc * R).sum().backward()
    pp = plain(Xp.cuda())[..., pad:pad + c["W"]]
    (pp * R).sum().backward()
    torch.cuda.synchronize()
    assert_close_out(pc, pp, "pred on the crop")
    gp = dict(plain.named_parameters())
    for k, p in cyc.named_parameters():
        assert_close_grad(p.grad, gp[k].grad, "grad." + k)


# ------------------------------------------------------------------ 5. carried options
def test_device_state_chained_twice_is_one_window(pkg):
    """net(x, state, return_state="device") over two windows of T steps equals one window of 2T: the carried h images keep
    their wrapped halo columns through nint_state_copy, and the whole is the CPU model's"""
    c = CM.CASES["A"]
    T = c["T"]
    d = data_of(c, T=2 * T)
    net = make_net(pkg, c, "f32")
    with torch.no_grad():
        X = d["X"].cuda()
        whole, st_whole = net(X, None, return_state="device")
        _, st = net(X[:, :T].contiguous(), None, return_state="device")
        pred, st2 = net(X[:, T:].contiguous(), st, return_state="device")
        want, hs, cs = CM.forward(d["X"].double(), params_of(c, dtype=torch.float64), return_states=True)
    assert_close_out(pred, whole, "chained vs whole")
    assert_close_out(pred, want.float(), "chained vs the CPU model")
    for l, ((h, cc), (hw, cw)) in enumerate(zip(st2.tensors(), st_whole.tensors())):
        assert_close_out(h, hw, f"h_T layer {l}")
        assert_close_out(cc, cw, f"c_T layer {l}")
        assert_close_out(h, hs[l].float(), f"h_T layer {l} vs the CPU model")
    # ... and a wrapped state never reaches a zero-padding engine
    plain = make_net(pkg, c, "f32", cyclic=False)
    with pytest.raises(ValueError, match="cyclic longitude"):
        plain(X[:, :T].contiguous(), st)


def _trainer_grads(pkg, c, X, y, dtype="f32", **kw):
    from nasa_niswan_amd.trainer import FusedTrainer
    net = make_net(pkg, c, dtype)
    tr = FusedTrainer(net, lr=1e-3, halo=(1, 0), **kw)
    loss = tr.step(X, y).clone()
    torch.cuda.synchronize()
    names = [k for k, _ in net.named_parameters()]
    return loss, {k: tr.flat.grad[o:o + p.numel()].clone().view(p.shape) for k, o, p in zip(names, tr.flat.offsets, tr.flat.params)}


def _cpu_step(c, X, y, h0=None, c0=None, frozen=0):
    """loss and gradients of the trainer's step on the CPU model: MSE + L1 on the crop of rows [1, H - 1), all columns"""
    from oracle import convlstm_oracle as O
    p = {k: v.double().requires_grad_(True) for k, v in params_of(c).items()}
    pred, hs, cs = CM.forward(X.double(), p, return_states=True, h0=h0, c0=c0)
    loss = O.loss_mse_l1(y.double(), pred[:, :, 1:-1])
    loss.backward()
    return loss.detach(), {k: v.grad.float() for k, v in p.items()}, [t.detach() for t in hs], [t.detach() for t in cs]


def _window(c, T, seed=31):
    d = data_of(c, seed=seed, T=T)
    y = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((c["B"], OUT, c["H"] - 2, c["W"])).astype(np.float32))
    return d["X"], y


def test_bptt_segments_give_the_unsegmented_gradients(pkg):
    c = CM.CASES["A"]
    X, y = _window(c, 4)
    l1, g1 = _trainer_grads(pkg, c, X.cuda(), y.cuda())
    l2, g2 = _trainer_grads(pkg, c, X.cuda(), y.cuda(), bptt_segments=2)
    lo, go, _, _ = _cpu_step(c, X, y)
    assert_close_out(l2, l1, "loss, segments vs whole")
    assert_close_out(l1, lo.float(), "loss vs the CPU model")
    for k in g1:
        assert_close_grad(g2[k], g1[k], "segments vs whole: " + k)
        assert_close_grad(g2[k], go[k], "segments vs the CPU model: " + k)


def test_freeze_layers_is_autograd_with_requires_grad_false(pkg):
    from oracle import convlstm_oracle as O
    c = CM.CASES["B"]
    X, y = _window(c, c["T"])
    _, g = _trainer_grads(pkg, c, X.cuda(), y.cuda(), freeze_layers=1)
    net = make_net(pkg, c, "f32")
    net.layers[0].requires_grad_(False)
    O.loss_mse_l1(y.cuda(), net(X.cuda())[:, :, 1:-1]).backward()
    _, go, _, _ = _cpu_step(c, X, y)
    live = [k for k, p in net.named_parameters() if p.requires_grad]
    assert live and all(not k.startswith("layers.0.") for k in live) and set(live) <= set(g)
    for k, p in net.named_parameters():
        if p.requires_grad:
            assert_close_grad(g[k], p.grad, "trainer vs autograd: " + k)
            assert_close_grad(g[k], go[k], "trainer vs the CPU model: " + k)
        else:
            assert p.grad is None


def test_stateful_trainer_runs_two_chunks(pkg):
    """lr = 0 keeps the weights, so the second chunk's loss is the CPU model's from the first chunk's final state"""
    from nasa_niswan_amd.trainer import FusedTrainer
    c = CM.CASES["A"]
    X, y1 = _window(c, 2 * c["T"])
    _, y2 = _window(c, c["T"], seed=41)
    X1, X2 = X[:, :c["T"]].contiguous(), X[:, c["T"]:].contiguous()
    tr = FusedTrainer(make_net(pkg, c, "f32"), lr=0.0, halo=(1, 0), stateful=True)
    la = tr.step(X1.cuda(), y1.cuda()).clone()
    lb = tr.step(X2.cuda(), y2.cuda()).clone()
    torch.cuda.synchronize()
    loa, _, hs, cs = _cpu_step(c, X1, y1)
    lob, gob, _, _ = _cpu_step(c, X2, y2, h0=hs, c0=cs)
    assert_close_out(la, loa.float(), "loss of chunk 1")
    assert_close_out(lb, lob.float(), "loss of chunk 2 (from the carried state)")
    names = [k for k, _ in tr.model.named_parameters()]
    for k, o, p in zip(names, tr.flat.offsets, tr.flat.params):
        assert_close_grad(tr.flat.grad[o:o + p.numel()].view(p.shape), gob[k], "chunk 2: " + k)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_slab_batch_of_a_cyclic_engine_is_preproc_then_pack(pkg, dtype):
    """the device data path (train.py --cyclic-longitude): a SlabBatch written straight into a cyclic engine's input slab by
    nint_preproc_fuse_pad_static_slab_cyclic holds the bytes of the materialised batch through nint_pack_btchw_xfold_cyclic,
    and the folded channels of the first and last columns hold the wrapped neighbours, not zeros.  A grid with a longitude
    halo is refused: the model wraps at its own edge."""
    from nasa_niswan_amd._lib import NintError
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    Cin, k, T, H, W, idx = 5, 5, 2, 20, 24, [3, 0]
    ds = SyntheticE33OMA_CRNN("train", padding=(H + 4, W), in_channels=Cin, sequence_length=T, levels=1, n_steps=24, grid=(H, W),
                              device="cuda")
    eng = SeqEngine([LayerCfg(Cin, 16, k)], dtype, "cuda", lon_cyclic=True)
    assert eng.cfgs[0].xfold
    B = len(idx)
    ws_a, ws_b = eng.acquire(B, T, H + 4, W, False, False), eng.acquire(B, T, H + 4, W, False, False)
    sb, _ = ds.slab_batch(idx)
    eng.pack_input(ws_a, sb)
    X, _ = ds.device_batch(idx)
    eng.pack_input(ws_b, X)
    torch.cuda.synchronize()
    assert torch.equal(ws_a.xs, ws_b.xs)
    g, P = ws_a.g, ws_a.g.P
    et = torch.float32 if dtype == "f32" else torch.bfloat16
    slab = ws_a.xs.view(et).view(T * B, g.Hh, g.Wh, ws_a.Cxp0)[:, P:P + H + 4, P:P + W].float()
    want = X.to(et).float().permute(1, 0, 3, 4, 2).reshape(T * B, H + 4, W, Cin)              # image t*B+b, channels last
    for kx in range(k):
        assert torch.equal(slab[..., kx * Cin:(kx + 1) * Cin], torch.roll(want, k // 2 - kx, 2)), kx
    wide = SyntheticE33OMA_CRNN("train", padding=(H + 4, W + 4), in_channels=Cin, sequence_length=T, levels=1, n_steps=24,
                                grid=(H, W), device="cuda")
    ws_c = eng.acquire(B, T, H + 4, W + 4, False, False)
    with pytest.raises(NintError, match="invalid argument"):
        eng.pack_input(ws_c, wide.slab_batch(idx)[0])


# ------------------------------------------------------------------ 6. no trace
def test_a_cyclic_net_leaves_no_trace_in_a_zero_padded_one(pkg):
    """A cyclic net and a zero-padded net of the same shapes run alternately in one process: the zero-padded net's outputs and
    gradients are bit for bit those of a zero-padded net that ran before the cyclic one existed (engines, workspaces and plans
    are per module; the library keeps no state), its workspaces carry lon_cyclic = 0 and its plan no wrap launch."""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    for dtype in ("f32", "bf16"):
        first, _ = run_gpu(pkg, "A", dtype, with_state=True, cyclic=False)
        for _ in range(2):
            cyc, _ = run_gpu(pkg, "A", dtype, with_state=True, cyclic=True)
            again, net = run_gpu(pkg, "A", dtype, with_state=True, cyclic=False)
            for k in first:
                assert torch.equal(again[k], first[k]), (dtype, k)
            assert not torch.equal(cyc["pred"], first["pred"])
        (eng,) = net._engines.values()
        for pool in eng.pool.values():
            for ws in pool:
                assert ws.seq.lon_cyclic == 0
                ws.seq.need_dx = 0                # (the engine took the pass's dx slab back: plan the chain without it)
                for bwd in ((0, 1) if ws.train else (0,)):
                    recs = (_lib.NintLaunchRec * 256)()
                    n = lib.nint_debug_seq_plan(C.byref(ws.seq), bwd, recs, 256)
                    assert 0 < n <= 256, (bwd, n)
                    idx = sorted({r.index for r in recs[:n]})
                    assert idx == list(range(len(idx)))            # consecutive: nothing planned in between


# ------------------------------------------------------------------ 7. guards
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_case_a_under_the_guarded_allocator(pkg, dtype):
    """tests/test_gpu_memory_contract.py's three runs (plain torch, guarded zero-filled, guarded poisoned) of a cyclic net:
    no store outside an extent, no result that depends on a byte the library did not write -- and after the backward pass
    every dG image has zero halo columns (and rows) again, while every h block written holds its own wrapped columns."""
    import test_gpu_memory_contract as MC
    c = CM.CASES["A"]
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    held = {}

    def scenario(gt):
        G = (lambda t: t) if gt is None else gt.guard_copy
        d = data_of(c)
        net = make_net(pkg, c, dtype, return_sequence=True)
        if gt is not None:
            gt.guard_module(net)
            MC._fill_unused_weight_tail(net._engine(torch.device("cuda", torch.cuda.current_device())), gt.fill)
        X = G(d["X"].cuda()).requires_grad_(True)
        st = [(G(h.cuda()).requires_grad_(True), G(cc.cuda()).requires_grad_(True)) for h, cc in zip(d["h0"], d["c0"])]
        pred, seq = net(X, st)
        ((pred * G(d["R"].cuda())).sum() + (seq * G(d["RS"].cuda())).sum()).backward()
        held["net"] = net
        res = {"pred": pred.detach(), "seq": seq.detach(), "dX": X.grad}
        res.update({"grad." + k: p.grad for k, p in net.named_parameters()})
        for l, (h, cc) in enumerate(st):
            res[f"dh0.{l}"], res[f"dc0.{l}"] = h.grad, cc.grad
        return res

    def self_check(gt):
        (eng,) = held["net"]._engines.values()
        et = torch.bfloat16 if eng.es == 2 else torch.float32
        seen = 0
        for pool in eng.pool.values():
            for ws in pool:
                if not ws.train:
                    continue
                g, P = ws.g, ws.g.P
                for l, ly in enumerate(eng.layers):
                    dG = ws.dG[l].view(et).view(T * B, g.Hh, g.Wh, 4 * ly.Ch16).float()
                    assert float(dG[:, P:P + H, P:P + W].abs().max()) > 0
                    assert float(dG[:, :, :P].abs().max()) == 0 and float(dG[:, :, P + W:].abs().max()) == 0, ("dG columns", l)
                    assert float(dG[:, :P].abs().max()) == 0 and float(dG[:, P + H:].abs().max()) == 0, ("dG rows", l)
                    h = ws.h[l].view(et).view((T + 1) * B, g.Hh, g.Wh, ly.Chp)
                    rows = h[:, P:P + H]
                    assert torch.equal(rows[:, :, :P], rows[:, :, W:W + P]) and torch.equal(rows[:, :, P + W:P + W + P], rows[:, :, P:2 * P])
                    assert float(h[:, :P].float().abs().max()) == 0 and float(h[:, P + H:].float().abs().max()) == 0, ("h rows", l)
                    assert float(h[:, :, P + W + P:].float().abs().max()) == 0, ("h columns behind the halo", l)
                    seen += 1
        assert seen == len(eng.layers)

    stack = (c["C"], c["hidden"], c["ks"])
    assert MC.three_runs(f"cyclic-A-{dtype}", scenario, MC.row_stride(stack, (H, W)), self_check) > 0


# ------------------------------------------------------------------ train.py
def test_train_py_cyclic_longitude_end_to_end(pkg, tmp_path, monkeypatch, capsys):
    """train.py --cyclic-longitude on the command line of the existing end-to-end tests: a latitude halo of 2, no longitude
    halo, two epochs through the device data path; the trainer's model runs the cyclic engine and the losses are finite"""
    import json
    from nasa_niswan_amd import train as T
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    snap = tmp_path / "s"
    argv = ["--model", "LSTM-cfg0", "--in-channels", "4", "--hidden-channels", "8", "--kernel-size", "3", "--num-layers", "1",
            "--sequence-length", "4", "--input-size", "32", "32", "--grid", "28", "32", "--batch-size", "2", "--num-epochs", "2",
            "--learning-rate", "1e-4", "--synthetic-steps", "24", "--dtype", "f32", "--snapshot-dir", str(snap), "--cyclic-longitude"]
    from nasa_niswan_amd import engine
    seen, init = [], engine.SeqEngine.__init__

    def spy(self, *a, **k):
        seen.append(k.get("lon_cyclic"))
        init(self, *a, **k)
    monkeypatch.setattr(engine.SeqEngine, "__init__", spy)
    logger = T.main(T.get_arguments(argv))
    epoch = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch: ")]
    assert len(epoch) == 2, epoch
    assert seen and all(v is True for v in seen), seen          # every engine the run built is a cyclic one
    assert len(logger["MSELoss"]) == 2 and np.isfinite(logger["MSELoss"]).all()
    assert json.load(open(snap / "configurations.json"))["cyclic_longitude"] is True
