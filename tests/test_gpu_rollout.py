"""GPU: roll-out training -- ``ConvLSTM(feedback=True)(x, free_from=s, feedback_grad=True)``,
nint_seq_bwd_rollout, nint_head_feedback_bwd: BPTT through the prediction that the closed-loop forward fed back.

Shapes: closed_loop_model.CASES -- B = 2, T = 4 on a ragged 13 x 37 grid, f32 and bf16, zero padding and cyclic longitude:
a folded input with O = 1, a plain input with c0 = 37 across a 16-byte group, one layer (the top layer is the bottom layer),
O == C.  The weights are rollout_model.case_params: the oracle's synthetic ones with layer 0's feedback columns scaled so
that the fed term is far above the gates (tests/test_rollout_cpu.py asserts the separation on the CPU model).
References: numpy on small integers (exact), the library's own entries (bit for bit), the open-loop backward pass of the
library on the substituted input (bit for bit), tests/rollout_model.py in f64 under CPU autograd at the standing gates of
tests/test_gpu_parity.py -- f32: outputs rtol 1e-4 / atol 1e-5, gradients <= 1e-3 * max|grad| + 1e-6; bf16: rel-L2 <= 2e-2
against the f32 model."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_model as CLM
import rollout_model as RM
import test_gpu_memory_contract as MC
from test_gpu_closed_loop import make_net, pkg, substituted      # noqa: F401  (pkg: the fixture)
from test_gpu_parity import assert_bf16, assert_close_grad, assert_close_out

pytestmark = pytest.mark.gpu
BOTH = ("f32", "bf16")
CYC = dict(argvalues=[False, True], ids=["zero-pad", "cyclic"])


def rollout_net(pkg, case, dtype, cyclic, gt=None, zero_feed=False, **kw):
    c = CLM.CASES[case]
    net, eng = make_net(pkg, case, dtype, cyclic, gt=gt, **kw)
    p = RM.case_params(c)
    if zero_feed:
        p["layers.0.conv.weight"][:, c["C"] - c["O"]:c["C"]] = 0
    net.load_state_dict(p)
    return net, eng


# ------------------------------------------------------------------ 1. nint_head_feedback_bwd alone
def _fbb_alone(lib, ex, dt, Cx, O_, Ch, k, cyc, ints, H=13, W=37, N=2, seed=7):
    """the entry on images [1, 1 + N) of buffers that hold one more image in front; returns what it may have touched, the
    composition of the existing entries on the same data, and (ints) the numpy result"""
    from nasa_niswan_amd._lib import stream_ptr
    es, et = (2, torch.bfloat16) if dt == 1 else (4, torch.float32)
    kc = lib.nint_kc(dt)
    rup = lambda a, b: (a + b - 1) // b * b
    g = MC._geom(lib, H, W, 2)
    Chp, Cxp, c0 = rup(Ch, kc), rup((k or 1) * Cx, kc), Cx - O_
    gen = torch.Generator().manual_seed(seed)
    rnd = (lambda *s, hi=3: torch.randint(-hi, hi + 1, s, generator=gen).float()) if ints else (lambda *s, hi=3: torch.randn(*s, generator=gen))
    dx = ex.copy(rnd((1 + N) * H * W * Cxp).to(et))              # every channel of every pixel holds data: only the fed ones may count
    dp0 = rnd((1 + N), O_, H, W)
    dp = ex.copy(dp0.reshape(-1).clone())
    w = ex.copy(rnd(O_, Ch, hi=1))                               # (ints: |dh| <= 32 * (3 + 3 * k) stays exact in bf16)
    dh = ex.empty((1 + N) * H * W * Chp, et, slack=0)
    st = stream_ptr()
    assert lib.nint_head_feedback_bwd(MC.P(dx), 1, MC.P(dp), 1, MC.P(dh), 1, N, Ch, Chp, O_, MC.P(w), Cx, Cxp, c0, k, cyc, C.byref(g), dt,
                                      st) == 0
    torch.cuda.synchronize()
    res = dict(dpred=dp[:(1 + N) * O_ * H * W].clone(), dh=dh[H * W * Chp:(1 + N) * H * W * Chp].clone())
    # the composition: unpack / unfold the step's dx, add the fed channels to dpred in f32, nint_head_bwd's dh pass
    full = torch.empty(N, Cx, H, W, device="cuda")
    src = C.c_void_p(dx.data_ptr() + H * W * Cxp * es)
    if k:
        fn = lib.nint_unfold_dx_cyclic if cyc else lib.nint_unfold_dx
        assert fn(src, MC.P(full), N, Cx, k, Cxp, H, W, dt, st) == 0
    else:
        assert lib.nint_unpack_compact(src, MC.P(full), N, Cx, Cxp, H, W, dt, st) == 0
    gsum = (dp0[1:].cuda() + full[:, c0:]).contiguous()
    dh2 = torch.empty(N * H * W * Chp, dtype=et, device="cuda")
    assert lib.nint_head_bwd(MC.P(dh2), 0, N, Ch, Chp, O_, MC.P(w), MC.P(gsum), MC.P(dh2), None, None, C.byref(g), dt, None, 0, st) == 0
    torch.cuda.synchronize()
    want = dict(dpred=torch.cat([dp0[:1].cuda().reshape(-1), gsum.reshape(-1)]), dh=dh2)
    exact = None
    if ints:
        d = dx[:(1 + N) * H * W * Cxp].float().cpu().numpy().reshape(1 + N, H, W, Cxp)[1:]
        xi = np.zeros((N, O_, H, W), np.float32)
        for o in range(O_):
            if not k:
                xi[:, o] = d[..., c0 + o]
            for kx in range(k):
                for x in range(W):
                    xs = x - kx + k // 2
                    xs = xs % W if cyc else xs
                    if 0 <= xs < W:
                        xi[:, o, :, x] += d[:, :, xs, kx * Cx + c0 + o]
        gn = dp0[1:].numpy() + xi
        dhn = np.zeros((N, H, W, Chp), np.float32)
        dhn[..., :Ch] = np.einsum("nohw,oc->nhwc", gn, w[:O_ * Ch].cpu().numpy().reshape(O_, Ch))
        exact = dict(dpred=np.concatenate([dp0[:1].numpy().reshape(-1), gn.reshape(-1)]), dh=dhn.reshape(-1))
    return res, want, exact


FBB_ALONE = [("thin-folded", 4, 1, 8, 5), ("plain-straddle", 40, 3, 8, 0), ("all-folded", 3, 3, 8, 5), ("single-folded", 4, 1, 16, 5),
             ("all-plain", 32, 32, 40, 0), ("chv-128", 5, 1, 72, 3)]


@pytest.mark.parametrize("cyc", [0, 1], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dt", [0, 1], ids=BOTH)
@pytest.mark.parametrize("name,Cx,O_,Ch,k", FBB_ALONE, ids=[f[0] for f in FBB_ALONE])
def test_head_feedback_bwd_alone(pkg, name, Cx, O_, Ch, k, dt, cyc):
    """on small integers (exact in both storage types) dpred and dh equal numpy exactly; on random data they equal
    nint_unpack_compact / nint_unfold_dx[_cyclic] -> f32 add -> nint_head_bwd(dh only) bit for bit; the dpred image in front
    of the step's stays; and all of it again on buffers of exactly their sizes under the poisoning allocator"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    for ints in (True, False):
        def call(ex):
            res, want, exact = _fbb_alone(lib, ex, dt, Cx, O_, Ch, k, cyc, ints)
            for key in res:
                assert torch.equal(res[key], want[key]), (name, ints, key)
                if exact is not None:
                    assert np.array_equal(res[key].float().cpu().numpy(), exact[key]), (name, key, "numpy")
            return res
        MC.both_ways(f"head_feedback_bwd {name} ints={ints}", call)


# ------------------------------------------------------------------ 2. bit identities
def _cot(c):
    d = RM.case_data(c)
    return d["X"].cuda(), d["dseq"].cuda(), d["dpred"].cuda()


def _rollout_engine(net, eng, X, F_, dseq, dpred, need_dx):
    """forward with feedback_grad, the roll-out backward and the head reduction, driven through the engine"""
    B, T, _, H, W = X.shape
    L = len(eng.cfgs)
    w, b = net.conv.weight, net.conv.bias
    ws = eng.acquire(B, T, H, W, True, False)
    try:
        net._pack_weights(eng)
        eng.forward(ws, X, feedback=(w, b, F_), feedback_grad=True)
        seq = eng.head_forward_seq(ws, w, b)
        slab = eng.rollout_cotangents(ws, w, dseq, dpred)
        dWs, dbs, dx = eng.backward(ws, need_dx, zero_state_grads=tuple(range(L)), rollout=slab)
        dw, db = eng.head_backward(ws, w, slab, write_dh=False, images=(B, T * B))
        torch.cuda.synchronize()
        return dict(seq=seq, dW=dWs, db=dbs, dx=dx, dw=dw.clone(), dbh=db.clone(), g=slab.clone())
    finally:
        eng.release(ws)


def _open_engine(net, eng, X, dseq, dpred):
    """the open-loop pass on X and its backward pass planned time-major all-classic (fuse_bwd = 1, wave = 0) with seq_grads"""
    B, T, _, H, W = X.shape
    L = len(eng.cfgs)
    w, b = net.conv.weight, net.conv.bias
    ws = eng.acquire(B, T, H, W, True, False)
    keep = (ws.seq.fuse_bwd, ws.seq.wave)
    try:
        net._pack_weights(eng)
        eng.forward(ws, X)
        seq = eng.head_forward_seq(ws, w, b)
        ws.seq.fuse_bwd, ws.seq.wave = 1, 0
        dw, db = eng.head_backward_seq(ws, w, dseq, dpred)
        dWs, dbs, dx = eng.backward(ws, True, zero_state_grads=tuple(range(L)), seq_grads=True)
        torch.cuda.synchronize()
        return dict(seq=seq, dW=dWs, db=dbs, dx=dx, dw=dw.clone(), dbh=db.clone())
    finally:
        ws.seq.fuse_bwd, ws.seq.wave = keep
        eng.release(ws)


@pytest.mark.parametrize("cyclic", **CYC)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(CLM.CASES))
def test_with_zero_feedback_columns_it_is_the_open_loop_backward_bit_for_bit(pkg, case, dtype, cyclic):
    """layer 0 does not see its feedback channels: xi = 0, the added zeros change nothing, and every gradient -- dW, db of every
    layer, the head's dw / db, dx off the fed channels -- equals the classic time-major open-loop backward on x_fed bit for bit"""
    c = CLM.CASES[case]
    net, eng = rollout_net(pkg, case, dtype, cyclic, zero_feed=True)
    X, dseq, dpred = _cot(c)
    c0 = c["C"] - c["O"]
    for F_ in (1, c["T"] - 1):
        for need_dx in (True, False):
            a = _rollout_engine(net, eng, X, F_, dseq, dpred, need_dx)
            o = _open_engine(net, eng, substituted(c, X, a["seq"], F_), dseq, dpred)
            assert torch.equal(a["seq"], o["seq"])
            for l in range(len(c["hidden"])):
                assert torch.equal(a["dW"][l], o["dW"][l]) and torch.equal(a["db"][l], o["db"][l]), (case, F_, need_dx, l)
            assert torch.equal(a["dw"], o["dw"]) and torch.equal(a["dbh"], o["dbh"]), (case, F_, need_dx, "head")
            if need_dx:
                assert torch.equal(a["dx"][:, :F_], o["dx"][:, :F_]) and torch.equal(a["dx"][:, :, :c0], o["dx"][:, :, :c0])
                assert not bool(a["dx"][:, F_:, c0:].any())
            else:
                assert a["dx"] is None


@pytest.mark.parametrize("cyclic", **CYC)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", ["thin", "wide"])
def test_the_one_step_scratch_and_the_module_give_the_same_bits(pkg, case, dtype, cyclic):
    """with live feedback columns: need_dx = 0 (x columns of the fed steps through the one-step scratch) equals need_dx = 1; the
    module's autograd route equals the engine's; feedback_grad=True with free_from >= T equals the call without the flag"""
    c = CLM.CASES[case]
    net, eng = rollout_net(pkg, case, dtype, cyclic, return_sequence=True)
    X, dseq, dpred = _cot(c)
    T = c["T"]
    a = _rollout_engine(net, eng, X, 1, dseq, dpred, True)
    b = _rollout_engine(net, eng, X, 1, dseq, dpred, False)
    for k in ("dw", "dbh", "g"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(u, v) for u, v in zip(a["dW"] + a["db"], b["dW"] + b["db"]))
    assert bool((a["g"][:(T - 1) * c["B"]] != _slab(c, dseq, dpred)[:(T - 1) * c["B"]]).any())         # something came back

    def module(F_, **kw):
        net.zero_grad()
        Xg = X.clone().requires_grad_(True)
        pred, seq = net(Xg, free_from=F_, **kw)
        torch.autograd.backward([pred, seq], [dpred, dseq])
        return [pred.detach(), seq.detach(), Xg.grad] + [p.grad.clone() for p in net.parameters()]
    m = module(1, feedback_grad=True)
    assert torch.equal(m[1], a["seq"]) and torch.equal(m[2], a["dx"])
    names = [n for n, _ in net.named_parameters()]
    got = dict(zip(names, m[3:]))
    for l in range(len(c["hidden"])):
        assert torch.equal(got[f"layers.{l}.conv.weight"], a["dW"][l]) and torch.equal(got[f"layers.{l}.conv.bias"], a["db"][l])
    assert torch.equal(got["conv.weight"], a["dw"]) and torch.equal(got["conv.bias"], a["dbh"])
    for F_ in (T, T + 2):
        assert all(torch.equal(u, v) for u, v in zip(module(F_, feedback_grad=True), module(F_)))
    assert all(torch.equal(u, v) for u, v in zip(module(T, feedback_grad=True), module(None)))


def _slab(c, dseq, dpred):
    B, T, O_, H, W = c["B"], c["T"], c["O"], c["H"], c["W"]
    s = dseq.view(B, T, O_, H, W).transpose(0, 1).contiguous()
    s[T - 1] += dpred
    return s.view(T * B, O_, H, W)


# ------------------------------------------------------------------ 3. against CPU autograd
def _grads_on_device(net, d, X, F_, with_state, **kw):
    """one call of the module under autograd with the case's cotangents: (seq, pred, {tensor name: gradient})"""
    net.zero_grad()
    Xg = X.clone().requires_grad_(True)
    cots = [d["dpred"].cuda(), d["dseq"].cuda()]
    if with_state:
        st = [(h.cuda().requires_grad_(True), cc.cuda().requires_grad_(True)) for h, cc in zip(d["h0"], d["c0"])]
        pred, seq, out = net(Xg, st, free_from=F_, return_state=True, **kw)
        outs = [pred, seq] + [t for pair in out for t in pair]
        cots = cots + [t.cuda() for pair in zip(d["dhT"], d["dcT"]) for t in pair]
    else:
        st = []
        pred, seq = net(Xg, free_from=F_, **kw)
        outs = [pred, seq]
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    g = {"d " + n: p.grad.clone() for n, p in net.named_parameters()}
    g["dx"] = Xg.grad.clone()
    for l, (h, cc) in enumerate(st):
        g[f"dh0[{l}]"], g[f"dc0[{l}]"] = h.grad.clone(), cc.grad.clone()
    return seq.detach(), pred.detach(), g


def _ref_grad(r, k):
    if k.startswith("d "):
        return r["params"][k[2:]]
    return r["dx"] if k == "dx" else (r["dh0"] if k.startswith("dh0") else r["dc0"])[int(k[4:-1])]


_rel = lambda a, b: float((a.double().cpu() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize("cyclic", **CYC)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(CLM.CASES))
def test_autograd_parity_with_the_cpu_model(pkg, case, dtype, cyclic):
    """net(x, [state,] free_from=F, feedback_grad=True) with cotangents on pred and seq (and, with a tensor state, on the
    returned state): outputs, every parameter gradient, dx (exact zeros on the fed channels of the fed steps) and the state
    gradients at the standing gates; and wherever the CPU model puts the teacher-forced gradient on x_fed more than two gates
    away, the device's gradient is more than one gate away from it -- the fed term is there.

    bf16: the standing gate is rel-L2 <= 2e-2 against the f32 model.  With the cases' scaled feedback columns some gradients of
    the EXISTING teacher-forced path miss it already: that path's rel-L2 on x_fed (same stack, same window, same cotangents;
    dx compared off the fed channels) is the storage-rounding floor, none of it code under test, and it is measured here, in
    the same test.  Where a roll-out gradient misses 2e-2 it may be at most twice its floor (one more rounded tensor per
    step enters).  Measured, worst over boundary, F and state: case `all` dx roll-out 3.81e-2 / floor 3.78e-2, dh0[0]
    3.44e-2 / 3.44e-2; every other tensor of every case stays under 2e-2, worst 1.98e-2.  The cotangents carry a mean (rollout_model.case_data): the head's
    bias gradient is their plain sum plus the fed term's, and zero-mean cotangents make that sum a difference of large
    numbers whose relative error measures the draw, not the code."""
    c = CLM.CASES[case]
    T, c0 = c["T"], c["C"] - c["O"]
    net, eng = rollout_net(pkg, case, dtype, cyclic, return_sequence=True)
    d = RM.case_data(c)
    X = d["X"].cuda()
    bad = []

    def held(fn, *a):
        try:
            fn(*a)
        except AssertionError as e:
            bad.append(str(e).splitlines()[0])

    cmp_out = (lambda a, b, what: assert_bf16(a, b, what, RM.BF16_GATE)) if dtype == "bf16" else assert_close_out
    for with_state in (False, True):
        for F_ in (1, 2, T - 1):
            ro, tf = RM.reference(case, cyclic, F_, with_state)
            tag = f"{case} {dtype} F={F_} state={int(with_state)}"
            seq, pred, g = _grads_on_device(net, d, X, F_, with_state, feedback_grad=True)
            held(cmp_out, seq, ro["seq"].float(), f"{tag} seq")
            held(cmp_out, pred, ro["pred"].float(), f"{tag} pred")
            assert not bool(g["dx"][:, F_:, c0:].any()), tag
            limit = {k: RM.BF16_GATE for k in g}
            if dtype == "bf16":
                # the floor: the existing teacher-forced path on x_fed against the f32 model on the same x_fed
                xf = substituted(c, X, seq, F_)
                _, _, g_tf = _grads_on_device(net, d, xf, None, with_state)
                kw = dict(dpred=d["dpred"], dseq=d["dseq"])
                if with_state:
                    kw.update(h0=[t.double() for t in d["h0"]], c0=[t.double() for t in d["c0"]], dhT=d["dhT"], dcT=d["dcT"])
                tf_dev = RM.grads(xf.cpu().double(), RM.case_params(c, torch.float64), None, cyclic, "f32", **kw)
                for k in g:
                    a, b = g_tf[k].clone(), _ref_grad(tf_dev, k).clone()
                    if k == "dx":       # (teacher forcing has a gradient on the fed channels of x_fed, the roll-out has none)
                        a[:, F_:, c0:] = 0
                        b[:, F_:, c0:] = 0
                    floor, r = _rel(a, b), _rel(g[k], _ref_grad(ro, k))
                    limit[k] = max(RM.BF16_GATE, 2 * floor)
                    print(f"  {tag} {k}: rel-L2 {r:.3e}  floor (teacher-forced) {floor:.3e}")
                    if r > limit[k]:
                        bad.append(f"{tag} {k}: rel-L2 {r:.3e} > {limit[k]:.3e} (floor {floor:.3e})")
            else:
                for k in g:
                    held(assert_close_grad, g[k], _ref_grad(ro, k).float(), f"{tag} {k}")
            # the fed term is there: away from the teacher-forced gradient wherever the CPU model separates the two
            sep = RM.separation(ro, tf)
            for n in ro["params"]:
                k, t = "d " + n, tf["params"][n]
                if dtype == "bf16":
                    far, dist = sep[n][1] * RM.BF16_GATE / limit[k], _rel(g[k], t) / limit[k]
                else:
                    far, dist = sep[n][0], float((g[k].cpu().double() - t).abs().max()) / RM.F32_GATE(t)
                if far > 2:
                    print(f"  {tag} {k}: {dist:.1f} gates from the teacher-forced gradient (CPU model: {far:.1f})")
                    if dist <= 1:
                        bad.append(f"{tag} {k}: within a gate of the teacher-forced gradient")
    assert not bad, "\n".join(bad)


def test_refusals_on_the_device(pkg):
    from nasa_niswan_amd._lib import NintError
    c = CLM.CASES["thin"]
    net, eng = rollout_net(pkg, "thin", "f32", False)
    X, dseq, dpred = _cot(c)
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    ws = eng.acquire(B, T, H, W, True, False)
    net._pack_weights(eng)
    # an unmarked fed window keeps today's refusal, and rollout= needs the mark
    eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 1))
    eng.head_backward(ws, net.conv.weight, dpred)
    with pytest.raises(NintError, match="invalid argument"):
        eng.backward(ws, False, zero_state_grads=(0, 1))
    with pytest.raises(ValueError, match="feedback_grad=True"):
        eng.backward(ws, False, zero_state_grads=(0, 1), rollout=torch.zeros(T * B, 1, H, W, device="cuda"))
    # a marked one needs its cotangents
    eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 1), feedback_grad=True)
    with pytest.raises(ValueError, match="rollout_cotangents"):
        eng.backward(ws, False, zero_state_grads=(0, 1))
    eng.release(ws)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(X, free_from=1)
    h = [(torch.zeros(B, ch, H, W, device="cuda", requires_grad=True), torch.zeros(B, ch, H, W, device="cuda")) for ch in c["hidden"]]
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(X, h, free_from=0, feedback_grad=True)


# ------------------------------------------------------------------ 4. the trainer
LR, BETAS, HALO = 1e-4, (0.5, 0.999), (2, 3)
TRAIN_VARIANTS = {"sequence": dict(sequence_loss=True), "last-step": {}, "sequence-accumulate2": dict(sequence_loss=True, accumulate_steps=2)}


def _train_batches(c, n, sq):
    rng = np.random.default_rng(91)
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    Hc, Wc = H - 2 * HALO[0], W - 2 * HALO[1]
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return [(f(B, T, c["C"], H, W), f(*((B, T, c["O"], Hc, Wc) if sq else (B, c["O"], Hc, Wc)))) for _ in range(n)]


def _cpu_fit(c, batches, cyclic, sq, k, F_=1):
    """the same steps under CPU autograd in f64 with torch.optim.Adam: per optimizer step the mean loss of its k micro-batches'
    last one (what step() returns), the mean gradient, the parameters after it"""
    p = {n: v.clone().requires_grad_(True) for n, v in RM.case_params(c, torch.float64).items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR, betas=BETAS)
    B, T, O_, H, W = c["B"], c["T"], c["O"], c["H"], c["W"]
    out = []
    for j in range(0, len(batches), k):
        opt.zero_grad()
        for X, y in batches[j:j + k]:
            r = RM.forward(X.double(), p, F_, cyclic, "f32")
            o = r["seq"].view(B, T, O_, H, W) if sq else r["pred"]
            d = y.double() - o[..., HALO[0]:H - HALO[0], HALO[1]:W - HALO[1]]
            loss = (d * d).mean() + d.abs().mean()
            (loss / k).backward()
        grads = {n: v.grad.detach().clone() for n, v in p.items()}
        opt.step()
        out.append(dict(loss=float(loss.detach()), grads=grads, params={n: v.detach().clone() for n, v in p.items()}))
    return out


@pytest.mark.parametrize("variant", sorted(TRAIN_VARIANTS))
@pytest.mark.parametrize("dtype", BOTH)
def test_two_rollout_trainer_steps_against_cpu_autograd_and_adam(pkg, dtype, variant):
    """FusedTrainer(rollout_from=1) on the folded cyclic case: the loss of every call, the bucket's gradient at the first
    optimizer step and the parameters after each, at the tolerances of tests/test_gpu_seq_train.py (loss: f32 1e-4 relative
    + 1e-5, bf16 2e-2 relative; parameters after k Adam steps at lr 1e-4: max |dp| <= k * 2.2 * lr, mean |dp| <= 2e-6 in f32,
    0.1 * lr * k in bf16; gradients: the standing gates)"""
    from nasa_niswan_amd.trainer import FusedTrainer
    c = CLM.CASES["thin"]
    kw = TRAIN_VARIANTS[variant]
    sq, k = kw.get("sequence_loss", False), kw.get("accumulate_steps", 1)
    batches = _train_batches(c, 2 * k, sq)
    want = _cpu_fit(c, batches, True, sq, k)
    net, eng = rollout_net(pkg, "thin", dtype, True)
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, rollout_from=1, **kw)
    names = [n for n, _ in net.named_parameters()]
    for step in (1, 2):
        for X, y in batches[(step - 1) * k:step * k]:
            loss = float(tr.step(X.cuda(), y.cuda()))
        o = want[step - 1]
        print(f"  {variant} {dtype} step {step}: loss {loss:.7f} cpu {o['loss']:.7f}")
        assert abs(loss - o["loss"]) <= (1e-4 * abs(o["loss"]) + 1e-5 if dtype == "f32" else 2e-2 * abs(o["loss"]))
        if step == 1:
            for i, n in enumerate(names):
                g = tr.flat.grad_view(i).view(o["grads"][n].shape) / k        # (the bucket holds the sum of the k micro-batches)
                if dtype == "bf16":
                    assert_bf16(g, o["grads"][n].float(), f"bucket d {n}", RM.BF16_GATE)
                else:
                    assert_close_grad(g, o["grads"][n].float(), f"bucket d {n}")
        for n, v in net.state_dict().items():
            d = (v.cpu().double() - o["params"][n]).abs()
            print(f"    after {step}: {n}: max |dp| {float(d.max()):.2e}, mean {float(d.mean()):.2e}")
            assert float(d.max()) <= step * 2.2 * LR, (n, step)
            assert float(d.mean()) <= (2e-6 if dtype == "f32" else 0.1 * LR * step), (n, step)
    # rollout_from >= T feeds nothing: the step is the step it was, bit for bit
    a, b = (rollout_net(pkg, "thin", dtype, True)[0] for _ in range(2))
    ta = FusedTrainer(a, lr=LR, betas=BETAS, halo=HALO, rollout_from=c["T"], **kw)
    tb = FusedTrainer(b, lr=LR, betas=BETAS, halo=HALO, **kw)
    for X, y in batches[:k]:
        la, lb = ta.step(X.cuda(), y.cuda()), tb.step(X.cuda(), y.cuda())
    assert torch.equal(la, lb) and torch.equal(ta.flat.data, tb.flat.data)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("variant", ["sequence-accumulate2", "last-step"])
def test_rollout_trainer_under_the_guarded_allocator(pkg, variant, dtype):
    """tests/test_gpu_memory_contract.py's three runs of two optimizer steps: no store outside an extent, no result from a byte
    the library did not write (the roll-out slab, the one-step d/dx scratch and dh_seq are uninitialised allocations)"""
    from nasa_niswan_amd.trainer import FusedTrainer
    c = CLM.CASES["wide" if variant == "last-step" else "thin"]
    case = "wide" if variant == "last-step" else "thin"
    kw = TRAIN_VARIANTS[variant]
    sq, k = kw.get("sequence_loss", False), kw.get("accumulate_steps", 1)

    def scenario(gt):
        G = (lambda t: t) if gt is None else gt.guard_copy
        net, _ = rollout_net(pkg, case, dtype, True, gt=gt)
        if gt is not None:
            gt.guard_module(net)            # (the case's weights were loaded after make_net guarded the module)
        tr = FusedTrainer(net, lr=1e-3, betas=BETAS, halo=HALO, rollout_from=2, max_grad_norm=0.05, **kw)
        res = {}
        for j, (X, y) in enumerate(_train_batches(c, 2 * k, sq)):
            res[f"loss.{j}"] = tr.step(G(X.cuda()), G(y.cuda())).detach().clone()
        res["bucket"], res["bucket.grad"], res["stats"] = tr.flat.data, tr.flat.grad, tr.stats
        return res
    stack = (c["C"], c["hidden"], c["ks"])
    assert MC.three_runs(f"rollout-trainer-{variant}-{dtype}", scenario, MC.row_stride(stack, (c["H"], c["W"]))) > 0


def test_train_py_rollout_from_end_to_end(pkg, tmp_path, monkeypatch):
    from nasa_niswan_amd import train as T
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--model", "LSTM-ro", "--in-channels", "5", "--hidden-channels", "8", "4", "--kernel-size", "3", "3", "--num-layers", "2",
            "--sequence-length", "4", "--input-size", "12", "16", "--grid", "12", "16", "--batch-size", "2", "--num-epochs", "1",
            "--learning-rate", "1e-4", "--synthetic-steps", "60", "--dtype", "f32", "--snapshot-dir", str(tmp_path / "s"),
            "--cyclic-longitude", "--tracer-input", "--rollout-from", "1"]
    logger = T.main(T.get_arguments(argv))
    assert np.isfinite(logger["MSELoss"]).all() and len(logger["MSELoss"]) >= 1
