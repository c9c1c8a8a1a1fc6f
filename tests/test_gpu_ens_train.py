"""GPU: ensemble training -- the noisy closed loop with the training stash on, nint_ens_loss into the roll-out
slab, the UNCHANGED roll-out backward as its adjoint, and FusedTrainer(ensemble_members=M).

Shapes: closed_loop_model.CASES "thin" (folded input, O = 1) and "wide" (plain input, O = 3): T = 4, rollout_from = 2, N = 2
samples x M = 2 / 3 member lanes on the ragged 13 x 37 grid; f32 and bf16, zero padding and cyclic longitude, plain and
residual head.  Weights: rollout_model.case_params (feedback columns scaled, so the fed term stands out) for the plain head,
residual_model.case_params for the residual one.  References: the library's own open-loop pass on the stored input (bit for
bit), tests/ens_loss_model.py on the device's own head output (bit for bit), tests/ens_train_model.py in f64 under CPU autograd
at the gates of tests/test_gpu_rollout.py (f32: <= 1e-3 * max|grad| + 1e-6; bf16: rel-L2 <= 2e-2 against the f32 model)."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_model as CLM
import ens_loss_model as LM
import ens_train_model as ETM
import residual_model as RES
import rollout_model as RM
import test_gpu_closed_loop as CL
import test_gpu_feedback_noise as FN
from oracle import small_audit as SM
from test_gpu_closed_loop import pkg      # noqa: F401  (the fixture)
from test_gpu_parity import assert_bf16, assert_close_grad

pytestmark = pytest.mark.gpu
BOTH = ("f32", "bf16")
CYC = dict(argvalues=[False, True], ids=["zero-pad", "cyclic"])
RESID = dict(argvalues=[False, True], ids=["plain-head", "residual"])
S, NS, HALO, SEED = 2, 2, (2, 3), 7              # rollout_from, samples, the crop's offset, the noise seed
LR, BETAS = 1e-4, (0.5, 0.999)
NAN = float("nan")


def case_net(pkg, case, dtype, cyclic, residual, gt=None):
    c = CLM.CASES[case]
    net, eng = CL.make_net(pkg, case, dtype, cyclic, gt=gt, **(dict(residual=True) if residual else {}))
    net.load_state_dict((RES if residual else RM).case_params(c))
    return net, eng


def params64(c, residual):
    return (RES if residual else RM).case_params(c, torch.float64)


def batch(c, M, every_step, seed=21):
    """N samples replicated into lanes n*M + m, and y of N samples (never replicated)"""
    rng = np.random.default_rng(seed)
    T, H, W, O = c["T"], c["H"], c["W"], c["O"]
    Hc, Wc = H - 2 * HALO[0], W - 2 * HALO[1]
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    Xs = f(NS, T, c["C"], H, W)
    y = f(*((NS, T, O, Hc, Wc) if every_step else (NS, O, Hc, Wc)))
    return ETM.replicate(Xs, M), y


def sigmas(c):
    return tuple(0.05 * (1 + o) for o in range(c["O"]))


def device_normals(pkg, c, B, draw, seed=SEED):
    """z (T, B, O, H, W) f32 on the CPU from nint_noise_normal under the given key (step0 = lane0 = 0)"""
    from nasa_niswan_amd import _lib
    lib = pkg.load_library()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), c["H"], c["W"], 2) == 0
    out = torch.empty(c["T"] * B, c["O"], c["H"], c["W"], device="cuda")
    assert lib.nint_noise_normal(C.c_void_p(out.data_ptr()), B, c["T"], c["O"], seed, draw, 0, 0, C.byref(g), None) == 0
    torch.cuda.synchronize()
    return out.cpu().view(c["T"], B, c["O"], c["H"], c["W"])


def engine_step(pkg, net, eng, X, y, M, alpha, every_step, fnoise, residual, feed=S):
    """the ensemble step's device calls, driven through the engine, every intermediate kept"""
    from nasa_niswan_amd.loss import EnsembleLoss
    B, T, _, H, W = X.shape
    L, O = len(eng.cfgs), net.conv.weight.shape[0]
    w, b = net.conv.weight, net.conv.bias
    Hc, Wc = y.shape[-2], y.shape[-1]
    ws = eng.acquire(B, T, H, W, True, False)
    try:
        net._pack_weights(eng)
        eng.forward(ws, X, feedback=(w, b, feed), feedback_grad=True, residual=O if residual else False, feedback_noise=fnoise)
        res = dict(xs=ws.xs.clone(), stochastic=ws.feedback.noise is not None)
        for l in range(L):
            res[f"h{l}"] = ws.h[l].clone()
        seq = eng.head_forward_seq(ws, w, b)
        res["seq"] = seq.clone()
        slab = ws.rollout_dpred(eng, O)
        slab.fill_(NAN)
        if not every_step:
            slab[:(T - 1) * B].zero_()
        n = (B // M) * (T if every_step else 1)
        scratch = torch.full((eng.ens_loss_scratch(n, M, O, H, W),), NAN, dtype=torch.float64, device="cuda")
        loss = torch.full((2,), NAN, device="cuda")
        stats, ens = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
        eng.ens_loss(ws, seq, y.contiguous(), slab, M, EnsembleLoss(alpha).on(X.device, O, T if every_step else None), None, scratch, loss,
                     stats, ens, HALO, Hc, Wc, every_step=every_step)
        res.update(l=slab.clone(), loss=loss[:1].clone(), stats=stats, ens=ens)
        eng.rollout_cotangents(ws, w, slab_filled=True, dh_written=False)
        dWs, dbs, _ = eng.backward(ws, False, zero_state_grads=tuple(range(L)), rollout=slab)
        dw, db = eng.head_backward(ws, w, slab, write_dh=False, images=(B, T * B))
        torch.cuda.synchronize()
        g = {}
        for l in range(L):
            g[f"layers.{l}.conv.weight"], g[f"layers.{l}.conv.bias"] = dWs[l].clone(), dbs[l].clone()
        g["conv.weight"], g["conv.bias"] = dw.clone(), db.clone()
        res["grads"] = g
        return res
    finally:
        eng.release(ws)


def model_slab(c, seq, y, M, alpha, every_step):
    """ens_loss_model on the device's own head output -> (the slab (T*B, O, H, W), the model's run)"""
    T, H, W, O = c["T"], c["H"], c["W"], c["O"]
    B = seq.shape[0]
    N = B // M
    Hc, Wc = y.shape[-2], y.shape[-1]
    s6 = seq.cpu().numpy().reshape(N, M, T, O, H, W)
    steps = list(range(T)) if every_step else [T - 1]
    x = np.stack([s6[n, :, t] for n in range(N) for t in steps])[..., HALO[0]:HALO[0] + Hc, HALO[1]:HALO[1] + Wc]
    r = LM.run(np.ascontiguousarray(x), y.cpu().numpy().reshape(N * len(steps), O, Hc, Wc), alpha)
    full = LM.full_images(r["dpred"], H, W, HALO[0], HALO[1]).reshape(N, len(steps), M, O, H, W)
    slab = np.zeros((T, N, M, O, H, W), np.float32)
    for k, t in enumerate(steps):
        slab[t] = full[:, k]
    return slab.reshape(T * B, O, H, W), r


def cpu_grads(c, X, l, cyclic, residual, add, p=None):
    """CPU autograd over the helper's closed loop in f64 (fed values rounded to f32) with the device's slab as the cotangent"""
    B, T, O, H, W = X.shape[0], c["T"], c["O"], c["H"], c["W"]
    p = {k: v.detach().clone().requires_grad_(True) for k, v in (params64(c, residual) if p is None else p).items()}
    r = ETM.forward(X.double(), p, S, cyclic, "f32", add=add, residual=residual)
    dseq = l.cpu().double().view(T, B, O, H, W).transpose(0, 1).reshape(B, T * O, H, W)
    (r["seq"] * dseq).sum().backward()
    return {k: v.grad for k, v in p.items()}


def fb_noise(c, draw):
    from nasa_niswan_amd.engine import InputNoise
    return InputNoise(sigmas(c), seed=SEED, draw=draw)


# ------------------------------------------------------------------ (a) (b) (c): forward contract, slab, the backward as the adjoint
@pytest.mark.parametrize("residual", **RESID)
@pytest.mark.parametrize("cyclic", **CYC)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case,M", [("thin", 2), ("wide", 3), ("thin", 3), ("wide", 2)])
def test_forward_contract_slab_and_bucket_gradients(pkg, case, M, dtype, cyclic, residual):
    c = CLM.CASES[case]
    every_step = M == 2                      # M = 2: a loss term at every step; M = 3: at the last one, the others zeroed
    alpha, draw = (1.0 if M == 2 else 0.5), 0x80000000 | 3
    net, eng = case_net(pkg, case, dtype, cyclic, residual)
    X, y = batch(c, M, every_step)
    B = X.shape[0]
    sig, z = sigmas(c), device_normals(pkg, c, B, draw)
    a = engine_step(pkg, net, eng, X.cuda(), y.cuda(), M, alpha, every_step, fb_noise(c, draw), residual)
    assert a["stochastic"]
    # (a) the noisy training forward is the open-loop pass over the input that holds the stored values, bit for bit
    with torch.no_grad():
        stored = FN.stored_input(c, X, a["seq"], FN.from_step(c, S, B), sig, z)
        o = FN.run(net, eng, stored.cuda(), None, residual=residual)
    for k in ["xs", "seq"] + [f"h{l}" for l in range(len(c["hidden"]))]:
        assert torch.equal(a[k], o[k]), (case, M, dtype, cyclic, residual, k)
    quiet = engine_step(pkg, net, eng, X.cuda(), y.cuda(), M, alpha, every_step, None, residual)
    assert not quiet["stochastic"] and not torch.equal(quiet["seq"], a["seq"])                 # the noise is in fact there
    # (b) the slab after the loss is the model applied to the device's own head output, bit for bit
    want, r = model_slab(c, a["seq"], y, M, alpha, every_step)
    SM.check_equal(a["l"].cpu().numpy(), want, "slab")
    SM.check_equal(a["loss"].cpu().numpy(), np.array([np.float32(LM.finish(a["ens"].cpu().numpy().tolist()[:3] + a["stats"].cpu().numpy().tolist()[:4],
                                                                           M, alpha, r["cnt"])[0])]), "loss_out from the device's sums")
    assert abs(float(a["loss"]) - r["loss"]) <= 1e-6 * abs(r["loss"]) + 1e-9
    # (c) the UNCHANGED roll-out backward is the adjoint of the noisy pass: CPU autograd with the device's slab as the cotangent
    add = (torch.tensor(sig, dtype=torch.float32).view(1, 1, -1, 1, 1) * z)
    ref = cpu_grads(c, X, a["l"], cyclic, residual, add)
    bad = []
    for k, g in a["grads"].items():
        try:
            if dtype == "bf16":
                assert_bf16(g.view(ref[k].shape), ref[k].float(), f"{case} M={M} {dtype} d {k}", RM.BF16_GATE)
            else:
                assert_close_grad(g.view(ref[k].shape), ref[k].float(), f"{case} M={M} {dtype} d {k}")
        except AssertionError as e:
            bad.append(str(e).splitlines()[0])
    # ... and it is NOT the adjoint of the noise-free window on the same cotangent (the noise moved the stash)
    assert not torch.equal(a["grads"]["layers.0.conv.weight"], quiet["grads"]["layers.0.conv.weight"])
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ (d) end to end, f32
# (data seed, step weights, output weights): the seeds were chosen on the CPU reference so that NO cell under a non-zero weight is
# excluded.  Steps before rollout_from hold identical members (the noise has not entered yet), so the sequence case discounts
# them to 0 -- the spin-up use of step weights; the wide case keeps one of its three outputs.
D_CASES = {("thin", 2): (21, [0.0, 0.0, 1.0, 1.0], None), ("wide", 3): (23, None, [0.0, 0.5, 0.0])}


@pytest.mark.parametrize("case,M", sorted(D_CASES))
def test_end_to_end_against_cpu_autograd_of_the_crps(pkg, case, M):
    """FusedTrainer.step in f32 against CPU autograd of the CRPS itself (f64 model, fed values rounded to f32, the noise from
    tests/noise_model.py under the trainer's keys): loss at 1e-4 relative + 1e-5, bucket gradients at <= 1e-3 max|grad| + 1e-6.
    First, on the CPU reference: every |x_i - t| and |x_i - x_j| under a non-zero weight exceeds 2 * (1e-4 |x| + 1e-5), twice
    the f32 output tolerance, so no sign can flip inside it.  Feedback noise sigma[o] = 1 + o.  Measured on the CPU reference:
    thin, M = 2, seed 21: smallest gap 1.279e-04, smallest margin over the bound 8.508e-05;
    wide, M = 3, seed 23: smallest gap 1.310e-04, smallest margin 7.098e-05."""
    from nasa_niswan_amd.loss import EnsembleLoss
    from nasa_niswan_amd.trainer import FusedTrainer
    c = CLM.CASES[case]
    every_step, alpha, cyclic, residual = M == 2, 0.75, True, False
    seed, step_w, out_w = D_CASES[(case, M)]
    X, y = batch(c, M, every_step, seed=seed)
    B, T, O, H, W = X.shape[0], c["T"], c["O"], c["H"], c["W"]
    sig = tuple(1.0 + o for o in range(O))
    add = ETM.feedback_add(sig, B, T, O, H, W, SEED, 0x80000000 | 0)
    p = {k: v.clone().requires_grad_(True) for k, v in params64(c, residual).items()}
    r = ETM.forward(X.double(), p, S, cyclic, "f32", add=add, residual=residual)
    margin, gap = ETM.smallest_gap(r["seq"], y.double(), M, HALO, every_step, O, step_w, out_w)
    print(f"  {case} M={M}: smallest gap {gap:.3e}, smallest margin over twice the tolerance {margin:.3e}")
    assert margin > 0, (gap, margin)
    loss = ETM.crps(r["seq"], y.double(), M, alpha, HALO, every_step, O, step_w, out_w)
    loss.backward()
    net, eng = case_net(pkg, case, "f32", cyclic, residual)
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, rollout_from=S, ensemble_members=M, feedback_noise=sig, noise_seed=SEED,
                      sequence_loss=every_step, ensemble_loss=EnsembleLoss(alpha, output_weights=out_w, step_weights=step_w))
    got = float(tr.step(X.cuda(), y.cuda()))
    print(f"  {case} M={M}: loss {got:.7f} cpu {float(loss):.7f}")
    assert abs(got - float(loss)) <= 1e-4 * abs(float(loss)) + 1e-5
    for i, (n, _) in enumerate(net.named_parameters()):
        assert_close_grad(tr.flat.grad_view(i).view(p[n].shape), p[n].grad.float(), f"{case} M={M} bucket d {n}")
    st = tr.ensemble_stats()
    assert abs(st["crps"] - float(loss)) <= 1e-4 * abs(float(loss)) + 1e-5 and st["spread"] > 0 and st["rmse_mean"] > 0
    lm, r2 = tr.epoch_stats()
    assert abs(lm - float(loss)) <= 1e-4 * abs(float(loss)) + 1e-5 and np.isfinite(r2)
    # refusals that need the lanes
    with pytest.raises(ValueError, match="whole ensembles"):
        tr.step(X[:B - 1].cuda(), y.cuda())
    with pytest.raises(ValueError, match="never replicated"):
        tr.step(X.cuda(), ETM.replicate(y, M).cuda())


# ------------------------------------------------------------------ (e) collapse: identical members
@pytest.mark.parametrize("case,M", [("thin", 2), ("wide", 3)])
def test_identical_members_collapse_onto_the_l1_rollout_step(pkg, case, M):
    """Identical members, built directly through the engine (no noise at all; the trainer refuses that): D = 0 and R = 0, so the
    gradient is that of the L1-only LossSpec(0, 1, 0) roll-out step on the same replicated lanes -- (1/M) sgn(x - t) / (N O Hc Wc)
    per member against sgn(x - t) / (N M O Hc Wc) per lane."""
    from nasa_niswan_amd.loss import LossSpec
    from nasa_niswan_amd.trainer import FusedTrainer
    c = CLM.CASES[case]
    X, y = batch(c, M, False)
    a_net, a_eng = case_net(pkg, case, "f32", True, False)
    a = engine_step(pkg, a_net, a_eng, X.cuda(), y.cuda(), M, 1.0, False, None, False)
    b_net, _ = case_net(pkg, case, "f32", True, False)
    tr = FusedTrainer(b_net, lr=LR, betas=BETAS, halo=HALO, rollout_from=S, loss=LossSpec(0, 1, 0))
    tr.step(X.cuda(), ETM.replicate(y, M).cuda())
    same = True
    for i, (n, _) in enumerate(b_net.named_parameters()):
        g, ref = a["grads"][n].reshape(-1), tr.flat.grad_view(i).reshape(-1)
        assert_close_grad(g, ref, f"{case} M={M} collapse d {n}")
        same = same and torch.equal(g, ref)
    print(f"  {case} M={M}: bit equality with the L1 roll-out step: {same}")
    if M == 2:
        # 1 / M is a power of two: (sgn / 2) * (1 / cnt) * 1 against sgn * (1 / (2 cnt)) -- the same f32 cotangent, the same launches
        assert same


# ------------------------------------------------------------------ (f) training works
@pytest.mark.parametrize("dtype", BOTH)
def test_three_trainer_steps_lower_the_crps_and_follow_cpu_adam(pkg, dtype):
    """three FusedTrainer.step calls on one batch lower ensemble_stats()['crps']; the parameters after each equal a CPU Adam on
    the gradients of (c) -- CPU autograd over the helper's closed loop with the device's own slab as the cotangent -- at the
    tolerances of tests/test_gpu_seq_train.py (max |dp| <= k * 2.2 * lr; mean |dp| <= 2e-6 in f32, 0.1 * lr * k in bf16).
    Every step draws new noise, so the CRPS of step k is that of (weights k, draw k): at the Adam check's lr = 1e-4 and sigma =
    0.05 the draw moves it by 1e-3 and three steps lower it by less -- the CPU model gives 1.13545, 1.13655, 1.13612 there, and
    the device the same digits.  The decrease is therefore asserted on a second trainer whose steps outweigh the draw, lr = 1e-3
    and sigma = 0.005 (CPU model: 1.15159, 1.15026, 1.14879)."""
    from nasa_niswan_amd.trainer import FusedTrainer
    case, M, cyclic, residual = "thin", 2, True, True
    c = CLM.CASES[case]
    X, y = batch(c, M, True)
    B, T, O, H, W = X.shape[0], c["T"], c["O"], c["H"], c["W"]
    sig = sigmas(c)
    net, eng = case_net(pkg, case, dtype, cyclic, residual)
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, rollout_from=S, ensemble_members=M, feedback_noise=sig, noise_seed=SEED,
                      sequence_loss=True)
    kept, inner = [], eng.ens_loss

    def spy(ws, seq, yv, slab, *a, **kw):
        inner(ws, seq, yv, slab, *a, **kw)
        kept.append(slab.clone())
    eng.ens_loss = spy
    p = {k: v.clone().requires_grad_(True) for k, v in params64(c, residual).items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR, betas=BETAS)
    crps = []
    try:
        for step in (1, 2, 3):
            tr.step(X.cuda(), y.cuda())
            crps.append(tr.ensemble_stats(reset=True)["crps"])
            tr.reset_stats()
            add = torch.tensor(sig, dtype=torch.float32).view(1, 1, -1, 1, 1) * device_normals(pkg, c, B, 0x80000000 | (step - 1))
            g = cpu_grads(c, X, kept[-1], cyclic, residual, add, p={k: v.detach() for k, v in p.items()})
            opt.zero_grad()
            for k in p:
                p[k].grad = g[k]
            opt.step()
            for n, v in net.state_dict().items():
                d = (v.cpu().double() - p[n].detach()).abs()
                print(f"    after {step}: {n}: max |dp| {float(d.max()):.2e}, mean {float(d.mean()):.2e}")
                assert float(d.max()) <= step * 2.2 * LR, (n, step)
                assert float(d.mean()) <= (2e-6 if dtype == "f32" else 0.1 * LR * step), (n, step)
    finally:
        del eng.ens_loss
    print(f"  crps over three steps at lr {LR}, sigma {sig}: {crps}")
    net2, _ = case_net(pkg, case, dtype, cyclic, residual)
    tr2 = FusedTrainer(net2, lr=1e-3, betas=BETAS, halo=HALO, rollout_from=S, ensemble_members=M, feedback_noise=0.005, noise_seed=SEED,
                       sequence_loss=True)
    crps = []
    for _ in range(3):
        tr2.step(X.cuda(), y.cuda())
        crps.append(tr2.ensemble_stats(reset=True)["crps"])
    print(f"  crps over three steps at lr 1e-3, sigma 0.005: {crps}")
    assert crps[0] > crps[1] > crps[2], crps


# ------------------------------------------------------------------ (g) the old paths
def _plan(ws):
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    s = ws.seq
    cap = 8 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    n = lib.nint_debug_seq_plan_rollout(C.byref(s), C.byref(ws.feedback.fb), recs, cap)
    assert 0 < n <= cap, n
    return bytes(recs)[:n * C.sizeof(_lib.NintLaunchRec)]


def test_the_old_paths_stay(pkg, monkeypatch):
    """a trainer built without ensemble_members runs the roll-out step it ran: it reaches neither the new entry nor the
    stochastic forward, two such trainers agree bit for bit, and the roll-out backward planned behind a noisy window is, record
    for record, the one planned behind the noise-free window; the autograd route still refuses the combination"""
    from nasa_niswan_amd.engine import InputNoise, SeqEngine
    from nasa_niswan_amd.trainer import FusedTrainer
    c = CLM.CASES["thin"]
    X, y = batch(c, 2, True)
    yl = ETM.replicate(y, 2)
    called, plans, reached = [], [], []
    inner_pass, inner_loss = SeqEngine._seq_pass, SeqEngine.ens_loss

    def spy_pass(self, ws, bwd, rg=None):
        called.append(ws.feedback.noise is not None)
        if rg is not None:
            plans.append(_plan(ws))
        return inner_pass(self, ws, bwd, rg)

    def spy_loss(self, *a, **k):
        reached.append(1)
        return inner_loss(self, *a, **k)
    monkeypatch.setattr(SeqEngine, "_seq_pass", spy_pass)
    monkeypatch.setattr(SeqEngine, "ens_loss", spy_loss)
    nets = [case_net(pkg, "thin", "bf16", True, False)[0] for _ in range(3)]
    trs = [FusedTrainer(n, lr=LR, betas=BETAS, halo=HALO, rollout_from=S, sequence_loss=True) for n in nets[:2]]
    la, lb = (t.step(X.cuda(), yl.cuda()) for t in trs)
    assert called == [False] * 4 and not reached and torch.equal(la, lb) and torch.equal(trs[0].flat.grad, trs[1].flat.grad)
    assert trs[0].ens_out is None
    with pytest.raises(ValueError, match="ensemble_members"):
        trs[0].ensemble_stats()
    ens = FusedTrainer(nets[2], lr=LR, betas=BETAS, halo=HALO, rollout_from=S, sequence_loss=True, ensemble_members=2, feedback_noise=0.05)
    ens.step(X.cuda(), y.cuda())
    assert called == [False] * 4 + [True, True] and reached == [1] and len(plans) == 3 and plans[0] == plans[1] == plans[2]
    with pytest.raises(ValueError, match="feedback_grad"):
        nets[0](X.cuda(), free_from=1, feedback_grad=True, feedback_noise=InputNoise(0.1))
