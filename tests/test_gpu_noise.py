"""GPU: the input noise -- nint_noise_normal, nint_input_noise, ``ConvLSTM.forward(input_noise=...)`` and
``FusedTrainer(input_noise=...)``.

Shapes: the closed-loop entry shapes, where this store pattern can go wrong -- 13 x 37 (the slack holds the wrap), 13 x 64 (no
slack), 3 x 261 (a thread's second pixel); spans Cx 4 / n 1 folded k = 5, Cx 3 / n 3 folded (every channel), Cx 40 / c0 37 / n 3
plain (an odd first channel and a 16-byte group straddle in bf16), Cx 8 / c0 1 / n 6 (a Philox tail of two channels), and Cx 600
/ c0 3 / n 590 (a span cut into two launches and a row cut into two workgroups); B = 2, T = 3, x_n0 = 1; f32 and bf16, zero
padding and cyclic longitude.
References: tests/noise_model.py -- the f64 normals for the generator, the numpy float32 update on the device's own z for the slab
(bit for bit, the whole slab); the module on a host-built noisy input (bit for bit)."""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_model as NM
import residual_model as RES
import test_gpu_bptt_segments as SEG
import test_gpu_memory_contract as MC
from test_gpu_closed_loop import pkg                                  # noqa: F401  (the fixture)
from test_gpu_residual import BETAS, HALO, LR, _train_batches, res_net

pytestmark = pytest.mark.gpu
BOTH = ("f32", "bf16")
GRIDS = [(13, 37), (13, 64), (3, 261)]
GRID_IDS = ["13x37", "13x64", "3x261"]
B_, T_, X_N0 = 2, 3, 1
KEY = dict(seed=0x9E3779B9, draw=7, step0=0xfffffffe, lane0=5)          # (step0 + t wraps mod 2^32 inside the window)
# (name, Cx, c0, n, k of a folded slab or 0, sigma)
SPANS = [("thin-folded", 4, 3, 1, 5, (0.5,)), ("all-folded", 3, 0, 3, 5, (0.5, 0.25, 1.0)), ("plain-straddle", 40, 37, 3, 0, (1.0, 0.5, 0.25)),
         ("plain-tail2", 8, 1, 6, 0, (0.5, 0.25, 0.0, 1.0, 2.0, 0.125))]
SPAN_IDS = [s[0] for s in SPANS]


def _lib():
    from nasa_niswan_amd import _lib as L
    return L, L.load()


def device_z(lib, g, B, T, n, key, ex=None):
    """(T*B, n, H, W) f32 numpy: nint_noise_normal"""
    from nasa_niswan_amd._lib import stream_ptr
    numel = B * T * n * g.H * g.W
    out = torch.empty(numel, dtype=torch.float32, device="cuda") if ex is None else ex.empty(numel, torch.float32, slack=0)
    assert lib.nint_noise_normal(MC.P(out), B, T, n, key["seed"], key["draw"], key["step0"], key["lane0"], C.byref(g), stream_ptr()) == 0
    torch.cuda.synchronize()
    return out[:numel].view(T * B, n, g.H, g.W).cpu().numpy()


# ====================================================================== 1. the generator
WORST = {}


@pytest.mark.parametrize("n", [1, 3, 6, 32])
@pytest.mark.parametrize("H,W", GRIDS, ids=GRID_IDS)
def test_generator_against_the_f64_model(pkg, H, W, n):
    """|dz| <= 2^-20 * max(1, r): about four times the sum of HIP's documented bounds for logf (1 ulp), sqrtf (1 ulp), sincospif
    (2 ulp) and two roundings, relative to r; a wrong word, key or pair moves z by O(1).  Exactly sized poisoned output: every
    element is written, nothing behind it."""
    L, lib = _lib()
    g = MC._geom(lib, H, W, 2)
    ex = MC.Exact(False)
    got = device_z(lib, g, B_, T_, n, KEY, ex)
    assert ex.done() > 0
    want, r = NM.z_images(B_, T_, n, H, W, with_r=True, **KEY)
    assert np.isfinite(got).all()
    ratio = float((np.abs(got.astype(np.float64) - want) / (2.0 ** -20 * np.maximum(1.0, r))).max())
    WORST[(H, W, n)] = ratio
    print(f"  generator {H}x{W} n {n}: worst |dz| / (2^-20 max(1, r)) = {ratio:.4f} (over all cases so far {max(WORST.values()):.4f})")
    assert ratio <= 1.0


def test_generator_keys(pkg):
    """the noise is a function of (seed, draw, lane, step, o, pixel) alone: lanes [B, 2B) of a 2B batch are a B batch at lane0 +
    B, steps [1, T) are a T - 1 window at step0 + 1, and the first n channels of a wider span are the narrower span, bit for bit;
    another seed or draw is another field"""
    L, lib = _lib()
    g = MC._geom(lib, 13, 37, 2)
    z = device_z(lib, g, 4, 3, 6, KEY).reshape(3, 4, 6, 13, 37)
    hi = device_z(lib, g, 2, 3, 6, dict(KEY, lane0=KEY["lane0"] + 2)).reshape(3, 2, 6, 13, 37)
    assert z[:, 2:].tobytes() == hi.tobytes()
    late = device_z(lib, g, 4, 2, 6, dict(KEY, step0=(KEY["step0"] + 1) & 0xffffffff)).reshape(2, 4, 6, 13, 37)
    assert z[1:].tobytes() == late.tobytes()
    few = device_z(lib, g, 4, 3, 3, KEY).reshape(3, 4, 3, 13, 37)
    assert z[:, :, :3].tobytes() == few.tobytes()
    for k in ("seed", "draw"):
        other = device_z(lib, g, 4, 3, 6, dict(KEY, **{k: KEY[k] + 1}))
        assert abs(float((other.ravel() * z.ravel()).mean())) * z.size ** .5 <= 5


# ====================================================================== 2. the slab update
def _slab_case(lib, L, H, W, Cx, c0, n, k, sigma, dt, cyc):
    from nasa_niswan_amd._lib import stream_ptr
    bf16 = dt == 1
    g = MC._geom(lib, H, W, 2)
    kc = lib.nint_kc(dt)
    Cxp = (max(k, 1) * Cx + kc - 1) // kc * kc
    rng = np.random.default_rng(1000 * H + W + Cx)
    N = X_N0 + B_ * T_ + 1                                    # an image in front and one behind: both stay
    src = rng.standard_normal((N, Cx, H, W)).astype(np.float32)
    src[X_N0, :, 0, 0] = -0.0
    slab = NM.make_slab(rng, src, g.Hh, g.Wh, g.P, Cxp, k, cyc, bf16)            # junk in every halo, slack column and pad channel
    ex = MC.Exact(False, g.Wh * Cxp * (2 if bf16 else 4))
    z = device_z(lib, g, B_, T_, n, KEY, ex)
    dev = ex.copy(torch.from_numpy(slab.view(np.uint8).reshape(-1).copy()))
    sg = ex.copy(torch.tensor(sigma, dtype=torch.float32))
    rc = lib.nint_input_noise(MC.P(dev), X_N0, B_, T_, Cx, Cxp, c0, n, MC.P(sg), k, cyc, KEY["seed"], KEY["draw"], KEY["step0"],
                              KEY["lane0"], C.byref(g), dt, stream_ptr())
    assert rc == 0
    assert ex.done() > 0                                      # (synchronises; the guards around slab, sigma and z are whole)
    got = dev.cpu().numpy().view(slab.dtype).reshape(slab.shape)
    want = NM.slab_update(slab, z, X_N0, Cx, c0, n, sigma, k, cyc, g.P, H, W)
    return slab, got, want, g


@pytest.mark.parametrize("cyc", [0, 1], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dt", [0, 1], ids=BOTH)
@pytest.mark.parametrize("H,W", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("name,Cx,c0,n,k,sigma", SPANS, ids=SPAN_IDS)
def test_slab_update_is_the_numpy_update_on_the_devices_z(pkg, name, Cx, c0, n, k, sigma, H, W, dt, cyc):
    """the whole slab, byte for byte: so every byte outside the span -- junk halo, slack, pad channels, the other channels, the
    images in front and behind -- is unchanged, fold copies agree, out-of-row copies stay 0 and sigma = 0 keeps -0.0"""
    L, lib = _lib()
    slab, got, want, g = _slab_case(lib, L, H, W, Cx, c0, n, k, sigma, dt, cyc)
    assert want.tobytes() != slab.tobytes()
    bad = np.argwhere(got.view(np.uint16 if dt else np.uint32) != want.view(np.uint16 if dt else np.uint32))
    assert len(bad) == 0, (name, len(bad), bad[:8].tolist())
    assert got[0].tobytes() == slab[0].tobytes() and got[-1].tobytes() == slab[-1].tobytes()


@pytest.mark.parametrize("dt", [0, 1], ids=BOTH)
def test_a_long_span_runs_in_pieces(pkg, dt):
    """no shape limit: n = 590 of Cx = 600 from an odd channel on 3 x 37 -- two launches (the second starts on an odd channel:
    in bf16 the two share a dword, updated in stream order) and two workgroups a row"""
    L, lib = _lib()
    sigma = tuple(0.25 + 0.125 * (o % 5) for o in range(590))
    slab, got, want, g = _slab_case(lib, L, 3, 37, 600, 3, 590, 0, sigma, dt, 1)
    assert got.tobytes() == want.tobytes() and want.tobytes() != slab.tobytes()


# ====================================================================== 3. the module
def _noise(O_, **kw):
    from nasa_niswan_amd.engine import InputNoise
    std = tuple(0.05 * (1 + o) for o in range(O_))
    return InputNoise(std, seed=11, draw=2, step0=3, lane0=5, **kw), std


def _run(net, x, **kw):
    """pred, seq, the returned state and every gradient of one call, as a flat dict of tensors"""
    x = x.clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    pred, seq, state = net(x, return_state=True, **kw)
    gen = torch.Generator(device="cuda").manual_seed(3)
    r = lambda t: torch.randn(t.shape, generator=gen, device="cuda")
    loss = (pred * r(pred)).sum() + (seq * r(seq)).sum() + sum((h * r(h)).sum() + (c * r(c)).sum() for h, c in state)
    loss.backward()
    out = dict(pred=pred.detach(), seq=seq.detach(), dx=x.grad)
    for l, (h, c) in enumerate(state):
        out[f"h{l}"], out[f"c{l}"] = h.detach(), c.detach()
    for n, p in net.named_parameters():
        out["d " + n] = p.grad.clone()
    return out


@pytest.mark.parametrize("variant", ["open", "free_from-2", "residual", "residual-free_from-2"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", ["thin", "wide"])
def test_module_with_noise_is_the_module_on_the_noisy_input(pkg, case, dtype, variant):
    """net(x, input_noise=N) against net(x') with x' built on the host from the device's z: pred, seq, the returned state and every
    gradient, x.grad included, bit for bit -- open loop, under free_from = 2 (the fed steps overwrite their noise) and with the
    residual head (the base of an unfed step is the noisy stored value)"""
    L, lib = _lib()
    c = RES.CASES[case]
    Bc, Tc, O_, Cc = c["B"], c["T"], c["O"], c["C"]
    assert (Bc, Tc) == (2, 4)
    net, eng = res_net(pkg, case, dtype, case == "thin", residual=variant.startswith("residual"), return_sequence=True)
    X = RES.case_data(c)["X"]
    N, std = _noise(O_)
    g = MC._geom(lib, c["H"], c["W"], 2)
    z = device_z(lib, g, Bc, Tc, O_, dict(seed=N.seed, draw=N.draw, step0=N.step0, lane0=N.lane0))
    X2 = torch.from_numpy(NM.noisy_input(X.numpy(), z, Cc - O_, std, dtype == "bf16"))
    assert not torch.equal(X2, X) and torch.equal(X2[:, :, :Cc - O_], X[:, :, :Cc - O_])
    kw = dict(free_from=2, feedback_grad=True) if variant.endswith("free_from-2") else {}
    a = _run(net, X.cuda(), input_noise=N, **kw)
    b = _run(net, X2.cuda(), **kw)
    clean = _run(net, X.cuda(), **kw)
    for k in a:
        assert torch.equal(a[k], b[k]), (case, dtype, variant, k)
    assert not torch.equal(a["pred"], clean["pred"])
    # None and an all-zero std are the call without the argument; an explicit span equals the default one
    from nasa_niswan_amd.engine import InputNoise
    for nz in (None, InputNoise(0.0), InputNoise((0.0,) * O_)):
        d = _run(net, X.cuda(), input_noise=nz, **kw)
        assert all(torch.equal(d[k], clean[k]) for k in clean)
    e = _run(net, X.cuda(), input_noise=_noise(O_, channels=(Cc - O_, O_))[0], **kw)
    assert all(torch.equal(e[k], a[k]) for k in a)


# ====================================================================== 4. the trainer
class Launches:
    """the nint_input_noise calls of a block: (draw, step0, lane0) of each"""

    def __init__(self, monkeypatch):
        from nasa_niswan_amd.engine import SeqEngine
        self.calls = []
        inner = SeqEngine.input_noise

        def spy(eng, ws, noise, *a, **k):
            self.calls.append((noise.draw, noise.step0, noise.lane0))
            return inner(eng, ws, noise, *a, **k)
        monkeypatch.setattr(SeqEngine, "input_noise", spy)


def _trainer(pkg, dtype="f32", **kw):
    from nasa_niswan_amd.trainer import FusedTrainer
    net, _ = res_net(pkg, "thin", dtype, True)
    return FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, **kw), net


def _losses(tr, batches):
    return [tr.step(X.cuda(), y.cuda()).clone() for X, y in batches]


def test_trainer_seeds_lanes_and_the_step_without_noise(pkg, monkeypatch):
    c = RES.CASES["thin"]
    batches = _train_batches(c, 3, False)
    spy = Launches(monkeypatch)
    a = _losses(_trainer(pkg, input_noise=0.1, noise_seed=5)[0], batches)
    assert spy.calls == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]            # one launch a step: draw = the count of step() calls
    b = _losses(_trainer(pkg, input_noise=0.1, noise_seed=5)[0], batches)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    other = _losses(_trainer(pkg, input_noise=0.1, noise_seed=6)[0], batches)
    assert not any(torch.equal(u, v) for u, v in zip(a, other))
    # another rank: lane0 = rank * B under the same seed (a one-rank stand-in for the process group: nothing is exchanged)
    import types
    tr, _ = _trainer(pkg, input_noise=0.1, noise_seed=5)
    tr.distributed, tr.world = True, 1
    tr.dist = types.SimpleNamespace(get_rank=lambda pg=None: 1, all_reduce=lambda *a, **k: None, ReduceOp=types.SimpleNamespace(SUM=None))
    spy.calls.clear()
    lane = _losses(tr, batches)
    assert spy.calls == [(0, 0, c["B"]), (1, 0, c["B"]), (2, 0, c["B"])]
    assert not any(torch.equal(u, v) for u, v in zip(a, lane))
    # None and 0.0: the step it was, and no launch
    spy.calls.clear()
    plain = _losses(_trainer(pkg)[0], batches)
    for kw in (dict(input_noise=None), dict(input_noise=0.0), dict(input_noise=0.0, noise_seed=9)):
        got = _losses(_trainer(pkg, **kw)[0], batches)
        assert all(torch.equal(u, v) for u, v in zip(plain, got)), kw
    assert spy.calls == []
    assert not torch.equal(plain[0], a[0])
    # set_input_noise switches it; evaluate() never adds noise
    tr, _ = _trainer(pkg, input_noise=0.1, noise_seed=5)
    X, y = batches[0]
    tr.evaluate(X.cuda(), y.cuda())
    assert spy.calls == []
    tr.set_input_noise(None)
    assert torch.equal(tr.step(X.cuda(), y.cuda()), plain[0]) and spy.calls == []


def test_trainer_kernel_names_under_the_profiler(pkg):
    """the launch count by kernel name: a step with noise runs input_noise_kernel once, a step with None or 0.0 never"""
    from torch.profiler import ProfilerActivity, profile
    c = RES.CASES["thin"]
    (X, y), = _train_batches(c, 1, False)
    counts = {}
    for name, kw in (("none", {}), ("zero", dict(input_noise=0.0)), ("noise", dict(input_noise=0.1))):
        tr, _ = _trainer(pkg, **kw)
        tr.step(X.cuda(), y.cuda())
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            tr.step(X.cuda(), y.cuda())
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        assert len(names) >= 5, ("the profiler saw no kernels of the step", names)
        counts[name] = sum("input_noise_kernel" in n for n in names)
    print("  input_noise_kernel launches per step:", counts)
    assert counts == dict(none=0, zero=0, noise=1)


@pytest.mark.parametrize("dtype", BOTH)
def test_trainer_segments_see_the_whole_windows_noise(pkg, dtype, monkeypatch):
    """bptt_segments = 2 against the whole window, both with noise: the loss bit for bit (every pass over a segment -- sweep and
    recompute -- carries its start as step0), the gradients inside the gates of tests/test_gpu_bptt_segments.py for the same
    comparison (f32: max|a - b| <= DEV_F32_GATE * max|b| per parameter; bf16: its check())"""
    c = RES.CASES["thin"]
    (X, y), = _train_batches(c, 1, False)
    spy = Launches(monkeypatch)
    runs = {}
    for name, kw in (("whole", {}), ("segments", dict(bptt_segments=2))):
        tr, net = _trainer(pkg, dtype, input_noise=0.1, noise_seed=5, **kw)
        loss = tr.step(X.cuda(), y.cuda()).clone()
        runs[name] = (loss, {n: tr.flat.grad_view(i).view(p.shape).clone() for i, (n, p) in enumerate(net.named_parameters())})
    S = c["T"] // 2
    assert spy.calls == [(0, 0, 0), (0, 0, 0), (0, S, 0), (0, 0, 0)]          # whole | sweep of segment 0, segment 1, recompute of 0
    assert torch.equal(runs["whole"][0], runs["segments"][0])
    clean = _trainer(pkg, dtype)[0].step(X.cuda(), y.cuda())
    assert not torch.equal(clean, runs["whole"][0])
    res, ref = runs["segments"][1], runs["whole"][1]
    if dtype == "f32":
        for k in res:
            worst = float((res[k].double() - ref[k].double()).abs().max()) / float(ref[k].double().abs().max())
            print(f"  {k}: segmented vs whole max abs / max {worst:.3e}")
            assert worst <= SEG.DEV_F32_GATE, (k, worst)
    SEG.check(res, ref, dtype)


@pytest.mark.parametrize("name,kw", [("rollout", dict(rollout_from=1)), ("sampled", dict(rollout_from=1, sampling_prob=0.5, sampling_seed=4)),
                                     ("sequence-loss", dict(sequence_loss=True)), ("stateful", dict(stateful=True)),
                                     ("frozen", dict(freeze_layers=1)), ("guards", dict(max_grad_norm=0.05, skip_nonfinite=True))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_trainer_options_compose_with_noise(pkg, name, kw, monkeypatch):
    """every option runs with noise, one launch a step, reproducibly under one seed, and not as the step without noise"""
    c = RES.CASES["thin"]
    batches = _train_batches(c, 2, bool(kw.get("sequence_loss")))
    spy = Launches(monkeypatch)
    a = _losses(_trainer(pkg, input_noise=0.1, noise_seed=5, **kw)[0], batches)
    assert [d for d, _, _ in spy.calls] == [0, 1]
    b = _losses(_trainer(pkg, input_noise=0.1, noise_seed=5, **kw)[0], batches)
    clean = _losses(_trainer(pkg, **kw)[0], batches)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and all(bool(torch.isfinite(u)) for u in a)
    assert not any(torch.equal(u, v) for u, v in zip(a, clean))


def test_trainer_takes_a_slab_batch_with_noise(pkg):
    """a SlabBatch window (the preproc kernel writes the slab; no f32 tensor exists) against the same window given as a tensor,
    whole and in two segments, all with noise on channels [1, 4): the loss bit for bit in all four, the bucket bit for bit between
    the two inputs of a plan"""
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from nasa_niswan_amd.trainer import FusedTrainer
    ds = SyntheticE33OMA_CRNN("train", padding=(12, 16), in_channels=5, sequence_length=4, n_steps=60, grid=(8, 12), device="cuda")
    out = {}
    for seg in (None, 2):
        for get in (ds.slab_batch, ds.device_batch):
            X, y = get([1, 9])
            tr = FusedTrainer(SEG.make_net(pkg, "two", "bf16"), lr=1e-3, halo=(2, 2), bptt_segments=seg, input_noise=(0.1, 0.0, 0.2),
                              noise_channels=(1, 3), noise_seed=4)
            out[(seg, get.__name__)] = (tr.step(X, y).clone(), tr.flat.grad.clone())
        a, b = out[(seg, "slab_batch")], out[(seg, "device_batch")]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), seg
    assert torch.equal(out[(None, "slab_batch")][0], out[(2, "slab_batch")][0])
    X, y = ds.slab_batch([1, 9])
    clean = FusedTrainer(SEG.make_net(pkg, "two", "bf16"), lr=1e-3, halo=(2, 2)).step(X, y)
    assert not torch.equal(clean, out[(None, "slab_batch")][0])


def test_trainer_micro_batches_draw_apart(pkg, monkeypatch):
    """accumulate_steps = 2: the two micro-batches of a group carry draw 0 and 1 -- the same batch twice sees two noises"""
    c = RES.CASES["thin"]
    (X, y), = _train_batches(c, 1, False)
    spy = Launches(monkeypatch)
    tr, _ = _trainer(pkg, input_noise=0.1, noise_seed=5, accumulate_steps=2)
    l0 = tr.step(X.cuda(), y.cuda()).clone()
    l1 = tr.step(X.cuda(), y.cuda()).clone()
    assert [d for d, _, _ in spy.calls] == [0, 1]
    assert not torch.equal(l0, l1)
    one, _ = _trainer(pkg, input_noise=0.1, noise_seed=5)
    assert torch.equal(one.step(X.cuda(), y.cuda()), l0)
