"""Fine-tuning on the MI355X: nint_seq.train_from (BPTT stops above the frozen layers), the grouped AdamW kernels, and
FusedTrainer / the autograd path / two ranks on top of them.

Shapes: the stack 5 -> [64, 32, 16], k [5, 3, 3], 2 outputs, on a padded grid of 20 x 40 -- half a tile each way (2.5
eight-row tiles, 2.5 sixteen-column tiles), so every launch has a leftover strip -- B = 2, T = 3, f32 and bf16."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import finetune_model as FM
import grad_clip_model as GM

pytestmark = pytest.mark.gpu
CIN, HIDDEN, KS, OUT = 5, [64, 32, 16], [5, 3, 3], 2
L = 3
B, T, H, W = 2, 3, 20, 40
HALO, HC, WC = (2, 4), 16, 32
SENTINEL = 12345.678


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


@pytest.fixture(scope="module")
def data():
    """the parameters, one batch, the cotangents, and the CPU oracle's gradients of sum(pred * Rp) -- computed once"""
    from oracle import convlstm_oracle as O
    params = O.synth_params(CIN, HIDDEN, KS, L, out_channels=OUT, seed=31)
    rng = np.random.default_rng(31)
    X = torch.from_numpy(rng.standard_normal((B, T, CIN, H, W)).astype(np.float32))
    Rp = torch.from_numpy(rng.standard_normal((B, OUT, H, W)).astype(np.float32))
    Rh = torch.from_numpy(rng.standard_normal((B, HIDDEN[-1], H, W)).astype(np.float32))
    leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    Xl = X.clone().requires_grad_(True)
    (O.convlstm_forward(Xl, leaf) * Rp).sum().backward()
    grads = {k: v.grad.clone() for k, v in leaf.items()}
    return dict(params=params, X=X, Rp=Rp, Rh=Rh, grads=grads, dX=Xl.grad.clone())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def check_grad(got, ref, dtype, what):
    """the standing tolerances of DESIGN section 2: f32 max-abs <= 1e-3 of the gradient's max, bf16 rel-L2 <= 2e-2"""
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    if dtype == "f32":
        e, m = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"  {what}: max abs err {e:.3e}, bound {1e-3 * m + 1e-6:.3e}")
        assert e <= 1e-3 * m + 1e-6, what
    else:
        r = float((got - ref).norm() / ref.norm())
        print(f"  {what}: rel-L2 {r:.3e}, bound 2e-2")
        assert r <= 2e-2, what


class Knobs:
    """engine switches for engines built inside the block"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from nasa_niswan_amd import engine
        self.old = {k: getattr(engine, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(engine, k, v)

    def __exit__(self, *a):
        from nasa_niswan_amd import engine
        for k, v in self.old.items():
            setattr(engine, k, v)


def make_engine(params, dtype, first=0):
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    cin = [CIN] + HIDDEN[:-1]
    eng = SeqEngine([LayerCfg(cin[l], HIDDEN[l], KS[l]) for l in range(first, L)], dtype, "cuda")
    Ws = [params[f"layers.{l}.conv.weight"].cuda() for l in range(first, L)]
    bs = [params[f"layers.{l}.conv.bias"].cuda() for l in range(first, L)]
    eng.pack_weights(Ws, bs)
    return eng


def h_of_every_step(eng, ws, l):
    """(B, T, Ch, H, W) f32: layer l's hidden state of every step, unpacked from its slab"""
    return torch.stack([eng._unpack_h(l, ws.h[l].data_ptr(), ws.B, ws.g, (t + 1) * ws.B) for t in range(ws.T)], dim=1)


# =========================================================================== 5. bit identity with the sub-stack
@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_frozen_pass_equals_the_sub_stack_engine_bit_for_bit(pkg, data, dtype, f):
    with Knobs(FORCE_TILE_ROWS=8, FORCE_WAVE=0):
        eng = make_engine(data["params"], dtype)
        sub = make_engine(data["params"], dtype, first=f)
        assert not sub.cfgs[0].xfold
        with eng.window(B, T, H, W, True, False, f) as ws:
            eng.forward(ws, data["X"].cuda())
            eng.set_dstate(ws, L - 1, "h", data["Rh"].cuda())
            dWs, dbs, _ = eng.backward(ws, False, zero_state_grads=range(L), train_from=f)
            below = h_of_every_step(eng, ws, f - 1)
        with sub.window(B, T, H, W, True, False) as ws2:
            sub.forward(ws2, below)
            sub.set_dstate(ws2, L - 1 - f, "h", data["Rh"].cuda())
            sWs, sbs, _ = sub.backward(ws2, False, zero_state_grads=range(L - f))
        torch.cuda.synchronize()
        assert dWs[:f] == [None] * f and dbs[:f] == [None] * f
        for l in range(f, L):
            assert float(dWs[l].abs().max()) > 0
            assert bits(dWs[l]) == bits(sWs[l - f]), f"dW of layer {l}"
            assert bits(dbs[l]) == bits(sbs[l - f]), f"db of layer {l}"


# =========================================================================== 6. the same gradients as the unfrozen pass
def bucket_run(eng, data, f, accumulate, prefill):
    """forward, head backward of sum(pred * Rp), BPTT with train_from = f into a flat bucket pre-filled with `prefill`"""
    p = data["params"]
    shapes = [p[f"layers.{l}.conv.{n}"].shape for l in range(L) for n in ("weight", "bias")] + [p["conv.weight"].shape, p["conv.bias"].shape]
    sizes = [int(np.prod(s)) for s in shapes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    bucket = prefill.clone() if torch.is_tensor(prefill) else torch.full((offs[-1],), float(prefill), device="cuda")
    view = [bucket[offs[i]:offs[i + 1]].view(shapes[i]) for i in range(len(shapes))]
    w_head = p["conv.weight"].cuda()
    with eng.window(B, T, H, W, True, False, f) as ws:
        eng.forward(ws, data["X"].cuda())
        eng.head_backward(ws, w_head, data["Rp"].cuda(), dw_out=view[2 * L].view(OUT, -1), db_out=view[2 * L + 1], accumulate=accumulate)
        eng.backward(ws, False, zero_state_grads=range(L), dW_out=view[0:2 * L:2], db_out=view[1:2 * L:2], accumulate=accumulate,
                     train_from=f)
    torch.cuda.synchronize()
    return bucket, view, offs


@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_frozen_pass_gives_the_gradients_of_the_unfrozen_pass_and_touches_nothing_below(pkg, data, dtype, f):
    eng = make_engine(data["params"], dtype)              # engine defaults
    _, full, _ = bucket_run(eng, data, 0, False, 0.0)
    bucket, view, offs = bucket_run(eng, data, f, False, SENTINEL)
    names = [f"layers.{l}.conv.{n}" for l in range(L) for n in ("weight", "bias")] + ["conv.weight", "conv.bias"]
    for i, name in enumerate(names):
        if i < 2 * f:
            continue
        check_grad(view[i], full[i], dtype, f"{name} against the f = 0 pass")
        check_grad(view[i], data["grads"][name], dtype, f"{name} against CPU autograd")
    n0 = offs[2 * f]
    assert n0 > 0 and bits(bucket[:n0]) == bits(torch.full((n0,), SENTINEL)), "the frozen layers' bucket regions"
    # accumulate = True: the trained regions receive old + gradient, the frozen ones stay
    start = torch.full((offs[-1],), SENTINEL, device="cuda")
    start[n0:] = torch.from_numpy(np.random.default_rng(3).standard_normal(offs[-1] - n0).astype(np.float32)).cuda()
    acc, _, _ = bucket_run(eng, data, f, True, start)
    assert bits(acc[:n0]) == bits(start[:n0])
    assert bits(acc[n0:]) == bits(start[n0:] + bucket[n0:]), "accumulate: (float)(old + gradient), the stored gradient's own bits"


# =========================================================================== 7. the workspace
@pytest.mark.parametrize("f", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_frozen_workspace_holds_no_stash_below_and_runs_the_same_forward_pass(pkg, data, dtype, f):
    eng = make_engine(data["params"], dtype)
    w, b = data["params"]["conv.weight"].cuda(), data["params"]["conv.bias"].cuda()
    outs = []
    for tf in (0, f):
        with eng.window(B, T, H, W, True, False, tf) as ws:
            assert ws.key == eng.pool_key(B, T, H, W, True, False, tf) and ws.train_from == tf and (ws.key[-1] == tf or not tf)
            for l in range(L):
                held = [ws.gates[l], ws.dG[l], ws.dc[l]]
                assert all(t is None for t in held) if l < tf else all(t is not None for t in held), (tf, l)
                assert (ws.seq.gates[l] is None) == (l < tf) and (ws.seq.dG[l] is None) == (l < tf)
            assert ws.dh[L - 1] is not None                   # what the head pass writes
            eng.forward(ws, data["X"].cuda())
            outs.append([bits(t) for t in ws.h + ws.c] + [bits(eng.head_forward(ws, w, b))])
    assert outs[0] == outs[1]
    full = sum(t.numel() * t.element_size() for ws in eng.pool[(B, T, H, W, True, False)] for t in ws.gates + ws.dG)
    part = sum(t.numel() * t.element_size() for ws in eng.pool[(B, T, H, W, True, False, f)] for t in ws.gates + ws.dG if t is not None)
    print(f"  stash + dG bytes: {full} unfrozen, {part} with train_from = {f}")
    assert part < full


def test_engine_refuses_what_does_not_go_with_frozen_layers(pkg, data):
    from nasa_niswan_amd._lib import NintError
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    eng = make_engine(data["params"], "f32")
    with eng.window(B, T, H, W, True, False, 1) as ws:
        eng.forward(ws, data["X"].cuda())
        eng.set_dstate(ws, L - 1, "h", data["Rh"].cuda())
        with pytest.raises(NintError, match="need_dx"):
            eng.backward(ws, True, zero_state_grads=range(L), train_from=1)
        with pytest.raises(NintError, match="parts"):
            eng.backward(ws, False, zero_state_grads=range(L), train_from=1, parts=1)
        with pytest.raises(NintError, match="no stash"):
            eng.backward(ws, False, zero_state_grads=range(L), train_from=0)
        dWs, dbs, dx = eng.backward(ws, False, zero_state_grads=range(L), train_from=L)      # no library call
        assert dWs == [None] * L and dbs == [None] * L and dx is None
    # a frozen 9x9 layer no longer blocks training the layers above it
    odd = SeqEngine([LayerCfg(4, 8, 9), LayerCfg(8, 8, 3)], "f32", "cuda")
    with pytest.raises(NintError, match="layer 0"):
        odd.acquire(1, 2, 12, 20, True, False)
    odd.release(odd.acquire(1, 2, 12, 20, True, False, 1))


# =========================================================================== 8. the grouped kernels through the C ABI
N8, GROUPS8 = 1000, [(3, 130, 1e-3, 1e-2), (130, 131, 1e-4, 0.0), (131, 900, 3e-4, 0.1)]
B1, B2, EPS = 0.5, 0.999, 1e-8


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def table(rows):
    from nasa_niswan_amd import _lib
    return (_lib.NintOptGroup * len(rows))(*[_lib.NintOptGroup(*r) for r in rows])


def adam_buffers(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(N8) * scale).astype(np.float32)
    p = rng.standard_normal(N8).astype(np.float32)
    m = (rng.standard_normal(N8) * 0.1).astype(np.float32)
    v = (rng.standard_normal(N8) ** 2 * 0.01).astype(np.float32)
    return [torch.from_numpy(a).cuda() for a in (p, g, m, v)]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def test_grouped_adam_against_the_host_model_and_plain_adam(pkg):
    lib = pkg.load_library()
    p, g, m, v = adam_buffers(1)
    before = [host(t) for t in (p, g, m, v)]
    for step in (1, 2):
        before = [host(t) for t in (p, g, m, v)]
        assert lib.nint_adam_flat_groups(P(p), P(g), P(m), P(v), table(GROUPS8), 3, B1, B2, EPS, step, 0.5, None) == 0
        worst = FM.audit([host(t) for t in (p, m, v)], before, GROUPS8, B1, B2, EPS, step, 0.5, what=f"step {step}")
        print(f"  grouped step {step}: worst error / bound {worst:.4f}; outside [3, 900) untouched")
        assert np.array_equal(host(g), before[1])
    # a zero-decay group is nint_adam_flat on its range at its lr, bit for bit
    rows = [(3, 130, 1e-3, 0.0), (130, 131, 1e-4, 0.0), (131, 900, 3e-4, 0.0)]
    p, g, m, v = adam_buffers(2)
    q = [t.clone() for t in (p, m, v)]
    assert lib.nint_adam_flat_groups(P(p), P(g), P(m), P(v), table(rows), 3, B1, B2, EPS, 3, 0.25, None) == 0
    for b, e, lr, _ in rows:
        off = lambda t: C.c_void_p(t.data_ptr() + 4 * b)
        assert lib.nint_adam_flat(off(q[0]), off(g), off(q[1]), off(q[2]), e - b, lr, B1, B2, EPS, 3, 0.25, None) == 0
    for a, c, k in zip((p, m, v), q, "pmv"):
        assert bits(a) == bits(c), k


class Guard:
    def __init__(self, lib):
        from nasa_niswan_amd import _lib
        self.lib = lib
        self.state = torch.zeros(_lib.NINT_OPT_STATE, dtype=torch.float64, device="cuda")
        self.gstate = torch.full((2 * _lib.NINT_MAX_OPT_GROUPS,), -7.0, dtype=torch.float64, device="cuda")
        self.nb = lib.nint_grad_norm_scratch_bytes()
        self.scratch = torch.full((self.nb // 8,), float("nan"), dtype=torch.float64, device="cuda")

    def call(self, p, g, m, v, rows, gs, max_norm, skip=1):
        rc = self.lib.nint_adam_flat_groups_guarded(P(p), P(g), P(m), P(v), table(rows), len(rows), B1, B2, EPS, gs, max_norm, skip,
                                                    P(self.state), P(self.gstate), P(self.scratch), self.nb, None)
        assert rc == 0, rc
        return host(self.state), host(self.gstate)


def test_guarded_grouped_adam_norm_clip_and_skip_run_over_the_range_only(pkg):
    lib = pkg.load_library()
    b0, e0 = GROUPS8[0][0], GROUPS8[-1][1]
    p, g, m, v = adam_buffers(4, scale=3.0)
    g[1] = float("inf")                                   # outside the range: never seen
    g[950] = float("nan")
    before = [host(t) for t in (p, g, m, v)]
    gd = Guard(lib)
    st0 = host(gd.state)
    st, gst = gd.call(p, g, m, v, GROUPS8, 0.5, 1.0)
    # S is nint_grad_norm_flat on the range, bit for bit
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert lib.nint_grad_norm_flat(C.c_void_p(g.data_ptr() + 4 * b0), e0 - b0, 0.5, P(out), P(gd.scratch), gd.nb, None) == 0
    assert host(out)[0] == st[GM.S_] and np.isfinite(st[GM.S_])
    worst = GM.check_state(st, before[1][b0:e0], e0 - b0, 0.5, 1.0, True, GROUPS8[0][2], B1, B2, before=st0)
    assert st[GM.COEF] < 1.0 and st[GM.APPLY] == 1.0 and st[GM.CLIPPED] == 1.0       # a clipped step
    # each group's scalars, f32 values held in doubles; [11] is group 0's step size
    bc1 = 1.0 - B1 ** 1
    for k, (_, _, lr, wd) in enumerate(GROUPS8):
        want = float(np.float32(lr / bc1))
        assert abs(gst[2 * k] - want) <= float(np.spacing(np.float32(want))) and float(np.float32(gst[2 * k])) == gst[2 * k], k
        assert gst[2 * k + 1] == FM.decay_multiplier(lr, wd), k
    assert gst[0] == st[GM.STEP_SIZE] and (gst[6:] == -7.0).all()
    # the clipped step audits with the device's scale
    w2 = FM.audit([host(t) for t in (p, m, v)], before, GROUPS8, B1, B2, EPS, 1, float(st[GM.SCALE]), what="clipped")
    print(f"  guarded grouped step: state worst ratio {worst:.3f}, body worst ratio {w2:.4f}, coef {st[GM.COEF]:.4f}")
    # an inf inside the range: skipped, nothing stored anywhere
    g[500] = float("inf")
    before = [host(t) for t in (p, g, m, v)]
    st, _ = gd.call(p, g, m, v, GROUPS8, 0.5, 1.0)
    assert st[GM.APPLY] == 0.0 and st[GM.SKIPPED] == 1.0 and st[GM.APPLIED] == 1.0
    for t, b4, k in zip((p, m, v), (before[0], before[2], before[3]), "pmv"):
        assert host(t).tobytes() == b4.tobytes(), k


# =========================================================================== 9. FusedTrainer against CPU autograd + torch.optim.AdamW
LR, WD, SCALES = 1e-4, 1e-2, [0.25, 0.5, 1.0]
VARIANTS = {"plain": {}, "segments": dict(bptt_segments=3), "stateful": dict(stateful=True), "sequence_loss": dict(sequence_loss=True),
            "accumulate": dict(accumulate_steps=2), "clip": dict(max_grad_norm=0.05)}


def fit_data(variant):
    """six batches (B, T, C, H, W) with their targets: the trainer's three optimizer steps use three of them, or all six with
    accumulate_steps = 2"""
    rng = np.random.default_rng(77)
    Xs = [torch.from_numpy(rng.standard_normal((B, T, CIN, H, W)).astype(np.float32)) for _ in range(6)]
    shape = (B, T, OUT, HC, WC) if variant == "sequence_loss" else (B, OUT, HC, WC)
    ys = [torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) for _ in range(6)]
    return Xs, ys


def oracle_fit(params, Xs, ys, f, variant, lr=LR, wd=WD, scales=SCALES):
    """the oracle forward, CPU autograd and torch.optim.AdamW (frozen layers: requires_grad False, in no group; biases in
    zero-decay groups): losses of every call and the final parameters"""
    from oracle import convlstm_oracle as O
    leaf = {k: v.clone().requires_grad_(not (k.startswith("layers.") and int(k.split(".")[1]) < f)) for k, v in params.items()}
    groups = []
    for l in list(range(f, L)) + [L]:
        stem = f"layers.{l}.conv." if l < L else "conv."
        glr = lr * (scales[l] if l < L else scales[-1])
        groups += [dict(params=[leaf[stem + "weight"]], lr=glr, weight_decay=wd), dict(params=[leaf[stem + "bias"]], lr=glr, weight_decay=0.0)]
    opt = torch.optim.AdamW(groups, lr=lr, betas=(0.5, 0.999), eps=1e-8, foreach=False)
    k = 2 if variant == "accumulate" else 1
    losses, state = [], None
    for i in range(3 * k):
        kw = {}
        if variant == "stateful" and state is not None:
            kw = dict(h0=[h.detach() for h in state[0]], c0=[c.detach() for c in state[1]])
        if variant == "sequence_loss":
            _, seq = O.convlstm_forward(Xs[i], leaf, return_sequence=True)
            pred = O.crop_pred(seq, HALO, (HC, WC)).reshape(B, T, OUT, HC, WC)
        else:
            out, hs, cs = O.convlstm_forward(Xs[i], leaf, return_states=True, **kw)
            state = (hs, cs)
            pred = O.crop_pred(out, HALO, (HC, WC))
        loss = O.loss_mse_l1(ys[i], pred)
        (loss / k).backward()
        losses.append(float(loss.detach()))
        if (i + 1) % k == 0:
            if variant == "clip":
                norm = torch.nn.utils.clip_grad_norm_([p for p in leaf.values() if p.requires_grad], VARIANTS["clip"]["max_grad_norm"])
                assert float(norm) > VARIANTS["clip"]["max_grad_norm"], "the threshold must clip"
            opt.step()
            opt.zero_grad()
    return losses, {k: v.detach() for k, v in leaf.items()}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("f", [1, 2])
def test_fused_trainer_with_frozen_layers_matches_autograd_and_adamw(pkg, data, f, variant):
    """Tolerances of test_fused_trainer_matches_reference_fit_loop_cfg0 (f32, lr 1e-4, three optimizer steps): loss within
    2e-6, weights max 6.5e-4 / mean 2e-6."""
    from nasa_niswan_amd.trainer import FusedTrainer
    Xs, ys = fit_data(variant)
    losses, final = oracle_fit(data["params"], Xs, ys, f, variant)
    net = pkg.ConvLSTM(CIN, HIDDEN, KS, L, out_channels=OUT, compute_dtype="f32").cuda()
    net.load_state_dict(data["params"])
    tr = FusedTrainer(net, lr=LR, betas=(0.5, 0.999), halo=HALO, freeze_layers=f, weight_decay=WD, layer_lr_scale=SCALES,
                      **VARIANTS[variant])
    n0 = tr.optimizer.n0
    start = tr.flat.data[:n0].clone()
    tr.flat.grad[:n0] = SENTINEL
    for i, want in enumerate(losses):
        loss = float(tr.step(Xs[i].cuda(), ys[i].cuda()))
        print(f"  {variant} f={f} call {i}: loss {loss:.7f} oracle {want:.7f} |diff| {abs(loss - want):.2e}")
        assert abs(loss - want) < 2e-6
    assert n0 == tr.flat.offsets[2 * f] and bits(tr.flat.data[:n0]) == bits(start), "frozen weights"
    assert not tr.optimizer.exp_avg[:n0].any() and not tr.optimizer.exp_avg_sq[:n0].any(), "frozen moments"
    assert bits(tr.flat.grad[:n0]) == bits(torch.full((n0,), SENTINEL)), "frozen gradient regions"
    assert [p.requires_grad for p in net.parameters()] == [False] * (2 * f) + [True] * (2 * (L - f) + 2)
    for k, v in net.state_dict().items():
        d = (v.cpu() - final[k]).abs()
        print(f"  {k}: max |dW| {float(d.max()):.2e}, mean {float(d.mean()):.2e}")
        assert float(d.max()) <= 6.5e-4 and float(d.mean()) <= 2e-6, k
    if variant == "clip":
        assert tr.grad_stats()["clipped"] == 3


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_head_only_fine_tuning_moves_the_head_alone(pkg, data, dtype):
    from nasa_niswan_amd.trainer import FusedTrainer
    Xs, ys = fit_data("plain")
    net = pkg.ConvLSTM(CIN, HIDDEN, KS, L, out_channels=OUT, compute_dtype=dtype).cuda()
    net.load_state_dict(data["params"])
    tr = FusedTrainer(net, lr=1e-2, betas=(0.5, 0.999), halo=HALO, freeze_layers=L, weight_decay=WD)
    n0 = tr.optimizer.n0
    start = tr.flat.data.clone()
    losses = [float(tr.step(Xs[0].cuda(), ys[0].cuda())) for _ in range(3)]
    print(f"  head only ({dtype}): losses {losses}")
    assert losses[0] > losses[1] > losses[2]
    assert n0 == tr.flat.offsets[2 * L] and bits(tr.flat.data[:n0]) == bits(start[:n0])
    assert not torch.equal(tr.flat.data[n0:], start[n0:])


def test_trainer_refuses_overlap_with_frozen_layers(pkg, data):
    from nasa_niswan_amd.trainer import FusedTrainer
    net = pkg.ConvLSTM(CIN, HIDDEN, KS, L, out_channels=OUT).cuda()
    with pytest.raises(ValueError, match="overlap_allreduce"):
        FusedTrainer(net, freeze_layers=1, overlap_allreduce=True)
    with pytest.raises(ValueError, match="freeze_layers"):
        FusedTrainer(net, freeze_layers=L + 1)


# =========================================================================== 10. the autograd path
@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_requires_grad_false_prunes_bptt_and_keeps_the_other_gradients(pkg, data, dtype, f):
    net = pkg.ConvLSTM(CIN, HIDDEN, KS, L, out_channels=OUT, compute_dtype=dtype).cuda()
    net.load_state_dict(data["params"])
    for l in range(f):
        net.layers[l].requires_grad_(False)
    X, Rp = data["X"].cuda(), data["Rp"].cuda()
    (net(X) * Rp).sum().backward()
    eng = net._engine(X.device)
    assert (B, T, H, W, True, False, f) in eng.pool and (B, T, H, W, True, False) not in eng.pool      # BPTT was pruned
    for name, p in net.named_parameters():
        if name.startswith("layers.") and int(name.split(".")[1]) < f:
            assert p.grad is None, name
        else:
            check_grad(p.grad, data["grads"][name], dtype, name)
    # a weight with requires_grad but a frozen bias counts as a trainable layer
    net.zero_grad(set_to_none=True)
    net.layers[0].conv.weight.requires_grad_(True)
    (net(X) * Rp).sum().backward()
    assert (B, T, H, W, True, False) in eng.pool and net.layers[0].conv.bias.grad is None
    check_grad(net.layers[0].conv.weight.grad, data["grads"]["layers.0.conv.weight"], dtype, "layers.0.conv.weight alone")
    net.layers[0].conv.weight.requires_grad_(False)
    # x.requires_grad_() on the same module: nothing is pruned and dx is right
    net.zero_grad(set_to_none=True)
    Xg = X.clone().requires_grad_(True)
    (net(Xg) * Rp).sum().backward()
    check_grad(Xg.grad, data["dX"], dtype, "dL/dx with frozen layers")
    check_grad(net.layers[L - 1].conv.weight.grad, data["grads"][f"layers.{L - 1}.conv.weight"], dtype, "top layer, with dx")
    assert all(net.layers[l].conv.weight.grad is None for l in range(f))


def test_a_tensor_state_of_layer_0_that_requires_grad_keeps_the_whole_pass(pkg, data):
    from oracle import convlstm_oracle as O
    net = pkg.ConvLSTM(CIN, HIDDEN, KS, L, out_channels=OUT, compute_dtype="f32").cuda()
    net.load_state_dict(data["params"])
    net.layers[0].requires_grad_(False)
    rng = np.random.default_rng(9)
    st = [(torch.from_numpy(rng.standard_normal((B, ch, H, W)).astype(np.float32) * 0.5),
           torch.from_numpy(rng.standard_normal((B, ch, H, W)).astype(np.float32) * 0.5)) for ch in HIDDEN]
    h00 = st[0][0].clone().requires_grad_(True)
    leaf = {k: v.clone() for k, v in data["params"].items()}
    (O.convlstm_forward(data["X"], leaf, h0=[h00] + [h for h, _ in st[1:]], c0=[c for _, c in st]) * data["Rp"]).sum().backward()
    dev = [(h.cuda(), c.cuda()) for h, c in st]
    hg = dev[0][0].clone().requires_grad_(True)
    dev[0] = (hg, dev[0][1])
    (net(data["X"].cuda(), dev) * data["Rp"].cuda()).sum().backward()
    assert (B, T, H, W, True, True) in net._engine(hg.device).pool
    check_grad(hg.grad, h00.grad, "f32", "dL/dh0 of layer 0")


# =========================================================================== 11. two ranks on one device
def _ddp_rank(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import nasa_niswan_amd as p
    from nasa_niswan_amd.trainer import FusedTrainer
    from nasa_niswan_amd.utils import shard_indices
    torch.manual_seed(100 + rank)
    net = p.ConvLSTM(6, [16, 8], [3, 3], 2, out_channels=2, compute_dtype="f32").cuda()
    tr = FusedTrainer(net, lr=1e-2, halo=(2, 2), freeze_layers=1, weight_decay=1e-2)
    sizes = []
    real = dist.all_reduce

    def spy(t, *a, **kw):
        sizes.append((t.numel(), t.data_ptr() - tr.flat.grad.data_ptr()))
        return real(t, *a, **kw)
    tr.dist = type("D", (), dict(all_reduce=staticmethod(spy), ReduceOp=dist.ReduceOp))
    g = torch.Generator().manual_seed(7)
    X = torch.randn(4, 3, 6, 20, 28, generator=g)
    y = torch.randn(4, 2, 16, 24, generator=g)
    losses = []
    for step in range(3):
        idx = shard_indices(4, step, rank, world, 2, shuffle=False)[0]
        losses.append(float(tr.step(X[idx].cuda(), y[idx].cuda())))
    torch.cuda.synchronize()
    torch.save({"w": tr.flat.data.detach().cpu(), "losses": losses, "exchanged": sizes, "n0": tr.optimizer.n0, "n": tr.flat.numel},
               f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_a_frozen_layer_match_the_global_batch_and_exchange_the_tail(pkg, tmp_path):
    import socket
    import torch.multiprocessing as mp
    from nasa_niswan_amd.trainer import FusedTrainer
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "ddp")
    mp.spawn(_ddp_rank, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert torch.equal(r0["w"], r1["w"])
    n0, n = r0["n0"], r0["n"]
    assert n0 > 0 and r0["exchanged"] == [(n - n0, 4 * n0)] * 3, "the exchanged tensor is the trained tail of the bucket"
    torch.manual_seed(100)
    net = pkg.ConvLSTM(6, [16, 8], [3, 3], 2, out_channels=2, compute_dtype="f32").cuda()
    tr = FusedTrainer(net, lr=1e-2, halo=(2, 2), freeze_layers=1, weight_decay=1e-2)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(4, 3, 6, 20, 28, generator=g)
    y = torch.randn(4, 2, 16, 24, generator=g)
    losses = [float(tr.step(X.cuda(), y.cuda())) for _ in range(3)]
    w = tr.flat.data.detach().cpu()
    err = float((w - r0["w"]).abs().max() / w.abs().max())
    print(f"  two ranks, layer 0 frozen, against the global batch: weights rel max err {err:.2e}")
    assert err < 2e-5
    for a, b, c in zip(losses, r0["losses"], r1["losses"]):
        assert abs(a - (b + c) / 2) < 1e-5 * abs(a)
