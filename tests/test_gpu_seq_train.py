"""GPU tests of training on the per-step head outputs (ConvLSTM(..., return_sequence=True) with gradients, and
FusedTrainer(sequence_loss=True)): the sequence head kernels at the C ABI, the per-step gradient's way into BPTT
(nint_seq.dh_seq), autograd parity with the CPU oracle, the fused sequence step and train.py --sequence-loss.

Tolerances are the project's standing ones (tests/test_gpu_parity.py header):
  f32 : outputs rtol 1e-4 / atol 1e-5; gradients max-abs error <= 1e-3 * max|grad| + 1e-6
  bf16: rel-L2 <= 2e-2 against the f32 oracle
The oracle is oracle.convlstm_oracle.convlstm_forward(..., return_sequence=True) under CPU autograd.

Shapes: S1 = ConvLSTM(4, [8], [3], 1) (the top layer is layer 0, classic); S3 = ConvLSTM(5, [64, 32, 16], [5, 3, 3], 3) (bf16:
fused top layer riding with the bottom pointwise pass under wave 4 / 5; f32: classic top layer); S3o = ConvLSTM(5, [16, 8, 8],
[3, 3, 3], 3, out_channels=3).  B = 2, T = 4 (a first, two middle and a time-0 BPTT step), grid 12 x 20 (a 4-row strip and a
partial column tile)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, H, W = 2, 4, 12, 20
SHAPES = {"S1": (4, [8], [3], 1), "S3": (5, [64, 32, 16], [5, 3, 3], 1), "S3o": (5, [16, 8, 8], [3, 3, 3], 3)}
SEEDS = {"S1": 21, "S3": 22, "S3o": 23}


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


@pytest.fixture
def knobs():
    """engine.FORCE_WAVE / FUSE_BWD, restored whatever the test does"""
    from nasa_niswan_amd import engine
    old = engine.FORCE_WAVE, engine.FUSE_BWD
    yield engine
    engine.FORCE_WAVE, engine.FUSE_BWD = old


def check_out(a, b, what):
    a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
    print(f"  {what}: max abs err {float(np.abs(a - b).max()):.3e} (ref max {float(np.abs(b).max()):.3e})")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=what)


def check_grad(a, b, what, dtype="f32"):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert torch.isfinite(a).all(), what
    if dtype == "f32":
        e, m = float((a - b).abs().max()), float(b.abs().max())
        print(f"  {what}: max abs err {e:.3e} (ref max {m:.3e})")
        assert e <= 1e-3 * m + 1e-6, f"{what}: {e} vs tolerance {1e-3 * m + 1e-6}"
    else:
        r = float((a - b).norm() / (b.norm() + 1e-30))
        print(f"  {what}: rel-L2 {r:.3e}")
        assert r <= 2e-2, f"{what}: rel-L2 {r} > 2e-2"


# ------------------------------------------------------------------ the oracle side, computed once per case
@functools.lru_cache(maxsize=None)
def case_data(shape):
    from oracle import convlstm_oracle as O
    cin, hidden, ks, out = SHAPES[shape]
    seed = SEEDS[shape]
    params = O.synth_params(cin, hidden, ks, len(hidden), out_channels=out, seed=seed)
    rng = np.random.default_rng(seed)
    X = torch.from_numpy(rng.standard_normal((B, T, cin, H, W)).astype(np.float32))
    Rp = torch.from_numpy(rng.standard_normal((B, out, H, W)).astype(np.float32))
    Rs = torch.from_numpy(rng.standard_normal((B, T * out, H, W)).astype(np.float32))
    return params, X, Rp, Rs


@functools.lru_cache(maxsize=None)
def oracle_grads(shape, mode):
    """mode: 'both' = (pred*Rp).sum() + (seq*Rs).sum(), 'seq' = the second term alone, 'pred' = the first alone"""
    from oracle import convlstm_oracle as O
    params, X, Rp, Rs = case_data(shape)
    leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    Xo = X.clone().requires_grad_(True)
    pred, seq = O.convlstm_forward(Xo, leaf, return_sequence=True)
    loss = (pred * Rp).sum() * (mode != "seq") + (seq * Rs).sum() * (mode != "pred")
    loss.backward()
    g = {k: v.grad.detach() for k, v in leaf.items()}
    g["X"] = Xo.grad.detach()
    return pred.detach(), seq.detach(), g


def gpu_grads(pkg, shape, dtype, mode, return_sequence=True):
    params, X, Rp, Rs = case_data(shape)
    cin, hidden, ks, out = SHAPES[shape]
    net = pkg.ConvLSTM(cin, hidden, ks, len(hidden), out_channels=out, return_sequence=return_sequence, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    Xg = X.cuda().requires_grad_(True)
    if return_sequence:
        pred, seq = net(Xg)
    else:
        pred, seq = net(Xg), None
    loss = 0
    if mode != "seq":
        loss = loss + (pred * Rp.cuda()).sum()
    if mode != "pred":
        loss = loss + (seq * Rs.cuda()).sum()
    loss.backward()
    g = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    g["X"] = Xg.grad.detach().cpu()
    return pred.detach().cpu(), None if seq is None else seq.detach().cpu(), g


# ------------------------------------------------------------------ 1 / 2: the head kernels at the C ABI
class HeadCase:
    """A top-layer h slab of (T+1)*B random images (slot 0 = the initial state) in the storage type, head weights, and the stored
    values read back (exact: what the kernels see)."""

    def __init__(self, pkg, Ch, O, dtype, Bn=2, Tn=3, Hn=12, Wn=20, seed=0):
        from nasa_niswan_amd import _lib
        self.lib = lib = pkg.load_library()
        self.dt = _lib.NINT_BF16 if dtype == "bf16" else _lib.NINT_F32
        self.es = 2 if dtype == "bf16" else 4
        self.B, self.T, self.H, self.W, self.Ch, self.O = Bn, Tn, Hn, Wn, Ch, O
        kc = lib.nint_kc(self.dt)
        self.Chp = (Ch + kc - 1) // kc * kc
        self.g = _lib.NintGeom()
        assert lib.nint_geom_make(C.byref(self.g), Hn, Wn, 1) == 0
        gen = torch.Generator().manual_seed(1000 * Ch + 10 * O + seed)
        h = torch.randn(Bn, Tn + 1, Ch, Hn, Wn, generator=gen).cuda()
        self.w = (torch.randn(O, Ch, generator=gen) / Ch ** 0.5).cuda()
        self.b = torch.randn(O, generator=gen).cuda()
        self.dseq = torch.randn(Bn, Tn * O, Hn, Wn, generator=gen).cuda()
        self.dlast = torch.randn(Bn, O, Hn, Wn, generator=gen).cuda()
        self.slab = torch.zeros((Tn + 1) * Bn * self.g.Hh * self.g.Wh * self.Chp * self.es, dtype=torch.uint8, device="cuda")
        self.ck(lib.nint_pack_btchw(self.p(h), self.p(self.slab), Bn, Tn + 1, Ch, self.Chp, C.byref(self.g), self.dt, None))
        stored = torch.empty((Tn + 1) * Bn, Ch, Hn, Wn, device="cuda")
        self.ck(lib.nint_unpack_halo(self.p(self.slab), self.p(stored), 0, (Tn + 1) * Bn, Ch, self.Chp, C.byref(self.g), self.dt, None))
        self.h = stored.view(Tn + 1, Bn, Ch, Hn, Wn)[1:].double().cpu()          # [t][b]: h_t = slot t + 1
        self.scratch = torch.empty(256 * O * (Ch + 1), device="cuda")

    @staticmethod
    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    @staticmethod
    def ck(rc):
        assert rc == 0, rc

    def fwd_seq(self):
        seq = torch.full((self.B, self.T * self.O, self.H, self.W), float("nan"), device="cuda")
        self.ck(self.lib.nint_head_fwd_seq(self.p(self.slab), self.B, self.T, self.Ch, self.Chp, self.O, self.p(self.w), self.p(self.b),
                                           self.p(seq), C.byref(self.g), self.dt, None))
        return seq

    def fwd_steps(self):
        outs = []
        for t in range(self.T):
            pred = torch.empty(self.B, self.O, self.H, self.W, device="cuda")
            self.ck(self.lib.nint_head_fwd(self.p(self.slab), (t + 1) * self.B, self.B, self.Ch, self.Chp, self.O, self.p(self.w),
                                           self.p(self.b), self.p(pred), C.byref(self.g), self.dt, None))
            outs.append(pred)
        return torch.cat(outs, dim=1)

    def bwd_seq(self, dseq, dlast, scratch=True):
        n = self.T * self.B * self.H * self.W * self.Chp
        dh = torch.full((n * self.es,), 0xAB, dtype=torch.uint8, device="cuda")
        dw = torch.full((self.O, self.Ch), float("nan"), device="cuda")
        db = torch.full((self.O,), float("nan"), device="cuda")
        self.ck(self.lib.nint_head_bwd_seq(self.p(self.slab), self.B, self.T, self.Ch, self.Chp, self.O, self.p(self.w), self.p(dseq),
                                           self.p(dlast), self.p(dh), self.p(dw), self.p(db), C.byref(self.g), self.dt,
                                           self.p(self.scratch) if scratch else None, self.scratch.numel() * 4 if scratch else 0, None))
        return dh, dw, db

    def dh_values(self, dh):
        """(T, B, Chp, H, W) f32 of a compact ET slab, padding channels included"""
        raw = dh.view(torch.bfloat16 if self.es == 2 else torch.float32).view(self.T, self.B, self.H, self.W, self.Chp)
        return raw.float().permute(0, 1, 4, 2, 3).cpu()


HEAD_GRID = [(Ch, O) for Ch in (8, 40, 72, 136) for O in (1, 3)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Ch,O", HEAD_GRID + [(72, 200), (136, 200)])
def test_head_fwd_seq_equals_the_per_step_launches_bit_for_bit(pkg, Ch, O, dtype):
    """Ch 8 / 40 / 72 / 136: the 32-, 64-, 128-channel register bodies and the generic wide body (f32 pads 40 to 48 and 72 to 80,
    bf16 to 64 and 96; 136 pads beyond 128 in both).  200 outputs at 72 channels: a weight image [O][128] of 100 KiB, the staged
    body with the dynamic-LDS opt-in; at 136 channels the wide body at a large O."""
    hc = HeadCase(pkg, Ch, O, dtype)
    seq, ref = hc.fwd_seq(), hc.fwd_steps()
    assert torch.isfinite(seq).all() and torch.equal(seq, ref)
    want = torch.einsum("oc,tbcyx->btoyx", hc.w.double().cpu(), hc.h) + hc.b.double().cpu().view(1, 1, O, 1, 1)
    check_out(seq.cpu().view(hc.B, hc.T, O, hc.H, hc.W), want.float(), f"seq Ch={Ch} O={O} {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Ch,O", HEAD_GRID + [(40, 20)])
def test_head_bwd_seq_against_f64_sums_of_the_stored_slab(pkg, Ch, O, dtype):
    """dh_seq, dw, db of nint_head_bwd_seq against f64 einsums of the slab as stored, for both cotangents, dpred_last alone and
    dseq alone; with the caller's scratch (the two-stage tiled reduction; 20 outputs x 41: the register-tiled one) and without
    (one workgroup per output).  dw / db: f32 sums of exact inputs, the standing gradient tolerance in both storage types.
    dh_seq: the same in f32; a bf16 slab rounds each value once (half an ulp, 2^-9 relative, on top of the f32 error), so there
    the bound is 2^-8 * max|dh| elementwise and the standing rel-L2 2e-2.  Padding channels are zero; two runs are bit-equal."""
    hc = HeadCase(pkg, Ch, O, dtype)
    w64 = hc.w.double().cpu()
    for name, dseq, dlast in (("both", hc.dseq, hc.dlast), ("last-only", None, hc.dlast), ("seq-only", hc.dseq, None)):
        d = torch.zeros(hc.B, hc.T, O, hc.H, hc.W, dtype=torch.float64)
        if dseq is not None:
            d += dseq.double().cpu().view(hc.B, hc.T, O, hc.H, hc.W)
        if dlast is not None:
            d[:, hc.T - 1] += dlast.double().cpu()
        want_dh = torch.einsum("oc,btoyx->tbcyx", w64, d)
        want_dw = torch.einsum("btoyx,tbcyx->oc", d, hc.h)
        want_db = d.sum(dim=(0, 1, 3, 4))
        for scratch in (True, False):
            dh, dw, db = hc.bwd_seq(dseq, dlast, scratch)
            dh2, dw2, db2 = hc.bwd_seq(dseq, dlast, scratch)
            assert torch.equal(dh, dh2) and torch.equal(dw, dw2) and torch.equal(db, db2), (name, scratch)
            vals = hc.dh_values(dh)
            assert float(vals[:, :, Ch:].abs().max()) == 0.0 if hc.Chp > Ch else True
            what = f"{name} scratch={scratch} Ch={Ch} O={O} {dtype}"
            if dtype == "f32":
                check_grad(vals[:, :, :Ch], want_dh, "dh_seq " + what)
            else:
                e, m = float((vals[:, :, :Ch].double() - want_dh).abs().max()), float(want_dh.abs().max())
                print(f"  dh_seq {what}: max abs err {e:.3e} (ref max {m:.3e})")
                assert e <= 2.0 ** -8 * m + 1e-6
                check_grad(vals[:, :, :Ch], want_dh, "dh_seq " + what, "bf16")
            check_grad(dw, want_dw, "dw " + what)
            check_grad(db, want_db, "db " + what)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ["S1", "S3", "S3o"])
def test_models_last_sequence_block_is_pred(pkg, shape, dtype):
    """seq[:, (T-1)*O:] equals pred bit for bit, in eval and with gradients on; f32 against the oracle to the output tolerance"""
    params, X, _, _ = case_data(shape)
    cin, hidden, ks, out = SHAPES[shape]
    net = pkg.ConvLSTM(cin, hidden, ks, len(hidden), out_channels=out, return_sequence=True, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    with torch.no_grad():
        pred0, seq0 = net(X.cuda())
    pred1, seq1 = net(X.cuda())
    assert seq1.requires_grad and pred1.requires_grad
    assert seq0.shape == (B, T * out, H, W) and torch.equal(seq0[:, (T - 1) * out:], pred0)
    assert torch.equal(seq1, seq0) and torch.equal(pred1, pred0)
    opred, oseq, _ = oracle_grads(shape, "both")
    if dtype == "f32":
        check_out(seq0, oseq, f"seq {shape}")
    else:
        check_grad(seq0, oseq, f"seq {shape}", "bf16")


# ------------------------------------------------------------------ 3: bit identity with the many-to-one path
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fuse", [0, 1, 2])
@pytest.mark.parametrize("wave", [0, 1, 4, 5])
@pytest.mark.parametrize("shape", ["S1", "S3"])
def test_block_t_minus_1_alone_is_the_many_to_one_backward_bit_for_bit(pkg, knobs, shape, wave, fuse, dtype):
    """Today's backward with the head gradient in dh[L-1], then the new one on the same stash with dh_seq zero except block
    T-1, which holds those same bytes, and dh[L-1] filled with NaN (it must not be read).  Adding zero is exact, so every dW,
    db and dx is equal: a difference is a misplaced addend."""
    knobs.FORCE_WAVE, knobs.FUSE_BWD = wave, fuse
    params, X, Rp, _ = case_data(shape)
    cin, hidden, ks, out = SHAPES[shape]
    L = len(hidden)
    net = pkg.ConvLSTM(cin, hidden, ks, L, out_channels=out, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    eng = net._engine(torch.device("cuda", 0))
    ws = eng.acquire(B, T, H, W, True, False)
    assert ws.seq.fuse_bwd == fuse and ws._dh_seq is None
    eng.pack_weights([c.conv.weight for c in net.layers], [c.conv.bias for c in net.layers])
    eng.forward(ws, X.cuda())
    assert ws.seq.wave == (wave if L > 1 else 0)
    eng.head_backward(ws, net.conv.weight, Rp.cuda())
    head = ws.dh[-1].clone()
    dWa, dba, dxa = eng.backward(ws, True, zero_state_grads=range(L))
    assert ws._dh_seq is None                                   # the many-to-one path allocates nothing new
    slab = ws.dh_seq_slab(eng)
    slab.zero_()
    assert slab.numel() == T * head.numel()
    slab[(T - 1) * head.numel():] = head
    ws.dh[-1].fill_(0xFF)
    dWb, dbb, dxb = eng.backward(ws, True, zero_state_grads=range(L), seq_grads=True)
    assert ws.seq.dh_seq is None                                # cleared after the call
    eng.release(ws)
    assert torch.isfinite(dxa).all() and torch.equal(dxa, dxb)
    for l in range(L):
        assert torch.isfinite(dWa[l]).all() and torch.equal(dWa[l], dWb[l]), l
        assert torch.equal(dba[l], dbb[l]), l


# ------------------------------------------------------------------ 4: autograd parity
def _parity(pkg, shape, dtype, mode):
    pred, seq, g = gpu_grads(pkg, shape, dtype, mode)
    opred, oseq, og = oracle_grads(shape, mode)
    assert set(g) == set(og)
    for k in sorted(g):
        check_grad(g[k], og[k], f"{shape} {dtype} {mode} d{k}", dtype)
    return g


@pytest.mark.parametrize("mode", ["both", "seq", "pred"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ["S1", "S3", "S3o"])
def test_autograd_through_seq_matches_the_oracle(pkg, shape, dtype, mode):
    """loss = (pred*Rp).sum() + (seq*Rs).sum() with seeded random Rp, Rs (every time block carries its own cotangent), the
    second term alone (pred unused: its cotangent is absent, not zeros) and the first alone with return_sequence=True, which
    must also equal the return_sequence=False gradients to the same tolerance."""
    g = _parity(pkg, shape, dtype, mode)
    if mode == "pred":
        _, _, g0 = gpu_grads(pkg, shape, dtype, "pred", return_sequence=False)
        for k in sorted(g):
            check_grad(g[k], g0[k], f"{shape} {dtype} pred-only against return_sequence=False d{k}", dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fuse", [0, 1, 2])
@pytest.mark.parametrize("wave", [0, 1, 4, 5])
def test_autograd_through_seq_under_every_schedule(pkg, knobs, wave, fuse, dtype):
    knobs.FORCE_WAVE, knobs.FUSE_BWD = wave, fuse
    _parity(pkg, "S3", dtype, "both")


def test_unused_outputs_give_no_gradient_and_release_the_workspace(pkg):
    params, X, _, _ = case_data("S1")
    net = pkg.ConvLSTM(4, [8], [3], 1, return_sequence=True).cuda()
    net.load_state_dict(params)
    eng = net._engine(torch.device("cuda", 0))
    for _ in range(3):
        pred, seq = net(X.cuda())
        (seq * seq).mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    assert sum(len(v) for v in eng.pool.values()) == 1 and not any(ws.in_use for v in eng.pool.values() for ws in v)


# ------------------------------------------------------------------ 5: the fused sequence step
HALO, CROP = (1, 2), (10, 16)
LR, BETAS = 1e-4, (0.5, 0.999)


@functools.lru_cache(maxsize=None)
def trainer_targets(shape):
    out = SHAPES[shape][3]
    rng = np.random.default_rng(SEEDS[shape] + 500)
    shp = (B, T) + ((out,) if out > 1 else ()) + CROP
    return torch.from_numpy(rng.standard_normal(shp).astype(np.float32))


@functools.lru_cache(maxsize=None)
def oracle_seq_steps(shape, nsteps=3):
    """The oracle's train_step recipe (train.py:96-110) with the sequence loss: loss_mse_l1(y_seq, crop(seq)), CPU autograd, the
    numpy Adam.  Returns per step: loss, gradients, parameters after the step, and the cropped seq before it."""
    from oracle import convlstm_oracle as O
    params, X, _, _ = case_data(shape)
    y = trainer_targets(shape)
    yv = y.reshape(B, -1, *CROP)
    p = params
    st = {"m": {k: torch.zeros_like(v) for k, v in p.items()}, "v": {k: torch.zeros_like(v) for k, v in p.items()}}
    out = []
    for step in range(1, nsteps + 1):
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
        _, seq = O.convlstm_forward(X, leaf, return_sequence=True)
        sc = O.crop_pred(seq, HALO, CROP)
        loss = O.loss_mse_l1(yv, sc)
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in leaf.items()}
        newp, m, v = {}, {}, {}
        for k in p:
            a, b_, c = O.adam_step_numpy(p[k].numpy(), grads[k].numpy(), st["m"][k].numpy(), st["v"][k].numpy(), step, LR, BETAS)
            newp[k], m[k], v[k] = torch.from_numpy(a), torch.from_numpy(b_), torch.from_numpy(c)
        p, st = newp, {"m": m, "v": v}
        out.append(dict(loss=float(loss.detach()), grads=grads, params=p, seq_crop=sc.detach()))
    return out


def _trainer(pkg, shape, dtype, fallback):
    from nasa_niswan_amd.trainer import FusedTrainer
    params, X, _, _ = case_data(shape)
    cin, hidden, ks, out = SHAPES[shape]
    net = pkg.ConvLSTM(cin, hidden, ks, len(hidden), out_channels=out, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, sequence_loss=True)
    eng = net._engine(torch.device("cuda", 0))
    calls = []
    real = eng.head_loss_seq_fused

    def spy(*a, **k):
        if fallback:
            calls.append(False)
            return False
        calls.append(real(*a, **k))
        return calls[-1]
    eng.head_loss_seq_fused = spy
    return net, tr, calls


@pytest.mark.parametrize("fallback", [False, True], ids=["fused", "three-launch"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ["S1", "S3", "S3o"])
def test_fused_sequence_step_matches_the_oracle_fit_loop(pkg, shape, dtype, fallback):
    """Loss, the gradients in the bucket and the parameters after 1 and 3 Adam steps (lr 1e-4, betas (0.5, 0.999)), through the
    fused head / loss pass and through the three-launch fallback.  Loss: the output tolerance (f32) / 2e-2 relative (bf16).
    Parameters: Adam's first steps move a weight by about lr * sign(g), so a near-zero gradient whose sign differs in the last
    bit moves it by 2 * lr per step whatever the storage type: max |dp| <= k * 2.2 * lr after k steps (tests/test_gpu_train.py
    uses the same 6.5e-4 for k = 3 at this lr).  Mean |dp|: f32 the standing 2e-6 of that test; bf16: with a rel-L2 gradient
    error eps = 2e-2 about 0.8 * eps of roughly normal gradients sit below the error and may flip (2 * lr each) and the rest
    moves by about eps * lr: 2.6 * eps * lr per step, bounded here by 0.1 * lr * k."""
    params, X, _, _ = case_data(shape)
    y = trainer_targets(shape)
    want = oracle_seq_steps(shape)
    net, tr, calls = _trainer(pkg, shape, dtype, fallback)
    Xd, yd = X.cuda(), y.cuda()
    names = [k for k, _ in net.named_parameters()]
    for step in (1, 2, 3):
        loss = float(tr.step(Xd, yd))
        o = want[step - 1]
        print(f"  {shape} {dtype} step {step}: loss {loss:.7f} oracle {o['loss']:.7f}")
        if dtype == "f32":
            assert abs(loss - o["loss"]) <= 1e-4 * abs(o["loss"]) + 1e-5
        else:
            assert abs(loss - o["loss"]) <= 2e-2 * abs(o["loss"])
        if step == 1:
            for i, k in enumerate(names):
                check_grad(tr.flat.grad_view(i).view(o["grads"][k].shape), o["grads"][k], f"{shape} {dtype} bucket d{k}", dtype)
        if step in (1, 3):
            for k, v in net.state_dict().items():
                d = (v.cpu() - o["params"][k]).abs()
                print(f"    after {step}: {k}: max |dp| {float(d.max()):.2e}, mean {float(d.mean()):.2e}")
                assert float(d.max()) <= step * 2.2 * LR, (k, step)
                assert float(d.mean()) <= (2e-6 if dtype == "f32" else 0.1 * LR * step), (k, step)
    assert calls == [not fallback] * 3                        # the path the case is about did run
    if dtype == "f32":
        # the trainer's accumulators: mean over the three calls of the loss and of r2_score(y, cropped seq)
        from oracle import convlstm_oracle as O
        loss_e, r2_e = tr.epoch_stats()
        yv = y.reshape(B, -1, *CROP).numpy()
        want_r2 = np.mean([O.r2_score_np(yv, o["seq_crop"].numpy()) for o in want])
        want_loss = np.mean([o["loss"] for o in want])
        print(f"  epoch stats: loss {loss_e:.7f} (oracle {want_loss:.7f}), R2 {r2_e:.7f} (oracle {want_r2:.7f})")
        assert abs(loss_e - want_loss) <= 1e-4 * abs(want_loss) + 1e-5 and abs(r2_e - want_r2) <= 1e-4 * abs(want_r2) + 1e-5


@pytest.mark.parametrize("shape", ["S1", "S3o"])
def test_evaluate_with_sequence_loss_accumulates_the_oracle_statistics(pkg, shape):
    """evaluate(): the loss over every step and R2 of the cropped sequence, one call = one batch of the statistics"""
    from oracle import convlstm_oracle as O
    params, X, _, _ = case_data(shape)
    y = trainer_targets(shape)
    o = oracle_seq_steps(shape)[0]
    net, tr, _ = _trainer(pkg, shape, "f32", False)
    seq = tr.evaluate(X.cuda(), y.cuda())
    assert seq.shape == (B, T * SHAPES[shape][3], H, W)
    check_out(seq[:, :, HALO[0]:HALO[0] + CROP[0], HALO[1]:HALO[1] + CROP[1]], o["seq_crop"], "evaluate seq")
    loss_e, r2_e = tr.epoch_stats()
    want_r2 = O.r2_score_np(y.reshape(B, -1, *CROP).numpy(), o["seq_crop"].numpy())
    assert abs(loss_e - o["loss"]) <= 1e-4 * abs(o["loss"]) + 1e-5 and abs(r2_e - want_r2) <= 1e-4 * abs(want_r2) + 1e-5
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), params[k]), k              # no update


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_backward_in_two_parts_with_a_per_step_gradient_is_bit_identical(pkg, dtype):
    """bwd_parts = 1 then 2 (the data-parallel exchange in two pieces) with nint_seq.dh_seq set in both calls: part 2 is layer
    0's weight gradient only, so every gradient equals the one-call backward's bit for bit."""
    params, X, Rp, Rs = case_data("S3")
    cin, hidden, ks, out = SHAPES["S3"]
    L = len(hidden)
    net = pkg.ConvLSTM(cin, hidden, ks, L, compute_dtype=dtype).cuda()
    net.load_state_dict(params)
    eng = net._engine(torch.device("cuda", 0))
    ws = eng.acquire(B, T, H, W, True, False)
    eng.pack_weights([c.conv.weight for c in net.layers], [c.conv.bias for c in net.layers])
    eng.forward(ws, X.cuda())
    eng.head_backward_seq(ws, net.conv.weight, Rs.cuda(), Rp.cuda())
    dW1, db1, _ = eng.backward(ws, False, zero_state_grads=range(L), seq_grads=True)
    dW2 = [torch.full_like(t, float("nan")) for t in dW1]
    db2 = [torch.full_like(t, float("nan")) for t in db1]
    eng.backward(ws, False, zero_state_grads=range(L), dW_out=dW2, db_out=db2, parts=1, seq_grads=True)
    assert torch.isnan(dW2[0]).all() and torch.isfinite(dW2[1]).all()
    eng.backward(ws, False, zero_state_grads=range(L), dW_out=dW2, db_out=db2, parts=2, seq_grads=True)
    eng.release(ws)
    for l in range(L):
        assert torch.isfinite(dW1[l]).all() and torch.equal(dW1[l], dW2[l]) and torch.equal(db1[l], db2[l]), l


# ------------------------------------------------------------------ 6: data path and train.py
def test_device_batch_sequence_targets_equal_the_z_scored_host_windows(pkg):
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    for levels in (1, 2):
        kw = dict(padding=(14, 22), in_channels=3 * levels + 2, sequence_length=4, levels=levels, n_steps=40, grid=(10, 16),
                  device="cuda", seed=7)
        ds = SyntheticE33OMA_CRNN("train", sequence_targets=True, **kw)
        ds0 = SyntheticE33OMA_CRNN("train", **kw)
        idx = [0, 5, len(ds) - 1]
        X, y = ds.device_batch(idx)
        X0, y0 = ds0.device_batch(idx)
        sb, y2 = ds.slab_batch(idx)
        assert y.shape == ((3, 4, 10, 16) if levels == 1 else (3, 4, 2, 10, 16)) and y.is_contiguous()
        assert torch.equal(X, X0) and torch.equal(y2, y) and torch.equal(y[:, -1], y0)
        for b, i in enumerate(idx):
            _, yw = ds.window(i)
            ref = (yw - ds.y_mean) / ds.y_std
            np.testing.assert_allclose(y[b].cpu().numpy(), ref[:, 0] if levels == 1 else ref, rtol=1e-6, atol=1e-6)


def test_train_py_sequence_loss_end_to_end(pkg, tmp_path):
    """train.py --sequence-loss on the BASELINE configs[0] command line, two epochs in a child
    process: exit 0, finite losses, the usual artefacts."""
    snap = tmp_path / "snap"
    argv = [sys.executable, os.path.join(ROOT, "nasa-niswan_amd", "train.py"), "--in-channels", "4", "--hidden-channels", "8",
            "--kernel-size", "3", "--num-layers", "1", "--sequence-length", "4", "--input-size", "32", "32", "--grid", "32", "32",
            "--batch-size", "2", "--num-epochs", "2", "--synthetic-steps", "24", "--sequence-loss", "--snapshot-dir", str(snap)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Epoch: ")]
    assert len(lines) == 2 and all("Loss:" in ln and "R2T:" in ln and "R2V:" in ln for ln in lines), out.stdout
    with open(snap / "logger.npy", "rb") as f:
        a, b_, c = np.load(f), np.load(f), np.load(f)
    assert a.shape == b_.shape == c.shape == (2,) and np.isfinite(a).all() and np.isfinite(b_).all() and np.isfinite(c).all()
    cfg = json.load(open(snap / "configurations.json"))
    assert cfg["sequence_loss"] is True and cfg["sequence_length"] == 4
