#!/usr/bin/env python3
"""The ensemble training loss and step against their alternatives, on the closed-loop bench stack: 20 feedback
channels, 100 x 144 cyclic, T = 12, bf16, B = 8 lanes.

    python tools/ensemble_train_bench.py [--iters 10] [--rounds 3]

  (a)  nint_ens_loss alone over the (lanes, T, O, H, W) head output, every step listed, at 4 samples x 2 members and 1 sample x 8
       members: time and bytes per second (the members read + the gradients written, 2 * T * B * O * H * W f32)
  (b)  nint_loss_crop_spec over the same T*B images: the same prediction and gradient bytes
  (c)  nint_ens_accum on the same members (reads only)
  (d)  the torch expression of the same loss and gradient (autograd through abs of the pairwise differences): time, peak memory
  (e)  FusedTrainer.step: the ensemble step (sequence loss, feedback noise) against the deterministic roll-out step at the same
       lane count, alternating, --rounds rounds; and the head_forward_seq pass and the fused head / loss pass alone

Every variant is warmed up, then timed with device events over --iters passes."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nasa_niswan_amd as pkg  # noqa: E402
from nasa_niswan_amd import _lib  # noqa: E402
from nasa_niswan_amd.loss import EnsembleLoss, LossSpec, crop_loss_launch  # noqa: E402
from nasa_niswan_amd.trainer import FusedTrainer  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def loss_rows(args, B, T, O, H, W):
    lib = pkg.load_library()
    img = O * H * W
    seq = torch.randn(B, T, O, H, W, device="cuda")
    slab = torch.empty(T * B, O, H, W, device="cuda")
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    ens = torch.zeros(4, dtype=torch.float64, device="cuda")
    loss = torch.zeros(_lib.NINT_LOSS_SPEC_SCRATCH_FLOATS, device="cuda")
    nbytes = 2 * T * B * img * 4
    for N, M in ((4, 2), (1, 8)):
        ns = N * T
        y = torch.randn(ns, O, H, W, device="cuda")
        pairs = [(n, t) for n in range(N) for t in range(T)]
        poff = (C.c_int64 * ns)(*[((n * M) * T + t) * img for n, t in pairs])
        doff = (C.c_int64 * ns)(*[(t * B + n * M) * img for n, t in pairs])
        nb = lib.nint_ens_loss_scratch_bytes(ns, M, O, H, W)
        scratch = torch.empty(nb // 8, dtype=torch.float64, device="cuda")
        sp = _lib.NintEnsLossSpec()
        sp.alpha, sp.cnt, sp.ow, sp.ow_row, sp.nrows = 0.95, float(ns) * O * H * W, None, None, 0

        def run():
            rc = lib.nint_ens_loss(P(seq), poff, T * img, P(slab), doff, img, M, P(y), None, 0.0, C.byref(sp), P(loss), P(stats), P(ens),
                                   P(scratch), nb, ns, O, H, W, 0, 0, H, W, _lib.stream_ptr())
            assert rc == 0, rc
        ms = timed(run, args.iters)
        print(f"(a) nint_ens_loss    {N} samples x {M} members x {T} steps: {ms:8.3f} ms  {nbytes / 1e9:.3f} GB moved  {nbytes / ms / 1e9:.3f} TB/s"
              f"  (+ {ns * img * 4 / 1e9:.3f} GB of targets)")

        pix = torch.zeros(1, _lib.NINT_ENS_PIX, O, H, W, dtype=torch.float64, device="cuda")
        sample = torch.empty(ns, O, _lib.NINT_ENS_SAMPLE, dtype=torch.float64, device="cuda")
        hist = torch.zeros(1, O, M + 2, dtype=torch.int64, device="cuda")
        nb2 = lib.nint_ens_scratch_bytes(ns, M, O, H, W)
        scr2 = torch.empty(nb2 // 8, dtype=torch.float64, device="cuda")

        def accum():
            rc = lib.nint_ens_accum(P(seq), poff, T * img, M, P(y), None, 1, None, P(pix), P(sample), P(hist), None, P(scr2), nb2, ns, O, H, W,
                                    0, 0, H, W, _lib.stream_ptr())
            assert rc == 0, rc
        ms2 = timed(accum, args.iters)
        print(f"(c) nint_ens_accum   the same members: {ms2:8.3f} ms  {nbytes / 2 / 1e9:.3f} GB read  {nbytes / 2 / ms2 / 1e9:.3f} TB/s")

        def torch_loss():
            x = seq.view(N, M, T, O, H, W).detach().requires_grad_(True)
            t = y.view(N, 1, T, O, H, W)
            a = (x - t).abs().sum(dim=1)
            d = sum((x[:, i] - x[:, j]).abs() for i in range(M) for j in range(i + 1, M))
            kp = (M - 1 + 0.95) / (M * M * (M - 1))
            l = (a / M - kp * d).mean()
            l.backward()
            return l, x.grad
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms3 = timed(torch_loss, max(2, args.iters // 3))
        print(f"(d) torch CRPS + autograd, {N} x {M}: {ms3:8.3f} ms  peak memory above the inputs "
              f"{(torch.cuda.max_memory_allocated() - base) / 1e9:.2f} GB")
    pred = seq.view(B * T, O, H, W)
    yb = torch.randn(B * T, O, H, W, device="cuda")
    spec = LossSpec(0, 1, 0).on(seq.device, O)
    ms = timed(lambda: crop_loss_launch(pred, yb, slab, loss, stats, B * T, O, H, W, 0, 0, H, W, None, spec), args.iters)
    print(f"(b) nint_loss_crop_spec over the same {B * T} images: {ms:8.3f} ms  {nbytes / 1e9:.3f} GB moved  {nbytes / ms / 1e9:.3f} TB/s"
          f"  (+ {B * T * img * 4 / 1e9:.3f} GB of targets)")


def step_rows(args, B, T, O, H, W):
    C0 = 62 + O
    mk = lambda: pkg.ConvLSTM(C0, [64, 32, 16], [5, 3, 3], 3, out_channels=O, compute_dtype="bf16", lon_cyclic=True, feedback=True).cuda()
    X = torch.randn(B, T, C0, H, W, device="cuda")
    s = 1
    for N, M in ((4, 2), (1, 8)):
        yl, ye = torch.randn(B, T, O, H, W, device="cuda"), torch.randn(N, T, O, H, W, device="cuda")
        det = FusedTrainer(mk(), halo=(0, 0), rollout_from=s, sequence_loss=True)
        ens = FusedTrainer(mk(), halo=(0, 0), rollout_from=s, sequence_loss=True, ensemble_members=M, feedback_noise=0.05,
                           ensemble_loss=EnsembleLoss(0.95))
        for rnd in range(args.rounds):
            td = timed(lambda: det.step(X, yl), args.iters)
            te = timed(lambda: ens.step(X, ye), args.iters)
            print(f"(e) round {rnd}: deterministic roll-out step B={B}: {td:8.3f} ms;  ensemble step {N} x {M}: {te:8.3f} ms;  difference {te - td:+.3f} ms")
        net = ens.model
        eng = net._engine(X.device)
        ws = eng.acquire(B, T, H, W, True, False)
        net._pack_weights(eng)
        eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, s), feedback_grad=True)
        th = timed(lambda: eng.head_forward_seq(ws, net.conv.weight, net.conv.bias), args.iters)
        slab = ws.rollout_dpred(eng, O)
        tf = timed(lambda: eng.head_loss_seq_fused(ws, net.conv.weight, net.conv.bias, yl, slab, det.scratch, det.stats, (0, 0), H, W), args.iters)
        tc = timed(lambda: eng.rollout_cotangents(ws, net.conv.weight, slab_filled=True, dh_written=False), args.iters)
        eng.release(ws)
        print(f"    head_forward_seq {th:8.3f} ms;  the fused head / loss pass it replaces {tf:8.3f} ms;  the unfed steps' dh {tc:8.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_train_bench.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.manual_seed(0)
    B, T, O, H, W = 8, 12, 20, 100, 144
    loss_rows(args, B, T, O, H, W)
    step_rows(args, B, T, O, H, W)


if __name__ == "__main__":
    main()
