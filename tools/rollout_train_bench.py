#!/usr/bin/env python3
"""The roll-out training step against its teacher-forced alternatives, on the closed-loop bench stack:
hidden 64/32/16, k 5/3/3, 100 x 144 cyclic, T = 12, B = 8, bf16, C = 62 + 20, O = 20, rollout_from = 1.

    python tools/rollout_train_bench.py [--rounds 7] [--iters 10] [--dtype bf16] [--batch 8] [--sequence-loss] ...

  (a)  FusedTrainer(rollout_from=s).step: the closed-loop forward, the fused head / loss pass, BPTT through the fed-back
       prediction, the head's gradients from the slab, Adam
  (b)  the teacher-forced step of the same shape planned as (a)'s BPTT is: time-major, all-classic (FUSE_BWD = 1, FORCE_WAVE = 0)
  (c)  the default teacher-forced step
  --sampling-prob P [P ...]: (s) FusedTrainer(rollout_from=s, sampling_prob=P).step for every P: a fresh
       feed mask per step.  P = 1 is (a), call for call
  --input-noise STD: (n) (c) with FusedTrainer(input_noise=STD): one nint_input_noise launch more per step

Expectation to check, not a gate: (a) is (b) plus T - s feedback launches forward, T - s backward launches and the x columns
of layer 0's dgrad at the fed steps.  Every variant is warmed up, then timed with device events over --iters steps; the
variants alternate inside a round and the rounds give the spread (min / median / max of the per-step time).  The
head_feedback_bwd kernel alone is tools/kbench.py's row."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nasa_niswan_amd as pkg  # noqa: E402
from nasa_niswan_amd import engine as E  # noqa: E402
from nasa_niswan_amd.trainer import FusedTrainer  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=12)
    ap.add_argument("--C", type=int, default=82, help="input channels, the last --O of them feedback channels")
    ap.add_argument("--O", type=int, default=20)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--W", type=int, default=144)
    ap.add_argument("--hidden", default="64,32,16")
    ap.add_argument("--ks", default="5,3,3")
    ap.add_argument("--rollout-from", type=int, default=1)
    ap.add_argument("--sequence-loss", action="store_true")
    ap.add_argument("--sampling-prob", type=float, nargs="*", default=[], help="also time the scheduled-sampling step at these probabilities")
    ap.add_argument("--input-noise", type=float, default=None, metavar="STD", help="also time the teacher-forced default step with this input noise on the feedback channels")
    ap.add_argument("--zero-pad", action="store_true", help="zero padding instead of cyclic longitude")
    ap.add_argument("--residual", action="store_true", help="the residual head (DESIGN.md 4.22): ConvLSTM(residual=True) in every variant")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_train_bench.py needs an MI355X: a timing taken elsewhere says nothing")
    hidden, ks = [int(v) for v in args.hidden.split(",")], [int(v) for v in args.ks.split(",")]
    B, T, C_, O, H, W, s = args.batch, args.T, args.C, args.O, args.H, args.W, args.rollout_from
    sq = args.sequence_loss
    torch.manual_seed(0)
    X = torch.randn(B, T, C_, H, W, device="cuda")
    y = torch.randn(*((B, T, O, H, W) if sq else (B, O, H, W)), device="cuda")

    def trainer(**kw):
        # (one model each: a step moves the weights; a tiny learning rate keeps the three on the same data path all run long)
        net = pkg.ConvLSTM(C_, hidden, ks, len(hidden), out_channels=O, compute_dtype=args.dtype, lon_cyclic=not args.zero_pad,
                           feedback=True, **({"residual": True} if args.residual else {})).cuda()
        return FusedTrainer(net, lr=1e-6, halo=(0, 0), sequence_loss=sq, **kw)
    tr_a, tr_b, tr_c = trainer(rollout_from=s), trainer(), trainer()

    def classic():
        # a workspace keeps the fuse_bwd it was built with: the time-major all-classic plan is set on it for this step alone
        eng = tr_b.model._engine(X.device)
        old_w, E.FORCE_WAVE = E.FORCE_WAVE, 0
        ws = eng.acquire(B, T, H, W, True, False)
        old_f, ws.seq.fuse_bwd = ws.seq.fuse_bwd, 1
        eng.release(ws)
        try:
            tr_b.step(X, y)
        finally:
            ws.seq.fuse_bwd, E.FORCE_WAVE = old_f, old_w

    variants = [("(a) roll-out step", lambda: tr_a.step(X, y)), ("(b) teacher-forced, time-major all-classic", classic),
                ("(c) teacher-forced, default plan", lambda: tr_c.step(X, y))]
    for p in args.sampling_prob:
        tr_s = trainer(rollout_from=s, sampling_prob=p, sampling_seed=0)
        variants.append((f"(s) scheduled sampling, p = {p:g}", lambda tr_s=tr_s: tr_s.step(X, y)))
    if args.input_noise is not None:
        tr_n = trainer(input_noise=args.input_noise)
        variants.append((f"(n) teacher-forced, default plan, noise {args.input_noise:g}", lambda: tr_n.step(X, y)))
    for _, fn in variants:                         # warm-up: every shape and code object the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        order = variants if r % 2 == 0 else variants[::-1]
        for name, fn in order:
            times[name].append(timed(fn, args.iters))
    print(f"{args.dtype} B={B} T={T} C={C_} O={O} {H}x{W} hidden={hidden} k={ks} rollout_from={s} {'RESIDUAL head ' if args.residual else ''}"
          f"{'sequence loss' if sq else 'last-step loss'} {'zero padding' if args.zero_pad else 'cyclic longitude'}; "
          f"{args.rounds} rounds x {args.iters} steps; loss (a) {float(tr_a.step(X, y)):.5f} (c) {float(tr_c.step(X, y)):.5f}")
    print(f"{'variant':48s} {'min':>9s} {'median':>9s} {'max':>9s}  ms per step")
    for name, _ in variants:
        v = times[name]
        print(f"{name:48s} {min(v):9.3f} {statistics.median(v):9.3f} {max(v):9.3f}")


if __name__ == "__main__":
    main()
