#!/usr/bin/env python3
"""The closed-loop forward pass against its alternatives, on the bench stack with feedback channels:
hidden 64/32/16, k 5/3/3, 100 x 144 cyclic, T = 12, B = 8, bf16, C = 62 + 20, O = 20, free_from = 1.

    python tools/closed_loop_bench.py [--rounds 7] [--iters 20] [--dtype bf16] [--batch 8] ...

  (a)  the closed-loop pass (SeqEngine.forward(feedback=...)), alone and with the per-step head behind it
  (b)  the same roll-out driven from the host with the calls the package had before: T windows of one step through
       net(x_t, state, return_state="device"), the prediction concatenated into the next step's input on the host side
  (c)  the open-loop forward of the same shape, in the engine's wave mode and time-major (wave 0)

Every variant is warmed up, then timed with device events over --iters passes; the variants alternate inside a round and the
rounds give the spread (min / median / max of the per-pass time).  The head_feedback kernel alone is tools/kbench.py's row."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nasa_niswan_amd as pkg  # noqa: E402
from nasa_niswan_amd import engine as E  # noqa: E402


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
    ap.add_argument("--free-from", type=int, default=1)
    ap.add_argument("--zero-pad", action="store_true", help="zero padding instead of cyclic longitude")
    ap.add_argument("--residual", action="store_true", help="the residual head (DESIGN.md 4.22): the closed-loop passes of (a) feed round(x + head)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_bench.py needs an MI355X: a timing taken elsewhere says nothing")
    hidden, ks = [int(v) for v in args.hidden.split(",")], [int(v) for v in args.ks.split(",")]
    B, T, C_, O, H, W, s = args.batch, args.T, args.C, args.O, args.H, args.W, args.free_from
    torch.manual_seed(0)
    net = pkg.ConvLSTM(C_, hidden, ks, len(hidden), out_channels=O, compute_dtype=args.dtype, lon_cyclic=not args.zero_pad,
                       feedback=True).cuda().eval()
    X = torch.randn(B, T, C_, H, W, device="cuda")
    eng = net._engine(X.device)
    w, b = net.conv.weight, net.conv.bias
    ws = eng.acquire(B, T, H, W, False, False)
    net._pack_weights(eng)
    out = {}

    def closed():
        eng.forward(ws, X, feedback=(w, b, s), **({"residual": O} if args.residual else {}))

    def closed_seq():
        eng.forward(ws, X, feedback=(w, b, s), **({"residual": O} if args.residual else {}))
        out["closed"] = eng.head_forward_seq(ws, w, b)

    def open_(wave):
        def run():
            old, E.FORCE_WAVE = E.FORCE_WAVE, wave
            try:
                eng.forward(ws, X)
            finally:
                E.FORCE_WAVE = old
        return run

    def host():
        state, pred, preds = None, None, []
        for t in range(T):
            x_t = X[:, t:t + 1]
            if t >= max(s, 1):
                x_t = torch.cat([x_t[:, :, :C_ - O], pred[:, None]], dim=2)
            pred, state = net(x_t.contiguous(), state, return_state="device")
            preds.append(pred)
        out["host"] = torch.cat(preds, dim=1)

    variants = [("(a) closed loop", closed), ("(a) closed loop + per-step head", closed_seq),
                ("(b) host-driven roll-out, T one-step windows", host),
                ("(c) open loop, engine's wave mode", open_(None)), ("(c) open loop, time-major (wave 0)", open_(0))]
    with torch.no_grad():
        for _, fn in variants:                     # warm-up: every shape and code object the timed windows use
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        d = (out["closed"] - out["host"]).abs().max().item()
        print(f"closed loop vs host-driven roll-out: max |difference| of the per-step predictions {d:.3e} "
              f"(max |prediction| {out['closed'].abs().max().item():.3e})")
        times = {name: [] for name, _ in variants}
        for r in range(args.rounds):
            order = variants if r % 2 == 0 else variants[::-1]
            for name, fn in order:
                times[name].append(timed(fn, args.iters))
    print(f"{args.dtype} B={B} T={T} C={C_} O={O} {H}x{W} hidden={hidden} k={ks} free_from={s} "
          f"{'zero padding' if args.zero_pad else 'cyclic longitude'}; wave mode {ws.seq.wave}; {args.rounds} rounds x {args.iters} passes")
    print(f"{'variant':48s} {'min':>9s} {'median':>9s} {'max':>9s}  ms per pass")
    for name, _ in variants:
        v = times[name]
        print(f"{name:48s} {min(v):9.3f} {statistics.median(v):9.3f} {max(v):9.3f}")
    eng.release(ws)


if __name__ == "__main__":
    main()
