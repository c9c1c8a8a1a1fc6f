#!/usr/bin/env python3
"""What the guarded optimizer step costs: ms per FusedTrainer step on the bench workload (cfg1-20level: ConvLSTM(62, (64,32,16),
(5,3,3)), 20 outputs, T = 12, 100x154, bf16) with max_grad_norm / skip_nonfinite on against off, in alternating windows of one
process, timed with device events.

    python tools/clip_cost.py [--batch 8] [--steps 40] [--rounds 6] [--warmup 10]
    python tools/clip_cost.py --root /path/to/another/checkout      # that tree's package (built); one without the guard
                                                                    # is measured "off" only: the step time to put beside
Prints one line per round and a JSON line with the medians."""
import argparse
import inspect
import json
import os
import statistics
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import nasa_niswan_amd as pkg
    pkg.load_library()
    from nasa_niswan_amd.trainer import FusedTrainer
    has_guard = "max_grad_norm" in inspect.signature(FusedTrainer.__init__).parameters
    variants = {"off": {}}
    if has_guard:
        variants["on"] = dict(max_grad_norm=args.max_grad_norm, skip_nonfinite=True)
    gen = torch.Generator(device="cuda").manual_seed(1000)
    X = torch.randn(args.batch, 12, 62, 100, 154, device="cuda", generator=gen)
    y = torch.randn(args.batch, 20, 90, 144, device="cuda", generator=gen)
    trainers = {}
    for name, kw in variants.items():
        torch.manual_seed(0)
        net = pkg.ConvLSTM(62, [64, 32, 16], [5, 3, 3], 3, out_channels=20, compute_dtype="bf16").cuda()
        trainers[name] = FusedTrainer(net, lr=1e-3, betas=(0.5, 0.999), halo=(5, 5), **kw)
        for _ in range(args.warmup):
            trainers[name].step(X, y)
    torch.cuda.synchronize()
    ms = {name: [] for name in trainers}
    for r in range(args.rounds):
        for name, tr in trainers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                tr.step(X, y)
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / args.steps)
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.4f} ms/step" for k, v in ms.items()), flush=True)
    out = {"root": os.path.abspath(args.root), "batch": args.batch, "steps": args.steps, "rounds": args.rounds,
           "ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
           "ms_per_step_min_max": {k: [min(v), max(v)] for k, v in ms.items()}}
    if has_guard:
        out["grad_stats"] = trainers["on"].grad_stats()
        out["guard_cost_ms"] = out["ms_per_step"]["on"] - out["ms_per_step"]["off"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
