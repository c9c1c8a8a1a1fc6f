#!/usr/bin/env python3
"""What checkpointed BPTT costs and saves, on one MI355X in one process, bf16:

  bench     the bench stack ConvLSTM(62, (64, 32, 16), (5, 3, 3)), head out 20, 100 x 154, B = 8, T = 12
  cfg3      BASELINE configs[3]: ConvLSTM(62, (128, 128, 128), (3, 3, 3)), head out 20, 190 x 298, B = 2, T = 24

For each, one `FusedTrainer.step` with the whole window resident against `bptt_segments` = 2 / 3 / 4: the step time (device
events; the median over `--windows` windows of `--reps` back-to-back steps, the variants alternating window by window so
that a drifting clock touches all of them alike) and `torch.cuda.max_memory_allocated` of a step over what was allocated
before the trainer's first one (workspaces, kept states, the split-K scratch; weights, the batch and the optimizer's
moments are in the base).  Every variant has a model and an engine of its own; the memory figure is taken from a fresh
engine, before the timed windows.

    python tools/segment_cost.py [--reps 5] [--windows 5] [--only bench|cfg3] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (C_in, hidden, kernels, out, B, T, Hp, Wp, halo, grid)
CASES = {
    "bench": (62, (64, 32, 16), (5, 3, 3), 20, 8, 12, 100, 154, (5, 5), (90, 144)),
    "cfg3": (62, (128, 128, 128), (3, 3, 3), 20, 2, 24, 190, 298, (5, 5), (180, 288)),
}
SEGMENTS = (None, 2, 3, 4)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps                # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", type=str, default=None, choices=sorted(CASES))
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_cost.py measures on an MI355X; there is nothing to report without one")
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.trainer import FusedTrainer
    from oracle import convlstm_oracle as O
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "windows": args.windows, "dtype": "bf16",
           "unit": "ms per step, MB peak over the base"}
    for name, (Cin, hidden, ks, out, B, T, Hp, Wp, halo, grid) in CASES.items():
        if args.only and name != args.only:
            continue
        params = O.synth_params(Cin, hidden, ks, len(hidden), out_channels=out, seed=0)
        gen = torch.Generator().manual_seed(1)
        X = torch.randn(B, T, Cin, Hp, Wp, generator=gen).to(dev)
        y = torch.randn(B, out, *grid, generator=gen).to(dev)
        steps, peak = {}, {}
        for n in SEGMENTS:
            net = pkg.ConvLSTM(Cin, list(hidden), list(ks), len(hidden), out_channels=out, compute_dtype="bf16").to(dev)
            net.load_state_dict(params)
            tr = FusedTrainer(net, lr=1e-4, halo=halo, bptt_segments=n)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tr.step(X, y)                           # allocates every workspace this variant will ever hold
            torch.cuda.synchronize()
            peak[n] = (torch.cuda.max_memory_allocated() - base) / 1e6
            tr.step(X, y)
            steps[n] = lambda tr=tr: tr.step(X, y)
        torch.cuda.synchronize()
        samples = {n: [] for n in SEGMENTS}
        for _ in range(args.windows):
            for n, fn in steps.items():
                samples[n].append(window(fn, args.reps))
        whole = statistics.median(samples[None])
        res[name] = {"B": B, "T": T, "grid": [Hp, Wp], "stack": [Cin, list(hidden), list(ks), out]}
        for n in SEGMENTS:
            v = samples[n]
            res[name]["whole" if n is None else f"n{n}"] = {
                "ms": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                "vs_whole": round(statistics.median(v) / whole, 4), "peak_mb": round(peak[n], 1)}
        del steps, samples
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
