#!/usr/bin/env python3
"""What freezing the lower layers saves, on one MI355X in one process: `FusedTrainer.step` on the bench
workload -- ConvLSTM(62, (64, 32, 16), (5, 3, 3)), head out 20, 100 x 154, bf16, B = 8, T = 12 -- with `freeze_layers` =
0, 1, 2, 3.

Per setting: the step time between device events -- the median, min and max over `--windows` windows of `--reps`
back-to-back steps (100 timed steps by default), the settings alternating window by window so that a drifting clock touches
all of them alike -- and `torch.cuda.max_memory_allocated` of a step over what was allocated before the trainer's first one.
Every setting has a model and an engine of its own.  `--freeze 0` passes no fine-tuning argument at all, so the same file
measures a checkout from before the switch existed: the unfrozen step must sit inside that one's run-to-run spread.

    python tools/finetune_step.py [--freeze 0 1 2 3] [--reps 10] [--windows 10] [--out FILE.json]
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

CIN, HIDDEN, KS, OUT, B, T, HP, WP, HALO, GRID = 62, (64, 32, 16), (5, 3, 3), 20, 8, 12, 100, 154, (5, 5), (90, 144)


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
    ap.add_argument("--freeze", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_step.py measures on an MI355X; there is nothing to report without one")
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.trainer import FusedTrainer
    from oracle import convlstm_oracle as O
    dev = torch.device("cuda", 0)
    params = O.synth_params(CIN, HIDDEN, KS, len(HIDDEN), out_channels=OUT, seed=0)
    gen = torch.Generator().manual_seed(1)
    X = torch.randn(B, T, CIN, HP, WP, generator=gen).to(dev)
    y = torch.randn(B, OUT, *GRID, generator=gen).to(dev)
    steps, peak = {}, {}
    for f in args.freeze:
        net = pkg.ConvLSTM(CIN, list(HIDDEN), list(KS), len(HIDDEN), out_channels=OUT, compute_dtype="bf16").to(dev)
        net.load_state_dict(params)
        kw = dict(freeze_layers=f) if f else {}
        tr = FusedTrainer(net, lr=1e-4, halo=HALO, **kw)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tr.step(X, y)                               # allocates every workspace this setting will ever hold
        torch.cuda.synchronize()
        peak[f] = (torch.cuda.max_memory_allocated() - base) / 1e6
        steps[f] = lambda tr=tr: tr.step(X, y)
    for _ in range(args.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    samples = {f: [] for f in steps}
    for _ in range(args.windows):
        for f, fn in steps.items():
            samples[f].append(window(fn, args.reps))
    res = {"device": torch.cuda.get_device_name(0), "workload": "cfg1-20level", "dtype": "bf16", "B": B, "T": T, "reps": args.reps,
           "windows": args.windows, "timed_steps": args.reps * args.windows, "unit": "ms per step, MB peak over the base"}
    ref = statistics.median(samples[args.freeze[0]])
    for f, v in samples.items():
        res[f"freeze{f}"] = {"ms": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                             "vs_first": round(statistics.median(v) / ref, 4), "peak_mb": round(peak[f], 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
