#!/usr/bin/env python3
"""What carrying the recurrent state costs, at the reference stack (5, [64, 32, 16], [5, 3, 3]) on the
100 x 154 grid in bf16, B = 1 and B = 8, from device events on one MI355X:

  handoff   one SeqEngine.load_state + save_state pair: two nint_state_copy launches, the state never leaves slab form
  tensors   the same carry through f32 NCHW tensors: ConvLSTMState.tensors() (2L unpack launches) and
            SeqEngine.state_from_tensors (2L fills + 2L pack launches)
  step      one T = 1 `net(x, state, return_state="device")` call under torch.no_grad(): roll-forward inference, one record
            step per call

Each figure is the median over `--windows` windows of `--reps` back-to-back repetitions (the three kinds alternate window
by window, so a drifting clock touches all of them alike); min and max of the windows are printed beside it.

    python tools/state_cost.py [--reps 200] [--windows 7] [--out FILE.json]
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


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per repetition


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("state_cost.py measures on an MI355X; there is nothing to report without one")
    import nasa_niswan_amd as pkg
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "windows": args.windows, "dtype": "bf16", "grid": [100, 154],
           "stack": [5, [64, 32, 16], [5, 3, 3]], "unit": "us"}
    net = pkg.ConvLSTM(5, [64, 32, 16], [5, 3, 3], 3, compute_dtype="bf16").to(dev).eval()
    eng = net._engine(dev)
    for B in (1, 8):
        x = torch.randn(B, 1, 5, 100, 154, device=dev)
        ws = eng.acquire(B, 1, 100, 154, False, True)
        with torch.no_grad():
            _, st = net(x, return_state="device")
        box = {"st": st}

        def handoff():
            eng.load_state(ws, box["st"])
            eng.save_state(ws, box["st"])

        def tensors():
            box["st"] = eng.state_from_tensors(box["st"].tensors())

        def step():
            with torch.no_grad():
                _, box["st"] = net(x, box["st"], return_state="device")

        kinds = {"handoff": handoff, "tensors": tensors, "step": step}
        for fn in kinds.values():                  # every shape the timed windows use, code objects loaded
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in kinds}
        for _ in range(args.windows):
            for k, fn in kinds.items():
                samples[k].append(window(fn, args.reps))
        eng.release(ws)
        res[f"B{B}"] = {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                        for k, v in samples.items()}
        state_bytes = sum(t.numel() * t.element_size() for t in st.h + st.c)
        res[f"B{B}"]["state_bytes"] = state_bytes
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
