#!/usr/bin/env python3
"""The ensemble statistics kernel and the stochastic feedback against their alternatives, on the roll-out bench
stack: 20 feedback channels, 100 x 144 cyclic, bf16, spin-up 1 + horizon 11, 8 starts x 8 members.

    python tools/ensemble_bench.py [--iters 10] [--starts 8] [--members 8]

  (a)  nint_ens_accum reading the (lanes, T, O, H, W) head output in place: time and bytes per second of the algorithmic read
       (N * M * O * Hc * Wc f32)
  (b)  nint_skill_accum over the same images (every lane's free-run steps as samples): the byte rate of the kernel whose
       mapping (a) shares
  (c)  the torch expression a user would write on the device: gather the members, sort-based CRPS and `var`; its peak memory
  (d)  the closed-loop forward of 8 lanes with feedback_noise off and on (SeqEngine.forward); with --package-root TREE
       --closed-loop-only the same pass of another checkout of the package (the parent commit, which has no noise: off only)
  (e)  rollout_ensemble's wall time against `members` x rollout_skill on the same starts of a synthetic tracer_input record

Every variant is warmed up, then timed with device events over --iters passes."""
import argparse
import ctypes as C
import os
import sys

import torch

import time

_root = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--package-root=")]
sys.path.insert(0, os.path.abspath(_root[0]) if _root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nasa_niswan_amd as pkg  # noqa: E402
from nasa_niswan_amd.engine import InputNoise  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--starts", type=int, default=8)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--package-root", default=None, help="(as --package-root=TREE) import the package from this checkout")
    ap.add_argument("--closed-loop-only", action="store_true", help="row (d) alone; the noise row only where the package has it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench.py needs an MI355X: a timing taken elsewhere says nothing")
    S, M, O, H, W, spinup, horizon = args.starts, args.members, 20, 100, 144, 1, 11
    T, img = spinup + horizon, O * H * W
    torch.manual_seed(0)
    if not args.closed_loop_only:
        stats_rows(args, S, M, O, H, W, spinup, horizon)
    has_noise = "feedback_noise" in pkg.engine.SeqEngine.forward.__code__.co_varnames
    net = pkg.ConvLSTM(62 + O, [64, 32, 16], [5, 3, 3], 3, out_channels=O, compute_dtype="bf16", lon_cyclic=True, feedback=True).cuda().eval()
    X = torch.randn(8, T, 62 + O, H, W, device="cuda")
    eng = net._engine(X.device)
    with torch.no_grad():
        ws = eng.acquire(8, T, H, W, False, False)
        net._pack_weights(eng)
        fb = (net.conv.weight, net.conv.bias, spinup)
        for rnd in range(3):
            t = timed(lambda: eng.forward(ws, X, feedback=fb), args.iters)
            print(f"(d) closed-loop forward B=8 T={T}, feedback noise off: {t:8.3f} ms per pass ({T - spinup} feedback launches)")
            if has_noise:
                fn = InputNoise(0.05, seed=1, draw=1)
                t = timed(lambda: eng.forward(ws, X, feedback=fb, feedback_noise=fn), args.iters)
                print(f"(d) closed-loop forward B=8 T={T}, feedback noise on : {t:8.3f} ms per pass")
        eng.release(ws)
    if not args.closed_loop_only:
        rollout_rows(args, S, M, O, H, W, spinup, horizon)


def rollout_rows(args, S, M, O, H, W, spinup, horizon):
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from nasa_niswan_amd.inference import rollout_ensemble, rollout_skill
    T = spinup + horizon
    ds = SyntheticE33OMA_CRNN("train", padding=None, in_channels=62 + O, sequence_length=T, levels=O, n_steps=S * T + 2, grid=(H, W),
                              device="cuda", tracer_input=True)
    net = pkg.ConvLSTM(62 + O, [64, 32, 16], [5, 3, 3], 3, out_channels=O, compute_dtype="bf16", lon_cyclic=True, feedback=True).cuda().eval()
    starts = [1 + i * T for i in range(S)]

    def wall(fn):
        fn(); torch.cuda.synchronize()
        t0 = time.time()
        fn().sums()
        return (time.time() - t0) * 1e3

    te = wall(lambda: rollout_ensemble(net, ds, starts, horizon, spinup, M, ic_noise=0.05, feedback_noise=0.02, batch_size=8, halo=(0, 0)))
    ts = wall(lambda: rollout_skill(net, ds, starts, horizon, spinup, 8, halo=(0, 0)))
    print(f"(e) rollout_ensemble {S} starts x {M} members: {te:8.1f} ms wall;  rollout_skill on the same starts: {ts:8.1f} ms, "
          f"x {M} = {M * ts:8.1f} ms")


def stats_rows(args, S, M, O, H, W, spinup, horizon):
    from nasa_niswan_amd.inference import EnsembleAccumulator, SkillAccumulator
    T, img = spinup + horizon, O * H * W
    seq = torch.randn(S * M, T, O, H, W, device="cuda")
    y = torch.randn(S * horizon, O, H, W, device="cuda")
    off = [((i * M) * T + spinup + j) * img for i in range(S) for j in range(horizon)]
    slots = [j for _ in range(S) for j in range(horizon)]
    acc = EnsembleAccumulator(O, H, W, M, nslots=horizon, device="cuda")

    def ens():
        acc._rows.clear(); acc._row_slots.clear()
        acc.update(seq, off, T * img, y, slots)

    ms = timed(ens, args.iters)
    nbytes = S * horizon * M * img * 4
    print(f"(a) nint_ens_accum   N={S * horizon} M={M}: {ms:8.3f} ms  {nbytes / 1e9:.3f} GB read  {nbytes / ms / 1e9:.3f} TB/s")

    sk = SkillAccumulator(O, H, W, nslots=1, device="cuda")
    pred = seq.view(S * M * T, O, H, W)
    ys = torch.randn(S * M * T, O, H, W, device="cuda")

    def skill():
        sk._rows.clear()
        sk.update_from_pred(pred, ys, (0, 0))

    ms2 = timed(skill, args.iters)
    nb2 = pred.numel() * 4
    print(f"(b) nint_skill_accum N={pred.shape[0]}: {ms2:8.3f} ms  {nb2 / 1e9:.3f} GB read  {nb2 / ms2 / 1e9:.3f} TB/s (prediction bytes; "
          f"the target doubles them: {2 * nb2 / ms2 / 1e9:.3f} TB/s)")
    print(f"    byte rate of (a) over (b): {(nbytes / ms) / (nb2 / ms2):.2f}")

    idx = torch.tensor([[(i * M + m) * T + spinup + j for m in range(M)] for i in range(S) for j in range(horizon)], device="cuda")

    def torch_stats():
        x = seq.view(S * M * T, O, H, W)[idx.reshape(-1)].view(S * horizon, M, O, H, W)          # the gather a user writes
        xs, _ = torch.sort(x, dim=1)
        k = torch.arange(M, device="cuda", dtype=torch.float32).view(1, M, 1, 1, 1)
        a = (x - y[:, None]).abs().mean(dim=1)
        d = ((2 * k - M + 1) * xs).sum(dim=1) / (M * (M - 1))                                   # sum_{i<j} |x_i - x_j| / (M (M-1)), sorted
        return (a - d).mean(dim=0), x.var(dim=1).mean(dim=0), ((x.mean(dim=1) - y) ** 2).mean(dim=0)

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms3 = timed(torch_stats, max(2, args.iters // 3))
    print(f"(c) torch sort-based CRPS + var: {ms3:8.3f} ms  peak memory above the inputs {(torch.cuda.max_memory_allocated() - base) / 1e9:.2f} GB "
          f"(f32 throughout, no rank histogram, no per-sample rows)")


if __name__ == "__main__":
    main()
