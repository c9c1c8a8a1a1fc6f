#!/usr/bin/env python3
"""The zonal power spectrum kernel against the torch expression a user would write, at the roll-out bench shape:
20 outputs on 100 x 144 cyclic, spin-up 1 + horizon 11, 8 starts x 8 members.

    python tools/spectrum_bench.py [--iters 10] [--starts 8] [--members 8] [--skip-rollout]

  (a)  nint_spec_accum reading the (lanes, T, O, H, W) head output in place (its two launches): time, the bytes of the
       algorithmic read (N * (M + 1) * O * Hc * Wc f32) and the f64 rate of the direct transform it performs
       (N * (M + 1) * O * Hc rows x Wc * K real-by-complex multiply-adds = 4 flop each)
  (b)  the equivalent torch expression on the same device tensor: gather the members, torch.fft.rfft of the f64 crop and the
       five weighted reductions per lead time; its time and its peak memory above the inputs
  (c)  rollout_ensemble(spectrum=acc) against rollout_ensemble() on the same starts of a synthetic tracer_input record: wall
       time, alternating, three rounds

Every variant is warmed up, then timed with device events over --iters passes."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nasa_niswan_amd as pkg  # noqa: E402


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
    ap.add_argument("--skip-rollout", action="store_true", help="rows (a) and (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_bench.py needs an MI355X: a timing taken elsewhere says nothing")
    S, M, O, H, W, spinup, horizon = args.starts, args.members, 20, 100, 144, 1, 11
    torch.manual_seed(0)
    kernel_rows(args, S, M, O, H, W, spinup, horizon)
    if not args.skip_rollout:
        rollout_rows(args, S, M, O, H, W, spinup, horizon)


def kernel_rows(args, S, M, O, H, W, spinup, horizon):
    from nasa_niswan_amd.inference import SpectrumAccumulator
    T, img, K = spinup + horizon, O * H * W, W // 2 + 1
    N = S * horizon
    lat = np.linspace(-89.0, 89.0, H)
    seq = torch.randn(S * M, T, O, H, W, device="cuda")
    y = torch.randn(N, O, H, W, device="cuda")
    off = [((i * M) * T + spinup + j) * img for i in range(S) for j in range(horizon)]
    slots = [j for _ in range(S) for j in range(horizon)]
    acc = SpectrumAccumulator(O, H, W, M=M, nslots=horizon, lat=lat, device="cuda", halo=(0, 0))

    def spec():
        acc.update(seq, off, T * img, y, slots)

    ms = timed(spec, args.iters)
    nbytes = N * (M + 1) * img * 4
    flop = 4.0 * N * (M + 1) * O * H * W * K
    print(f"(a) nint_spec_accum  N={N} M={M} O={O} {H}x{W} K={K}: {ms:8.3f} ms  {nbytes / 1e9:.3f} GB read ({nbytes / ms / 1e9:.3f} TB/s)  "
          f"{flop / 1e9:.2f} GFLOP f64 of the direct transform ({flop / ms / 1e9:.2f} TFLOP/s)")

    idx = torch.tensor([[(i * M + m) * T + spinup + j for m in range(M)] for i in range(S) for j in range(horizon)], device="cuda")
    w = torch.from_numpy(np.cos(np.deg2rad(lat))).cuda().view(1, 1, H, 1)
    sl = torch.tensor(slots, device="cuda")

    def torch_spec():
        x = seq.view(S * M * T, O, H, W)[idx.reshape(-1)].view(N, M, O, H, W)                   # the gather a user writes
        P = torch.fft.rfft(x.double(), dim=-1)                                                  # (N, M, O, H, K) complex128
        Y = torch.fft.rfft(y.double(), dim=-1)
        Sm = P.sum(dim=1)
        cross = Sm * Y.conj()
        rows = torch.stack([(w * (Y.real ** 2 + Y.imag ** 2)).sum(dim=2), (w * (P.real ** 2 + P.imag ** 2).sum(dim=1)).sum(dim=2),
                            (w * cross.real).sum(dim=2), (w * cross.imag).sum(dim=2),
                            (w * (Sm.real ** 2 + Sm.imag ** 2)).sum(dim=2)], dim=1)             # (N, 5, O, K)
        return torch.zeros(horizon, 5, O, K, dtype=torch.float64, device="cuda").index_add_(0, sl, rows)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms2 = timed(torch_spec, max(2, args.iters // 3))
    peak = torch.cuda.max_memory_allocated() - base
    scratch = acc._scratch.numel() * 8 + acc.spec.numel() * 8 + acc.tw.numel() * 8
    print(f"(b) torch rfft of the f64 crop + five weighted reductions: {ms2:8.3f} ms  peak memory above the inputs {peak / 1e9:.2f} GB "
          f"(the kernel's spec + scratch + table: {scratch / 1e6:.2f} MB)")
    print(f"    time of (a) over (b): {ms / ms2:.2f}")
    # the two agree (the kernel's table against rocFFT's): a sanity figure, not a test
    fresh = SpectrumAccumulator(O, H, W, M=M, nslots=horizon, lat=lat, device="cuda", halo=(0, 0))
    fresh.update(seq, off, T * img, y, slots)
    ref = torch_spec()
    rel = ((fresh.spec - ref).abs().amax() / ref.abs().amax()).item()
    print(f"    largest |kernel - torch| over the largest |torch| entry: {rel:.3e}")


def rollout_rows(args, S, M, O, H, W, spinup, horizon):
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    from nasa_niswan_amd.inference import SpectrumAccumulator, rollout_ensemble
    T = spinup + horizon
    ds = SyntheticE33OMA_CRNN("train", padding=None, in_channels=62 + O, sequence_length=T, levels=O, n_steps=S * T + 2, grid=(H, W),
                              device="cuda", tracer_input=True)
    net = pkg.ConvLSTM(62 + O, [64, 32, 16], [5, 3, 3], 3, out_channels=O, compute_dtype="bf16", lon_cyclic=True, feedback=True).cuda().eval()
    starts = [1 + i * T for i in range(S)]
    kw = dict(ic_noise=0.05, feedback_noise=0.02, batch_size=8, halo=(0, 0))

    def plain():
        return rollout_ensemble(net, ds, starts, horizon, spinup, M, **kw).sums()

    def with_spec():
        acc = SpectrumAccumulator(O, H, W, M=M, nslots=horizon, device="cuda", halo=(0, 0))
        r = rollout_ensemble(net, ds, starts, horizon, spinup, M, spectrum=acc, **kw).sums()
        acc.sums()
        return r

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3

    plain(), with_spec()
    for rnd in range(3):
        tp, tw = wall(plain), wall(with_spec)
        print(f"(c) rollout_ensemble {S} starts x {M} members, round {rnd}: {tp:8.1f} ms wall;  with spectrum=acc: {tw:8.1f} ms "
              f"(+{tw - tp:6.1f} ms)")


if __name__ == "__main__":
    main()
