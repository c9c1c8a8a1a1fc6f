#!/usr/bin/env python3
"""Per-kernel micro-benchmark at the bench workload's shapes (HIP events on the launch stream).
    python tools/kbench.py [--dtype bf16] [--batch 8] [--iters 20] [--only fwd0,dgrad0,head_skill,head_loss,head_loss_spec,...]
Prints one line per kernel: average ms, algorithmic TFLOP/s (or GB/s)."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nasa_niswan_amd as pkg  # noqa: E402
from nasa_niswan_amd.engine import LayerCfg, SeqEngine  # noqa: E402


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=12)
    ap.add_argument("--C", type=int, default=62)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--O", type=int, default=20, help="head outputs of the evaluation rows (head_fwd, head_skill, skill_plain)")
    ap.add_argument("--only", default="")
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--W", type=int, default=154)
    ap.add_argument("--zeros", action="store_true", help="all-zero inputs and weights (data-dependent power / clock check)")
    ap.add_argument("--lib", default=None, help="load this build of the library instead of the product one (A/B copies, stamp builds)")
    ap.add_argument("--wide", type=int, default=-1, help="nint_layer.wide of every layer: weight-gradient kernel family (-1: the engine's choice)")
    ap.add_argument("--tile-rows", type=int, default=0, help="force 4- or 8-row tiles for the gate / dgrad kernels")
    ap.add_argument("--hidden", default="64,32,16", help="hidden widths of the three layers (BASELINE configs[3]: 128,128,128)")
    ap.add_argument("--ks", default="5,3,3", help="kernel sizes of the three layers (configs[3]: 3,3,3)")
    ap.add_argument("--split", type=int, default=1, help="issue the forward gate kernel as this many launches over image groups")
    args = ap.parse_args()
    lib = pkg.load_library(args.lib) if args.lib else pkg.load_library()
    hidden, ks = tuple(int(v) for v in args.hidden.split(",")), tuple(int(v) for v in args.ks.split(","))
    cfgs, cin = [], args.C
    for ch, k in zip(hidden, ks):
        cfgs.append(LayerCfg(cin, ch, k)); cin = ch
    from nasa_niswan_amd import engine as _engine
    _engine.FORCE_TILE_ROWS = args.tile_rows
    eng = SeqEngine(cfgs, args.dtype, "cuda")
    for ly in eng.layers:
        ly.tile_rows = args.tile_rows
        if args.wide >= 0:
            ly.wide = args.wide
    B, T, H, W = args.batch, args.T, args.H, args.W
    ws = eng.acquire(B, T, H, W, True, False)
    ws_w = [torch.randn(4 * c.Ch, c.Cx + c.Ch, c.k, c.k, device="cuda") * (0.0 if args.zeros else 0.05) for c in cfgs]
    ws_b = [torch.zeros(4 * c.Ch, device="cuda") for c in cfgs]
    eng.pack_weights(ws_w, ws_b)
    X = torch.randn(B, T, args.C, H, W, device="cuda") * (0.0 if args.zeros else 1.0)
    eng.forward(ws, X)       # fills every slab with realistic (random-data) values
    for l in range(len(cfgs)):
        ws.dh[l].view(torch.bfloat16 if eng.es == 2 else torch.float32).normal_(); ws.dc[l].normal_()
    g, st = C.byref(ws.g), None
    es = eng.es
    halo_px, comp_px = ws.g.Hh * ws.g.Wh, H * W
    only = set(args.only.split(",")) if args.only else None
    rows = []

    def run(name, fn, flops=None, bytes_=None):
        if only and name not in only:
            return
        ms = timeit(fn, args.iters)
        extra = f"{flops / ms / 1e9:8.1f} TFLOP/s" if flops else (f"{bytes_ / ms / 1e6:8.1f} GB/s" if bytes_ else "")
        print(f"{name:22s} {ms * 1e3:9.1f} us  {extra}", flush=True)
        rows.append((name, ms))

    for l, cfg in enumerate(cfgs):
        ly = eng.layers[l]
        xs = ws.xs.data_ptr() + 1 * B * halo_px * ly.Cxp * es if l == 0 else ws.h[l - 1].data_ptr() + 2 * B * halo_px * ly.Cxp * es
        hs = B * halo_px * ly.Chp * es
        cs = B * comp_px * ly.Chp * 4
        gs = B * comp_px * 4 * ly.Ch16 * es
        dgs = B * halo_px * 4 * ly.Ch16 * es
        fl = 2.0 * B * H * W * cfg.k ** 2 * (cfg.Cx + cfg.Ch) * 4 * cfg.Ch

        def fwd(ly=ly, xs=xs, hs=hs, cs=cs, gs=gs, l=l):
            nb = B // args.split
            for part in range(args.split):      # image groups: every slab pointer advances by the group's images
                f = part * nb
                assert lib.nint_cell_fwd(C.byref(ly), g, eng.dt, nb if part < args.split - 1 else B - f,
                                         C.c_void_p(xs + f * halo_px * ly.Cxp * es),
                                         C.c_void_p(ws.h[l].data_ptr() + hs + f * halo_px * ly.Chp * es),
                                         C.c_void_p(ws.c[l].data_ptr() + cs + f * comp_px * ly.Chp * 4),
                                         C.c_void_p(ws.h[l].data_ptr() + 2 * hs + f * halo_px * ly.Chp * es),
                                         C.c_void_p(ws.c[l].data_ptr() + 2 * cs + f * comp_px * ly.Chp * 4),
                                         C.c_void_p(ws.gates[l].data_ptr() + gs + f * comp_px * 4 * ly.Ch16 * es), st) == 0
        run(f"fwd{l}", fwd, fl)

        def pw(ly=ly, cs=cs, gs=gs, dgs=dgs, l=l):
            assert lib.nint_cell_bwd_pointwise(C.byref(ly), g, eng.dt, B, C.c_void_p(ws.gates[l].data_ptr() + gs),
                                               C.c_void_p(ws.c[l].data_ptr() + cs), C.c_void_p(ws.c[l].data_ptr() + 2 * cs),
                                               C.c_void_p(ws.dh[l].data_ptr()), C.c_void_p(ws.dc[l].data_ptr()),
                                               C.c_void_p(ws.dG[l].data_ptr() + dgs), st) == 0
        run(f"pointwise{l}", pw, None, B * comp_px * ly.Ch16 * (9 * es + 16))   # gates+dG (ET), dh (ET), c_prev, c_new, dc r+w (f32)
    # fill dG for every t so that wgrad sees random data
    for l in range(len(cfgs)):
        ws.dG[l].view(torch.bfloat16 if es == 2 else torch.float32).normal_(std=0.05)
    for l, cfg in enumerate(cfgs):
        ly = eng.layers[l]
        dgs = B * halo_px * 4 * ly.Ch16 * es
        dx = ws.dh[l - 1].data_ptr() if l > 0 else None
        ncols = cfg.Ch + (cfg.Cx if l > 0 else 0)
        fl = 2.0 * B * H * W * cfg.k ** 2 * 4 * cfg.Ch * ncols

        def dg(ly=ly, dgs=dgs, dx=dx, l=l):
            assert lib.nint_conv_dgrad(C.byref(ly), g, eng.dt, B, C.c_void_p(ws.dG[l].data_ptr() + dgs),
                                       C.c_void_p(dx) if dx else None, C.c_void_p(ws.dh[l].data_ptr()), st) == 0
        run(f"dgrad{l}", dg, fl)
        gs, cs = B * comp_px * 4 * ly.Ch16 * es, B * comp_px * ly.Chp * 4

        def fused(ly=ly, dgs=dgs, dx=dx, l=l, gs=gs, cs=cs):      # dgrad(t+1) + pointwise backward(t) in one launch
            assert lib.nint_cell_bwd_fused(C.byref(ly), g, eng.dt, B, C.c_void_p(ws.dG[l].data_ptr() + dgs), C.c_void_p(dx) if dx else None,
                                           C.c_void_p(ws.gates[l].data_ptr() + gs), C.c_void_p(ws.c[l].data_ptr() + cs),
                                           C.c_void_p(ws.c[l].data_ptr() + 2 * cs), C.c_void_p(ws.dh[l].data_ptr()) if l < len(cfgs) - 1 else None,
                                           C.c_void_p(ws.dc[l].data_ptr()), C.c_void_p(ws.dG[l].data_ptr()), st) == 0
        run(f"fused{l}", fused, fl)
        dW = torch.empty(4 * cfg.Ch, cfg.Cx + cfg.Ch, cfg.k, cfg.k, device="cuda")
        db = torch.empty(4 * cfg.Ch, device="cuda")
        x_all = ws.xs.data_ptr() if l == 0 else ws.h[l - 1].data_ptr() + B * halo_px * ly.Cxp * es
        flw = 2.0 * T * B * H * W * cfg.k ** 2 * (cfg.Cx + cfg.Ch) * 4 * cfg.Ch

        def wg(ly=ly, x_all=x_all, dW=dW, db=db, l=l):
            assert lib.nint_conv_wgrad(C.byref(ly), g, eng.dt, T * B, C.c_void_p(ws.dG[l].data_ptr()), C.c_void_p(x_all),
                                       C.c_void_p(ws.h[l].data_ptr()), C.c_void_p(dW.data_ptr()), C.c_void_p(db.data_ptr()),
                                       C.c_void_p(eng.wg_partial.data_ptr()), eng.wg_partial.numel() * 4, eng.n_cu, st) == 0
        run(f"wgrad{l}", wg, flw)
    xs_pack = lambda: lib.nint_pack_btchw(C.c_void_p(X.data_ptr()), C.c_void_p(ws.xs.data_ptr()), B, T, args.C, ws.Cxp0, g, eng.dt, st)
    run("pack", xs_pack, None, X.numel() * 4 + B * T * comp_px * ws.Cxp0 * es)
    if args.C % 3 == 2 and (not only or only & {"preproc_slab", "preproc_nchw"}):
        # a-6: fuse + z-score + halo pad of a whole batch in one launch, from a record resident in HBM
        from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
        ds = SyntheticE33OMA_CRNN("train", padding=(H, W), in_channels=args.C, sequence_length=T, levels=(args.C - 2) // 3,
                                  n_steps=T + 2 * B + 4, grid=(H - 10, W - 10), device="cuda")
        idx = list(range(0, 2 * B, 2))
        sb, _ = ds.slab_batch(idx)
        alg = B * T * args.C * H * W
        run("preproc_slab", lambda: sb.fill_slab(eng, ws), None, alg * (4 + es))     # 4 B in + ET out per element
        run("preproc_nchw", lambda: ds.device_batch(idx), None, alg * 8)
    if not only or only & {"head_skill", "skill_plain", "head_fwd", "head_feedback", "head_feedback_bwd", "head_feedback_res", "head_feedback_bwd_res", "head_feedback_sel",
                           "head_feedback_sel1", "head_feedback_bwd_sel", "head_feedback_bwd_sel1", "head_loss", "head_loss_spec", "head_loss_spec3",
                           "input_noise", "noise_normal"}:
        # evaluation: the head on the last step's images + crop + the f64 skill sums in one pass (nint_head_skill_accum), and the
        # same sums from a prediction in memory (nint_skill_accum), one slot, cos-latitude row weights
        O, oy, ox = args.O, 5, 5
        Hc, Wc = H - 2 * oy, W - 2 * ox
        ly = eng.layers[-1]
        hw = torch.randn(O, ly.Ch, device="cuda") * 0.3
        hb = torch.randn(O, device="cuda")
        y = torch.randn(B, O, Hc, Wc, device="cuda")
        pix = torch.zeros(1, 5, O, Hc, Wc, dtype=torch.float64, device="cuda")
        smp = torch.empty(B, O, 8, dtype=torch.float64, device="cuda")
        nb = lib.nint_skill_scratch_bytes(B, O, Hc, Wc)
        scr = torch.empty(nb // 8, dtype=torch.float64, device="cuda")
        rw = torch.cos(torch.deg2rad(torch.linspace(-89, 89, Hc, dtype=torch.float64, device="cuda")))
        pred = torch.randn(B, O, H, W, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())

        def head_fwd():
            assert lib.nint_head_fwd(P(ws.h[-1]), T * B, B, ly.Ch, ly.Chp, O, P(hw), P(hb), P(pred), g, eng.dt, st) == 0

        def head_skill():
            assert lib.nint_head_skill_accum(P(ws.h[-1]), T * B, B, ly.Ch, ly.Chp, O, P(hw), P(hb), P(y), None, 1, P(rw), P(pix), P(smp),
                                             None, P(scr), nb, g, oy, ox, Hc, Wc, eng.dt, st) == 0

        def skill_plain():
            assert lib.nint_skill_accum(P(pred), P(y), None, 1, P(rw), P(pix), P(smp), P(scr), nb, B, O, H, W, oy, ox, Hc, Wc, st) == 0
        # training: head forward + crop + loss + d loss / d pred + dL/dh in one pass -- the entry the default step runs
        # (nint_head_loss_fused), and the configurable loss's general body (nint_head_loss_fused_spec) on the same data: with
        # spec (1, 1, 0), the same loss, and with all three terms plus output weights
        from nasa_niswan_amd import _lib as L
        dpl = torch.empty(B, O, H, W, device="cuda")
        dhl = torch.empty(B * comp_px * ly.Chp * es, dtype=torch.uint8, device="cuda")
        lsc = torch.zeros(L.NINT_LOSS_SPEC_SCRATCH_FLOATS, device="cuda")
        lst = torch.zeros(L.NINT_LOSS_STATS, dtype=torch.float64, device="cuda")
        owv = (0.5 + torch.rand(O, device="cuda")).float()
        sp110, sp111 = L.NintLossSpec(), L.NintLossSpec()
        sp110.mse, sp110.l1, sp110.huber, sp110.delta = 1.0, 1.0, 0.0, 1.0
        sp111.mse, sp111.l1, sp111.huber, sp111.delta = 1.0, 1.0, 1.0, 0.75
        sp111.ow, sp111.now, sp111.osum = owv.data_ptr(), O, float(owv.double().sum())

        def head_loss():
            assert lib.nint_head_loss_fused(P(ws.h[-1]), T * B, B, ly.Ch, ly.Chp, O, P(hw), P(hb), P(y), P(dpl), P(dhl), P(lsc), P(lst), g,
                                            oy, ox, Hc, Wc, eng.dt, st) == 0

        def head_loss_spec(sp=sp110):
            assert lib.nint_head_loss_fused_spec(P(ws.h[-1]), T * B, B, ly.Ch, ly.Chp, O, P(hw), P(hb), P(y), None, 0.0, C.byref(sp),
                                                 P(dpl), P(dhl), P(lsc), P(lst), g, oy, ox, Hc, Wc, eng.dt, st) == 0
        hl_bytes = B * comp_px * (2 * ly.Chp * es + O * 4) + y.numel() * 4      # h in, dh out, dpred out, the targets
        run("head_loss", head_loss, None, hl_bytes)
        run("head_loss_spec", head_loss_spec, None, hl_bytes)
        run("head_loss_spec3", lambda: head_loss_spec(sp111), None, hl_bytes)
        part = 2 * nb                                             # the per-wave partial rows, written and read back
        maps = 2 * pix.numel() * 8 + y.numel() * 4 + part         # pix read + written once per call, the targets
        run("head_fwd", head_fwd, None, B * comp_px * (ly.Chp * es + O * 4))
        if O <= args.C:
            # closed loop: the head of one step's images, rounded to ET, into the last O input channels of the next step's block
            # (nint_head_feedback; plain or folded as the engine lays the input out: --C 6 --O 1 is the folded reference stack)
            l0, kf = eng.layers[0], (cfgs[0].k if eng.cfgs[0].xfold else 0)

            def head_feedback():
                assert lib.nint_head_feedback(P(ws.h[-1]), B, B, ly.Ch, ly.Chp, O, P(hw), P(hb), P(ws.xs), B, args.C, l0.Cxp,
                                              args.C - O, kf, int(eng.lon_cyclic), g, eng.dt, st) == 0
            run("head_feedback", head_feedback, None, B * comp_px * (ly.Chp + max(kf, 1) * O) * es)
            # input noise on the same O channels of ALL T*B images of the slab: every fold copy of the span read and
            # written once; and the normals alone, f32 out
            nsig = torch.full((O,), 0.05, device="cuda")
            nz = torch.empty(T * B * O * ws.H * ws.W, device="cuda")

            def input_noise():
                assert lib.nint_input_noise(P(ws.xs), 0, B, T, args.C, l0.Cxp, args.C - O, O, P(nsig), kf, int(eng.lon_cyclic), 1, 2, 0, 0,
                                            g, eng.dt, st) == 0

            def noise_normal():
                assert lib.nint_noise_normal(P(nz), B, T, O, 1, 2, 0, 0, g, st) == 0
            run("input_noise", input_noise, None, 2 * T * B * comp_px * max(kf, 1) * O * es)
            run("noise_normal", noise_normal, None, nz.numel() * 4)
            # ... and its adjoint (nint_head_feedback_bwd): one step's dx block in (whole 64-byte lines: the fed span's lines), the
            # step's dpred images in and out, one dh block out
            fdx = torch.randn(B * comp_px * l0.Cxp, device="cuda").to(torch.bfloat16 if es == 2 else torch.float32)
            fdp = torch.randn(B, O, ws.H, ws.W, device="cuda")
            fdh = torch.empty(B * comp_px * ly.Chp * es, dtype=torch.uint8, device="cuda")
            c0 = args.C - O
            lines = (((max(kf, 1) - 1) * args.C + c0 + O) * es + 63) // 64 - c0 * es // 64      # 64-byte lines of a pixel's fed span

            def head_feedback_bwd():
                assert lib.nint_head_feedback_bwd(P(fdx), 0, P(fdp), 0, P(fdh), 0, B, ly.Ch, ly.Chp, O, P(hw), args.C, l0.Cxp, c0, kf,
                                                  int(eng.lon_cyclic), g, eng.dt, st) == 0
            fbb_bytes = lambda n_fed: comp_px * (n_fed * (lines * 64 + 2 * O * 4) + (B - n_fed) * O * 4 + B * ly.Chp * es)
            run("head_feedback_bwd", head_feedback_bwd, None, fbb_bytes(B))
            # the residual head: the same launches with the base (O more stored values per pixel, read from the
            # block before) and with the skip term (one more dpred image per fed image, read only)
            if hasattr(lib, "nint_head_feedback_res") and ws.T >= 2:
                fdp2 = torch.randn(2 * B, O, ws.H, ws.W, device="cuda")

                def head_feedback_res():
                    assert lib.nint_head_feedback_res(P(ws.h[-1]), B, B, ly.Ch, ly.Chp, O, P(hw), P(hb), P(ws.xs), B, args.C, l0.Cxp,
                                                      args.C - O, kf, int(eng.lon_cyclic), 0, None, g, eng.dt, st) == 0

                def head_feedback_bwd_res():
                    assert lib.nint_head_feedback_bwd_res(P(fdx), 0, P(fdp2), 0, P(fdh), 0, B, ly.Ch, ly.Chp, O, P(hw), args.C, l0.Cxp, c0,
                                                          kf, int(eng.lon_cyclic), B, None, g, eng.dt, st) == 0
                run("head_feedback_res", head_feedback_res, None, B * comp_px * ((ly.Chp + max(kf, 1) * O) * es + O * es))
                run("head_feedback_bwd_res", head_feedback_bwd_res, None, fbb_bytes(B) + B * comp_px * O * 4)
            # scheduled sampling: the masked instantiations under a half-set mask (every other image fed) and,
            # `1`, under an all-ones mask -- the same work as the unmasked rows above
            import numpy as np
            half, ones = np.arange(B, dtype=np.uint8) % 2, np.ones(B, np.uint8)
            nh = int(half.sum())

            def head_feedback_sel(m=half):
                assert lib.nint_head_feedback_sel(P(ws.h[-1]), B, B, ly.Ch, ly.Chp, O, P(hw), P(hb), P(ws.xs), B, args.C, l0.Cxp,
                                                  args.C - O, kf, int(eng.lon_cyclic), m.ctypes.data, g, eng.dt, st) == 0

            def head_feedback_bwd_sel(m=half):
                assert lib.nint_head_feedback_bwd_sel(P(fdx), 0, P(fdp), 0, P(fdh), 0, B, ly.Ch, ly.Chp, O, P(hw), args.C, l0.Cxp, c0, kf,
                                                      int(eng.lon_cyclic), m.ctypes.data, g, eng.dt, st) == 0
            if B <= 64:
                run("head_feedback_sel", head_feedback_sel, None, nh * comp_px * (ly.Chp + max(kf, 1) * O) * es)
                run("head_feedback_sel1", lambda: head_feedback_sel(ones), None, B * comp_px * (ly.Chp + max(kf, 1) * O) * es)
                run("head_feedback_bwd_sel", head_feedback_bwd_sel, None, fbb_bytes(nh))
                run("head_feedback_bwd_sel1", lambda: head_feedback_bwd_sel(ones), None, fbb_bytes(B))
        run("head_skill", head_skill, None, B * Hc * Wc * ly.Chp * es + maps)
        run("skill_plain", skill_plain, None, B * O * Hc * Wc * 4 + maps)
    tot = sum(ms * (T if not n.startswith(("wgrad", "pack", "preproc")) else 1) for n, ms in rows
              if n != "preproc_nchw" and not n.startswith(("head_", "skill_", "input_noise", "noise_")))      # (the evaluation and noise rows are no part of the default training step)
    print(f"sum over a step (T x per-step kernels + wgrad + pack): {tot:.2f} ms")


if __name__ == "__main__":
    main()
