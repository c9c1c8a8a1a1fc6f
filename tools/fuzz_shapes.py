#!/usr/bin/env python3
"""Random-shape screen of the whole sequence path against the CPU oracle (prediction, all gradients, input gradient):
layer counts 1-4, kernel sizes 1/3/5/7, ragged grids, thin and thick channel counts, B = 1-5, T = 1-4, both storage types,
the merged-grid launches forced on and off, both tile heights and the library's choice.
    python tools/fuzz_shapes.py [--n 40] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nasa_niswan_amd as pkg  # noqa: E402
from nasa_niswan_amd import engine  # noqa: E402
from oracle import convlstm_oracle as O  # noqa: E402
from oracle.stored_audit import stored_dG  # noqa: E402


def check_bias_grad(tag, name, db, dbo, dG_stored, dG_oracle, dtype):
    """The bias gradient is a sum that cancels (tests/test_gpu_bias_grad.py): bf16 mode is gated on its two factors instead of
    on a loose end-to-end figure -- (1) the REDUCTION: db equals the f32 column sum of the dG slab the kernels STORED (1e-5 of
    its max: a dropped or doubled tile shows here whatever the cancellation); (2) the SUMMANDS: the stored slab against the
    oracle's dG, elementwise (rel-L2 <= 3e-2, the gate of every other gradient).  What is then left between db and the oracle's
    db is a sum of per-element errors that are partly coherent (the bf16 rounding of one weight moves a whole column the same
    way), so its only honest bound is the coherent one, (3) |err| <= 3e-2 * ||dG_col||_1 -- measured up to 10 x the
    incoherent estimate 3e-2 * ||dG_col||_2 (fuzz seed 11 #9: 128 hidden channels, 7x7, 17 x 14 grid).  Returns the plain
    rel-L2 against the oracle for the log (worst seen: 7.7e-2, a B = 1, T = 1 top layer)."""
    db, dbo, go = db.double(), dbo.double(), dG_oracle.double()
    if dG_stored is not None:
        gs = dG_stored.double()
        colsum = gs.sum(dim=(0, 2, 3))
        e1 = float((db - colsum).abs().max() / (colsum.abs().max() + 1e-30))
        assert e1 <= 1e-5, (tag, name, "bias gradient is not the column sum of the stored dG slab", e1)
        e2 = float((gs - go).norm() / (go.norm() + 1e-30))
        assert e2 <= 3e-2, (tag, name, "stored dG slab against the oracle's dG", e2)
    bound = 3e-2 * go.abs().sum(dim=(0, 2, 3)) + 1e-30
    worst = float(((db - dbo).abs() / bound).max())
    assert worst <= 1.0, (tag, name, "bias gradient outside the coherent-error bound", worst)
    return float((db - dbo).norm() / (dbo.norm() + 1e-30))


def check_head_wgrad(tag, dW, dWo, h_stored, h_oracle, dpred):
    """The head's weight gradient dW[o][c] = sum_{b,y,x} dpred[b][o][y][x] * h[b][c][y][x] is, with a random-sign dpred, a sum
    that cancels like the bias gradients (seed 601 #125: 7,772 pixels, |dW| ~ 0.1-0.6, error 5.5e-2 relative under EVERY launch
    schedule while the prediction is 1.3e-3 off: profiles/r04_h_head_wgrad_case.txt).  Gated on its factors, as check_bias_grad:
    (1) the REDUCTION: dW equals the f64 sum over the h slab the forward pass STORED, to 1e-5 of the L1 norm of the summands;
    (2) the SUMMANDS: the stored h against the oracle's (rel-L2 <= 3e-2); (3) what is left against the oracle's dW within the
    coherent bound 3e-2 * sum |dpred| |h|.  Returns the plain rel-L2 for the log."""
    dW, dWo = dW.double().reshape(dWo.shape[0], -1), dWo.double().reshape(dWo.shape[0], -1)
    hs, ho, dp = h_stored.double(), h_oracle.double(), dpred.double()
    ref = torch.einsum("bohw,bchw->oc", dp, hs)
    l1s = torch.einsum("bohw,bchw->oc", dp.abs(), hs.abs()) + 1e-30
    e1 = float(((dW - ref).abs() / l1s).max())
    assert e1 <= 1e-5, (tag, "head weight gradient is not the sum over the stored h slab", e1)
    e2 = float((hs - ho).norm() / (ho.norm() + 1e-30))
    assert e2 <= 3e-2, (tag, "stored h of the top layer against the oracle's", e2)
    bound = 3e-2 * torch.einsum("bohw,bchw->oc", dp.abs(), ho.abs()) + 1e-30
    worst = float(((dW - dWo).abs() / bound).max())
    assert worst <= 1.0, (tag, "head weight gradient outside the coherent-error bound", worst)
    return float((dW - dWo).norm() / (dWo.norm() + 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--big", action="store_true", help="module mode on grids around the bench size (60-110 x 100-170, ragged), B = 1-3, T = 1-3")
    ap.add_argument("--wide", action="store_true", help="module mode on shapes the 8-wave 128-column weight-gradient kernel holds (bf16, hidden 32 / 64 / 128), the family forced on and off (nint_layer.wide = 2 / 1)")
    ap.add_argument("--dataset", action="store_true", help="the device preproc (z-score, level fusion, cyclic / reflect halo padding) of a resident synthetic record, as a batch tensor and through the model's input slab, against oracle/preproc_oracle.py instead")
    ap.add_argument("--cell", action="store_true", help="ConvLSTMCell(x, h, c) with a given state (forward, all five gradients) against oracle.cell_forward instead")
    ap.add_argument("--trainer", action="store_true", help="FusedTrainer.step (fused head / loss pass, flat gradient bucket) against oracle.train_step instead")
    ap.add_argument("--only", type=int, default=-1, help="plain module mode: replay the random stream up to this iteration and run it alone, printing every tensor's error")
    ap.add_argument("--force-wave", type=int, default=None, help="with --only: nint_seq.wave for the replayed case instead of the rotation's value")
    args = ap.parse_args()
    pkg.load_library()
    rng = np.random.default_rng(args.seed)
    worst = {"f32": 0.0, "bf16": 0.0}
    for it in range(args.n):
        L = int(rng.integers(1, 5))
        hidden = [int(rng.choice([4, 8, 16, 24, 32, 48, 64, 64, 128])) for _ in range(L)]
        ks = [int(rng.choice([1, 3, 3, 5, 5, 7])) for _ in range(L)]
        C = int(rng.choice([1, 3, 5, 7, 16, 33, 62, 100, 126]))
        out = int(rng.choice([1, 2, 5, 20, 20, 200]))
        B, T = int(rng.integers(1, 6)), int(rng.integers(1, 5))
        H, W = int(rng.integers(5, 40)), int(rng.integers(9, 70))
        if args.big:
            H, W, B, T = int(rng.integers(60, 111)), int(rng.integers(100, 171)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        dtype = "f32" if it % 2 == 0 else "bf16"
        engine.FORCE_WAVE = [None, 0, 1, 4, 2, 5, 4][it % 7]
        engine.FORCE_TILE_ROWS = [0, 0, 4, 8][it % 4]
        if args.wide:
            engine.FORCE_WIDE = [2, 2, 1][it % 3]
            dtype = "bf16"
            hidden = [int(rng.choice([32, 64, 64, 128])) if rng.random() < 0.8 else h_ for h_ in hidden]
            ks = [int(rng.choice([3, 3, 5, 7])) if k_ == 1 else k_ for k_ in ks]
            C = int(rng.choice([32, 62, 64, 126, 128])) if rng.random() < 0.7 else C
        if args.only >= 0:
            if it < args.only:                   # consume what the case would have drawn: X and the output weights
                rng.standard_normal((B, T, C, H, W)); rng.standard_normal((B, out, H, W))
                engine.FORCE_WAVE, engine.FORCE_TILE_ROWS, engine.FORCE_WIDE = None, 0, 0
                continue
            if it > args.only:
                break
            if args.force_wave is not None:
                engine.FORCE_WAVE = args.force_wave
        tag = f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={engine.FORCE_WAVE} rows={engine.FORCE_TILE_ROWS} wide={engine.FORCE_WIDE}"
        try:
            if args.dataset:
                from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
                from nasa_niswan_amd.engine import LayerCfg, SeqEngine
                from oracle import preproc_oracle as PO
                levels = int(rng.integers(1, 5))
                gh, gw = int(rng.integers(4, 24)), int(rng.integers(6, 48))
                # (px >= 1: with NO longitude halo the reference's `data[..., -0:]` slice returns the whole row and the output is
                # 2W wide -- dataset.py:67-80; `padding=None` is its way of not padding.  That accident is not reproduced.)
                py, px = int(rng.integers(0, min(6, gh - 1))), int(rng.integers(1, min(6, gw)))
                mode = ["reference", "reflect"][it % 2]
                seq = int(rng.integers(1, 5))
                Cin = 3 * levels + 2
                tag = f"#{it} dataset levels={levels} grid={gh}x{gw} pad=({py},{px}) {mode} T={seq} {dtype}"
                ds = SyntheticE33OMA_CRNN("train", padding=(gh + 2 * py, gw + 2 * px), in_channels=Cin, sequence_length=seq, levels=levels,
                                          n_steps=12 + seq, grid=(gh, gw), pad_mode=mode, device="cuda", seed=it)
                idx = [int(v) for v in rng.integers(0, len(ds), size=int(rng.integers(1, 4)))]
                X, y = ds.device_batch(idx)
                torch.cuda.synchronize()
                for b, ix in enumerate(idx):
                    (u, v, w_, pr, src), yr = ds.window(ix)
                    sq = (lambda a: a if levels > 1 else a[:, 0])
                    ref = PO.preproc_sample(sq(u), sq(v), sq(w_), pr, src, ds.X_mean, ds.X_std, (gh + 2 * py, gw + 2 * px), mode)
                    np.testing.assert_allclose(X[b].cpu().numpy(), ref, rtol=1e-6, atol=1e-6, err_msg=tag)
                # ... and straight into a model's input slab (folded or plain), then unpacked again
                k0 = int(rng.choice([3, 5]))
                eng = SeqEngine([LayerCfg(Cin, 16, k0)], dtype, "cuda")
                ws = eng.acquire(len(idx), seq, gh + 2 * py, gw + 2 * px, False, False)
                sb = ds.slab_batch(idx)[0]
                eng.pack_input(ws, sb)
                ws2 = eng.acquire(len(idx), seq, gh + 2 * py, gw + 2 * px, False, False)
                eng.pack_input(ws2, X)
                torch.cuda.synchronize()
                assert torch.equal(ws.xs, ws2.xs), (tag, "slab path differs from preproc -> pack", bool(eng.cfgs[0].xfold))
                print(f"ok   {tag} k0={k0} fold={bool(eng.cfgs[0].xfold)}", flush=True)
                continue
            if args.cell:
                Ch, k = hidden[0], ks[0]
                has_bias = bool(it % 5)
                tag = f"#{it} cell Cx={C} Ch={Ch} k={k} B={B} {H}x{W} {dtype} bias={has_bias} rows={engine.FORCE_TILE_ROWS}"
                cell = pkg.ConvLSTMCell(C, Ch, k, bias=has_bias, compute_dtype=dtype).cuda()
                Wt = (torch.from_numpy(rng.standard_normal((4 * Ch, C + Ch, k, k)).astype(np.float32)) / np.sqrt((C + Ch) * k * k))
                bt = torch.from_numpy(rng.standard_normal(4 * Ch).astype(np.float32)) * 0.2 if has_bias else None
                with torch.no_grad():
                    cell.conv.weight.copy_(Wt)
                    if has_bias:
                        cell.conv.bias.copy_(bt)
                mk = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
                x, h, c = mk(B, C, H, W), mk(B, Ch, H, W) * 0.5, mk(B, Ch, H, W)
                gh, gc = mk(B, Ch, H, W), mk(B, Ch, H, W)
                xd, hd, cd = (t.cuda().requires_grad_(True) for t in (x, h, c))
                h1, c1 = cell(xd, (hd, cd))
                ((h1 * gh.cuda()).sum() + (c1 * gc.cuda()).sum()).backward()
                torch.cuda.synchronize()
                xo, ho, co = (t.clone().requires_grad_(True) for t in (x, h, c))
                Wo = Wt.clone().requires_grad_(True)
                bo = bt.clone().requires_grad_(True) if has_bias else None
                pre = []
                h1o, c1o = O.cell_forward(xo, ho, co, Wo, bo, pre)
                ((h1o * gh).sum() + (c1o * gc).sum()).backward()
                res = {"h1": (h1.detach().cpu(), h1o.detach()), "c1": (c1.detach().cpu(), c1o.detach()), "dx": (xd.grad.cpu(), xo.grad),
                       "dh": (hd.grad.cpu(), ho.grad), "dc": (cd.grad.cpu(), co.grad), "dW": (cell.conv.weight.grad.cpu(), Wo.grad)}
                if has_bias:
                    res["db.bias"] = (cell.conv.bias.grad.cpu(), bo.grad)
                w = 0.0
                for k2, (a, b) in res.items():
                    a, b = a.double(), b.double()
                    assert torch.isfinite(a).all(), (tag, k2)
                    if dtype == "bf16" and k2.endswith("bias"):
                        eng = cell._engine(xd.device)
                        (ws,) = eng.pool[(B, 1, H, W, True, True)]
                        check_bias_grad(tag, k2, a, b, stored_dG(eng, ws, 0).cpu(), pre[0].grad, dtype)
                        continue
                    e = float((a - b).abs().max() / (b.abs().max() + 1e-30)) if dtype == "f32" else float((a - b).norm() / (b.norm() + 1e-30))
                    assert e <= (1e-3 if dtype == "f32" else 3e-2), (tag, k2, e)
                    w = max(w, e)
                worst[dtype] = max(worst[dtype], w)
                print(f"ok   {tag}  worst {w:.2e}", flush=True)
                continue
            if args.trainer:
                from nasa_niswan_amd.trainer import FusedTrainer
                hy, hx = int(rng.integers(0, min(4, (H - 2) // 2 + 1))), int(rng.integers(0, min(4, (W - 2) // 2 + 1)))   # (cropped grid >= 2 x 2)
                out, B = max(out, 2), max(B, 2)          # (keeps the reference's .squeeze() a no-op)
                params = O.synth_params(C, hidden, ks, L, out_channels=out, seed=it)
                X = torch.from_numpy(rng.standard_normal((B, T, C, H, W)).astype(np.float32))
                y = torch.from_numpy(rng.standard_normal((B, out, H - 2 * hy, W - 2 * hx)).astype(np.float32))
                net = pkg.ConvLSTM(C, hidden, ks, L, out_channels=out, compute_dtype=dtype).cuda()
                net.load_state_dict(params)
                tr = FusedTrainer(net, lr=1e-3, halo=(hy, hx))
                loss = float(tr.step(X.cuda(), y.cuda()))
                torch.cuda.synchronize()
                _, _, lo, _, grads = O.train_step(params, None, X, y, lr=1e-3, halo=(hy, hx))
                tol_l = 2e-6 if dtype == "f32" else 2e-2
                assert abs(loss - lo) <= tol_l * abs(lo), (tag, "loss", loss, lo)
                w = abs(loss - lo) / abs(lo)
                for i, (k, p) in enumerate(net.named_parameters()):
                    a, b = tr.flat.grad_view(i).detach().cpu().double(), grads[k].double()
                    assert torch.isfinite(a).all(), (tag, k)
                    e = float((a - b).abs().max() / (b.abs().max() + 1e-30)) if dtype == "f32" else float((a - b).norm() / (b.norm() + 1e-30))
                    assert e <= (1e-3 if dtype == "f32" else 3e-2), (tag, k, e)
                    w = max(w, e)
                worst[dtype] = max(worst[dtype], w)
                print(f"ok   {tag} halo=({hy},{hx}) trainer  worst {w:.2e}", flush=True)
                continue
            params = O.synth_params(C, hidden, ks, L, out_channels=out, seed=it)
            X = torch.from_numpy(rng.standard_normal((B, T, C, H, W)).astype(np.float32))
            wgt = torch.from_numpy(rng.standard_normal((B, out, H, W)).astype(np.float32))
            net = pkg.ConvLSTM(C, hidden, ks, L, out_channels=out, compute_dtype=dtype).cuda()
            net.load_state_dict(params)
            Xd = X.cuda().requires_grad_(True)
            pred = net(Xd)
            (pred * wgt.cuda()).sum().backward()
            torch.cuda.synchronize()
            leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            Xo = X.clone().requires_grad_(True)
            pre = {}
            po, hso, _ = O.convlstm_forward(Xo, leaf, return_states=True, preact=pre)
            (po * wgt).sum().backward()
            res = {"pred": (pred.detach().cpu(), po.detach()), "dX": (Xd.grad.cpu(), Xo.grad)}
            for k, p in net.named_parameters():
                res["grad." + k] = (p.grad.cpu(), leaf[k].grad)
            w = 0.0
            for k, (a, b) in res.items():
                a, b = a.double(), b.double()
                assert torch.isfinite(a).all(), (tag, k)
                if dtype == "f32":
                    e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
                    assert e <= 1e-3, (tag, k, e)
                elif k.startswith("grad.layers.") and k.endswith("bias"):
                    # sums that cancel: gated on their two factors, not on the end-to-end figure (check_bias_grad)
                    l = int(k.split(".")[2])
                    eng = net._engine(Xd.device)
                    (ws,) = eng.pool[(B, T, H, W, True, False)]
                    check_bias_grad(tag, k, a, b, stored_dG(eng, ws, l).cpu(), torch.cat([pre[(l, t)].grad for t in range(T)]), dtype)
                    continue
                elif k == "grad.conv.weight":
                    # the head's weight gradient: a sum over pixels with random signs (check_head_wgrad)
                    eng = net._engine(Xd.device)
                    (ws,) = eng.pool[(B, T, H, W, True, False)]
                    e = check_head_wgrad(tag, a, b, eng.h_last(ws, L - 1).cpu(), hso[-1].detach(), wgt)
                    if args.only >= 0:
                        print(f"     {k}: rel-L2 {e:.3e} (gated on its factors)", flush=True)
                else:
                    e = float((a - b).norm() / (b.norm() + 1e-30))
                    if args.only >= 0:
                        print(f"     {k}: rel-L2 {e:.3e}  |ref| {float(b.norm()):.3e}", flush=True)
                        if k == "grad.conv.weight":
                            print("       hip   ", a.flatten().tolist()); print("       oracle", b.flatten().tolist())
                    assert e <= 3e-2 or args.only >= 0, (tag, k, e)
                w = max(w, e)
            worst[dtype] = max(worst[dtype], w)
            print(f"ok   {tag}  worst {w:.2e}", flush=True)
        finally:
            engine.FORCE_WAVE, engine.FORCE_TILE_ROWS, engine.FORCE_WIDE = None, 0, 0
    print(f"{args.n} shapes ok; worst f32 max-rel {worst['f32']:.2e}, worst bf16 rel-L2 {worst['bf16']:.2e}")


if __name__ == "__main__":
    main()
