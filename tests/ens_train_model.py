"""CPU model of ENSEMBLE TRAINING (TEST INFRASTRUCTURE ONLY): the closed loop of tests/rollout_model.py (and, with
``residual``, of tests/residual_model.py) with an additive noise tensor on every fed value,

    for every step t >= free_from:   v = p_{t-1} + add[t];   x[:, t, C-O:] = v + (round_ET(v) - v).detach()

``add`` (T, B, O, H, W) is a constant -- sigma[o] * z, the product rounded to f32 as the device forms it -- so the derivative of
the stored value with respect to p is 1 under the straight-through rule, and the roll-out backward of the noise-free window is
this window's adjoint.  The B lanes are N samples x M members, lane n*M + m; ``crps`` is the almost-fair CRPS over the member
lanes in torch (autograd: sign gradients, 0 at ties)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

import closed_loop_model as CLM
import cyclic_model as CM
import noise_model as NM


def forward(x, params, free_from: int, cyclic: bool = False, storage: Optional[str] = "f32", add=None, residual: bool = False):
    """x (B,T,C,H,W) -> dict(pred, seq (B, T*O, H, W), x_fed): zero initial state"""
    L = CM.num_layers_of(params)
    B, T, C, H, W = x.shape
    w, b = params["conv.weight"], params["conv.bias"]
    O = w.shape[0]
    s = int(free_from)
    if s < 1:
        raise ValueError("step 0 is never fed")
    hs = [torch.zeros(B, params[f"layers.{i}.conv.bias"].shape[0] // 4, H, W, dtype=x.dtype) for i in range(L)]
    cs = [torch.zeros_like(h) for h in hs]
    outs, seen = [], []
    for t in range(T):
        x_t = x[:, t]
        if t >= s:
            v = outs[-1] if add is None else outs[-1] + add[t].to(x.dtype)
            x_t = torch.cat([x_t[:, :C - O], v + (CLM.round_et(v, storage) - v).detach()], dim=1)
        seen.append(x_t)
        inp = x_t
        for i in range(L):
            hs[i], cs[i] = CM.cell_forward(inp, hs[i], cs[i], params[f"layers.{i}.conv.weight"], params[f"layers.{i}.conv.bias"], cyclic)
            inp = hs[i]
        p = F.conv2d(hs[-1], w, b)
        outs.append(p + x_t[:, C - O:] if residual else p)
    return dict(pred=outs[-1], seq=torch.cat(outs, dim=1), x_fed=torch.stack(seen, dim=1))


def feedback_add(sig, B, T, O, H, W, seed, draw, lane0=0):
    """(T, B, O, H, W) f32: fl32(sigma[o] * z) with z the f64 model of nint_noise_normal rounded to f32 (tests/noise_model.py)"""
    z = NM.z_images(B, T, O, H, W, seed=seed, draw=draw, step0=0, lane0=lane0).astype(np.float32).reshape(T, B, O, H, W)
    sg = np.asarray(sig, np.float32).reshape(1, 1, O, 1, 1)
    return torch.from_numpy((sg * z).astype(np.float32))


def _cells(seq, y, M, halo, every_step, O, step_w, out_w=None):
    """members x (N, M, T', O, Hc, Wc), targets t (N, 1, T', O, Hc, Wc) and the weights (T', O) of the listed steps and outputs"""
    B, TO, H, W = seq.shape
    T, N = TO // O, B // M
    Hc, Wc = y.shape[-2], y.shape[-1]
    x = seq.view(N, M, T, O, H, W)[..., halo[0]:halo[0] + Hc, halo[1]:halo[1] + Wc]
    if every_step:
        t = y.view(N, 1, T, O, Hc, Wc)
        sw = torch.ones(T, dtype=seq.dtype) if step_w is None else torch.as_tensor(step_w, dtype=torch.float32).to(seq.dtype)
    else:
        x, t, sw = x[:, :, T - 1:], y.view(N, 1, 1, O, Hc, Wc), torch.ones(1, dtype=seq.dtype)
    ow = torch.ones(O, dtype=seq.dtype) if out_w is None else torch.as_tensor(out_w, dtype=torch.float32).to(seq.dtype)
    return x, t, sw.view(-1, 1) * ow.view(1, -1)


def crps(seq, y, M, alpha, halo, every_step, O, step_w=None, out_w=None):
    """seq (B, T*O, H, W) with lanes n*M + m, y (N, [T,] O, Hc, Wc): the almost-fair CRPS, the mean over the listed cells weighted
    by the step's weight (a step of weight 0 is out)"""
    x, t, sw = _cells(seq, y, M, halo, every_step, O, step_w, out_w)
    A = (x - t).abs().sum(dim=1)
    D = sum((x[:, i] - x[:, j]).abs() for i in range(M) for j in range(i + 1, M))
    kp = (M - 1.0 + alpha) / (M * M * (M - 1.0))
    per = A / M - kp * D                                                   # (N, T', O, Hc, Wc)
    w = sw.view(1, sw.shape[0], O, 1, 1).expand_as(per)
    live = w != 0
    return (per[live] * w[live]).sum() / w[live].sum()


def smallest_gap(seq, y, M, halo, every_step, O, step_w=None, out_w=None):
    """min over the cells under a non-zero weight of (gap - 2 * (1e-4 * |x| + 1e-5)) for every |x_i - t| and |x_i - x_j|:
    positive = no sign can flip inside twice the f32 output tolerance.  Returns (that margin, the smallest gap itself)."""
    x, t, sw = _cells(seq.detach(), y, M, halo, every_step, O, step_w, out_w)
    keep = (sw != 0).view(1, 1, sw.shape[0], O, 1, 1).expand_as(x)
    big = torch.full_like(x, float("inf"))
    tol = 2 * (1e-4 * x.abs() + 1e-5)
    first = torch.where(keep, (x - t).abs(), big)
    margins, gaps = [(first - tol).min()], [first.min()]
    for i in range(M):
        for j in range(i + 1, M):
            g = torch.where(keep[:, i], (x[:, i] - x[:, j]).abs(), big[:, i])
            margins.append((g - torch.maximum(tol[:, i], tol[:, j])).min())
            gaps.append(g.min())
    return float(min(margins)), float(min(gaps))


def replicate(Xs, M):
    """(N, ...) -> (N*M, ...): lane n*M + m holds sample n"""
    return Xs.repeat_interleave(M, dim=0)
