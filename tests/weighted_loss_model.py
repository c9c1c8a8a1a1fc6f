"""Host-side f64 model of the weighted crop + MSE + L1 loss (include/nint.h, the ``_weighted`` entries) and the weight maps
the tests use (TEST INFRASTRUCTURE ONLY; numpy / torch-CPU).  Same conventions as ``oracle/small_audit.py``, whose
comparators (``ratio``, ``check_stats``, ``check_loss_scalar``) take the dicts built here.

The arithmetic, per crop cell with ``w = wgt[cy][cx]`` and ``d = p - y`` formed in f32:
    loss  = (sum w d^2) / cnt + (sum w |d|) / cnt,      cnt = N * O * wsum,  wsum = the f64 sum of the f32 map
    dpred = (float)(((2.0 * d + sgn(d)) * (1.0 / cnt)) * (double)w),  +0 outside the crop and where w == 0
    a cell with w == 0 enters nothing (its target may be NaN)
    stats [0..4] += sum w d^2, sum w |d|, sum w y, sum w y^2, cnt; [5] += loss; [6] += weighted R2; [7] += 1"""
from __future__ import annotations

import numpy as np
import torch

from oracle import small_audit as SM


def wmap(Hc: int, Wc: int) -> np.ndarray:
    """The tests' weight map, f32 (Hc, Wc): cos(latitude) of Hc cell-centred rows times 1 + 0.25 sin(cx) (it varies along a row too);
    the first row and the last column are zero (the crop's edges: a crop-versus-grid coordinate slip shows), and from 8 x 8
    up an interior block [3:6, 4:9] is zero too.  At least half of the cells keep a weight: no case passes because most of it
    was masked away."""
    lat = -90.0 + (np.arange(Hc) + 0.5) * (180.0 / Hc)
    w = np.cos(np.deg2rad(lat))[:, None] * (1.0 + 0.25 * np.sin(np.arange(Wc, dtype=np.float64)))[None, :]
    w[0, :] = 0.0
    w[:, -1] = 0.0
    if Hc >= 8 and Wc >= 8:
        w[3:6, 4:9] = 0.0
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert (w >= 0).all() and 2 * int((w > 0).sum()) >= w.size, (Hc, Wc, int((w > 0).sum()))
    return w


def wsum_of(w) -> float:
    """what the caller passes by value: the f64 sum of the map as stored in f32"""
    return float(np.asarray(w, np.float32).astype(np.float64).sum())


def _r2w(s0: float, y64, wb, cnt: float):
    """sklearn.metrics.r2_score(y, p, sample_weight=w) from the weighted residual sum s0; the constant-target convention
    of small_audit._r2 on the cells that carry a weight.  Returns (r2, ss_tot about the weighted mean or None)."""
    live = wb > 0
    yl = y64[live]
    if yl.min() == yl.max():
        return (1.0 if s0 == 0.0 else 0.0), None
    mean = float(np.sum(np.where(live, wb * y64, 0.0))) / cnt
    ss = float(np.sum(np.where(live, wb * (y64 - mean) ** 2, 0.0)))
    return 1.0 - s0 / ss, ss


def _sums(d64, y64, wb, cnt: float):
    """the loss() style dict from d (f64, crop), y (f64, crop) and the broadcast weights.  Cells with w == 0 are taken out
    with np.where: NaN targets there must not reach a sum."""
    live = wb > 0
    z = lambda a: np.where(live, a, 0.0)
    with np.errstate(invalid="ignore"):
        s0, s1 = float(np.sum(z(wb * d64 * d64))), float(np.sum(z(wb * np.abs(d64))))
        s2, s3 = float(np.sum(z(wb * y64))), float(np.sum(z(wb * y64 * y64)))
        S2 = float(np.sum(z(wb * np.abs(y64))))
        r2, ss = _r2w(s0, np.where(live, y64, 0.0), wb, cnt)
    r2_tol = 0.0
    if ss is not None:
        # small_audit.loss's derivation with the weighted sums in place of the plain ones
        delta = SM.SUM_RTOL * (s3 + 2 * S2 * S2 / cnt) + 2.0 ** -51 * (s3 + S2 * S2 / cnt)
        q = s0 / ss
        r2_tol = q * (SM.SUM_RTOL + delta / ss) / (1.0 - delta / ss) + 2.0 ** -51 * (1.0 + q)
    return {"sums": np.array([s0, s1, s2, s3, cnt]), "abs": np.array([s0, s1, S2, s3, cnt]), "loss": s0 / cnt + s1 / cnt,
            "r2": r2, "r2_tol": r2_tol}


def loss(pred, y, w, oy: int, ox: int):
    """The weighted loss of pred (N, O, H, W) f32 cropped to y (N, O, Hc, Wc) f32 at (oy, ox) with the map w (Hc, Wc) f32:
    small_audit.loss's dict (dpred f32, sums, abs, loss, r2, r2_tol), every sum in f64 from d formed in f32."""
    pred, y, w = np.asarray(pred, np.float32), np.asarray(y, np.float32), np.asarray(w, np.float32)
    N, O, H, W = pred.shape
    Hc, Wc = y.shape[2:]
    assert w.shape == (Hc, Wc)
    with np.errstate(invalid="ignore"):
        d = pred[:, :, oy:oy + Hc, ox:ox + Wc] - y                  # f32, the definition
    d64, y64 = d.astype(np.float64), y.astype(np.float64)
    wb = np.broadcast_to(w.astype(np.float64), d64.shape)
    cnt = float(N * O) * wsum_of(w)
    out = _sums(d64, y64, wb, cnt)
    inv = 1.0 / cnt
    dp = np.zeros(pred.shape, np.float32)
    with np.errstate(invalid="ignore"):
        g = ((2.0 * d64 + np.sign(d64)) * inv) * wb
    dp[:, :, oy:oy + Hc, ox:ox + Wc] = np.where(wb > 0, g, 0.0).astype(np.float32)
    out["dpred"] = dp
    return out


def loss_torch(pred, y, w, oy: int, ox: int):
    """the same loss as a torch expression (any dtype, autograd): what the oracle fit loop minimises"""
    Hc, Wc = y.shape[-2], y.shape[-1]
    wt = torch.as_tensor(np.asarray(w, np.float32)).to(pred.dtype)
    d = pred[..., oy:oy + Hc, ox:ox + Wc] - y.reshape(pred.shape[:-2] + (Hc, Wc))
    live = wt > 0
    d = torch.where(live, d, torch.zeros_like(d))                   # a masked cell enters nothing, NaN target or not
    cnt = float(d.numel() // (Hc * Wc)) * wsum_of(w)
    return (wt * d * d).sum() / cnt + (wt * d.abs()).sum() / cnt


def r2_weighted(y, p, w) -> float:
    """sklearn's r2_score(y, p, sample_weight=w) on (..., Hc, Wc) arrays, spelled out in f64"""
    y, p = np.asarray(y, np.float64), np.asarray(p, np.float64)
    wb = np.broadcast_to(np.asarray(w, np.float32).astype(np.float64), y.shape)
    mean = np.sum(wb * y) / np.sum(wb)
    return float(1.0 - np.sum(wb * (y - p) ** 2) / np.sum(wb * (y - mean) ** 2))


def head_loss_fused(h, wh, b, y, w, oy: int, ox: int):
    """The fused head + weighted loss pass in f64 from the stored h (N, H, W, Ch): pred = wh . h + b, d = pred - y on the
    crop, dpred = (2 d + sign d) w / cnt (0 outside the crop and under a zero weight), dh = wh^T dpred (N, H, W, Ch).
    Returns (dpred, dh, loss)."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    w = np.asarray(w, np.float32)
    pred, _ = SM.head_fwd(h, wh, b)
    N, O, H, W = pred.shape
    Hc, Wc = y64.shape[2:]
    cnt = float(N * O) * wsum_of(w)
    crop = (slice(None), slice(None), slice(oy, oy + Hc), slice(ox, ox + Wc))
    wb = np.broadcast_to(w.astype(np.float64), y64.shape)
    with np.errstate(invalid="ignore"):
        d = np.where(wb > 0, pred[crop] - y64, 0.0)
    dp = np.zeros_like(pred)
    dp[crop] = (2.0 * d + np.sign(d)) * wb / cnt
    dh = np.einsum("noyx,oc->nyxc", dp, np.asarray(wh, np.float64))
    return dp, dh, float(np.sum(wb * d * d)) / cnt + float(np.sum(wb * np.abs(d))) / cnt
