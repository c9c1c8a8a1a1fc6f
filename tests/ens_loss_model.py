"""The model of nint_ens_loss (include/nint.h): numpy f64 in the kernel's documented order, python `fractions`
for the exact sums.  No GPU, no library.

Per cell (sample n, output o, crop pixel) with Wd = (double)q * (double)w != 0, x_i = (double)member i, t = (double)target:
    S = ((0 + x_0) + x_1) + ...          A = sum_i |x_i - t|          V = sum_i (M*x_i - S)^2         (i ascending, from 0.0)
    D = sum_{i<j} |x_i - x_j|            ((i, j) lexicographic, from 0.0)           m = S / M
    sgn(d) = 1 (d > 0), -1 (d < 0), d otherwise (0 stays 0, NaN stays NaN)
    R_i = sum_{j != i} sgn(x_i - x_j)    (j ascending, from 0.0)
    dpred_i = f32(((sgn(x_i - t) / M - kp * R_i) * (1 / cnt)) * Wd)
    terms: Wd*A, Wd*D, Wd*V, Wd*(m-t)^2, Wd*|m-t|, Wd*t, Wd*t^2  -> SA, SD, SV, S2, S1, Sy, Syy over the call
    loss = (SA / M - kp * SD) / cnt,     kp = (M - 1 + alpha) / (M^2 (M - 1))
numpy's elementwise f64 operations are single IEEE operations, so `cells` has the kernel's bits on any data; the sums over the
call are taken in another order than the kernel's trees and are equal only where they are exact (integers, dyadic weights)."""
from fractions import Fraction

import numpy as np

import ensemble_model as EM

TERMS = ("SA", "SD", "SV", "S2", "S1", "Sy", "Syy")


def kp_of(M, alpha):
    dM = float(M)
    return (dM - 1.0 + float(alpha)) / (dM * dM * (dM - 1.0))


def sgn(d):
    return np.where(d > 0, 1.0, np.where(d < 0, -1.0, d))


def weights(N, O, Hc, Wc, wgt=None, ow=None, ow_row=None):
    """(q (N, O) f32, w (Hc, Wc) f32, cnt f64): cnt = (sum of q as stored over samples and outputs) * wsum"""
    w = np.ones((Hc, Wc), np.float32) if wgt is None else np.asarray(wgt, np.float32)
    if ow is None:
        q = np.ones((N, O), np.float32)
    else:
        rows = np.zeros(N, np.int64) if ow_row is None else np.asarray(ow_row, np.int64)
        q = np.asarray(ow, np.float32)[rows]
    cnt = float(q.astype(np.float64).sum()) * float(w.astype(np.float64).sum())
    return q, w, cnt


def pairs(x, t):
    """the part of a cell that depends on neither alpha nor the weights: S, A, V, D, m (N, O, Hc, Wc) and R (N, M, O, Hc, Wc), f64"""
    x = np.asarray(x, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    M = x.shape[1]
    dM = float(M)
    with np.errstate(invalid="ignore"):
        S, A = np.zeros_like(t), np.zeros_like(t)
        for i in range(M):
            S = S + x[:, i]
            A = A + np.abs(x[:, i] - t)
        V, D = np.zeros_like(t), np.zeros_like(t)
        R = np.zeros_like(x)
        for i in range(M):
            dv = dM * x[:, i] - S
            V = V + dv * dv
            Ri = np.zeros_like(t)
            for j in range(M):
                if j == i:
                    continue
                d = x[:, i] - x[:, j]
                Ri = Ri + sgn(d)
                if j > i:
                    D = D + np.abs(d)
            R[:, i] = Ri
        return {"x": x, "t": t, "S": S, "A": A, "V": V, "D": D, "R": R, "m": S / dM}


def pairs_int(x, t, lo=-8, hi=8):
    """pairs() for integer-valued members in [lo, hi] (ensemble_model.int_data), where every sum is exact in any order and R_i
    is a count: by a histogram of the members' values instead of the M^2 loop (M = 64 with many samples).  Same keys, same bits."""
    x = np.asarray(x, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    M = x.shape[1]
    assert (x == np.rint(x)).all() and x.min() >= lo and x.max() <= hi
    vals = np.arange(lo, hi + 1, dtype=np.float64)
    cnt = np.stack([(x == v).sum(axis=1) for v in vals]).astype(np.float64)            # (nv, N, O, Hc, Wc)
    below = np.cumsum(cnt, axis=0) - cnt                                                # members < v
    above = float(M) - below - cnt
    diff = below - above                                                                # R of a member whose value is v
    idx = (x - lo).astype(np.int64)
    R = np.stack([np.take_along_axis(diff, idx[:, i][None], axis=0)[0] for i in range(M)], axis=1)
    S = x.sum(axis=1)
    A = np.abs(x - t[:, None]).sum(axis=1)
    V = ((float(M) * x - S[:, None]) ** 2).sum(axis=1)
    D = np.zeros_like(t)
    for a in range(len(vals)):
        for b in range(a + 1, len(vals)):
            D = D + cnt[a] * cnt[b] * (vals[b] - vals[a])
    return {"x": x, "t": t, "S": S, "A": A, "V": V, "D": D, "R": R + 0.0, "m": S / float(M)}


def cells(x, t, alpha, q, w, cnt, pre=None):
    """x (N, M, O, Hc, Wc) f32 members on the crop, t (N, O, Hc, Wc) f32, q (N, O), w (Hc, Wc) -> dict: dpred (N, M, O, Hc, Wc)
    f32 (+0 where Wd == 0), terms (7, N, O, Hc, Wc) f64 (0 where Wd == 0), live (N, O, Hc, Wc) bool.  ``pre``: pairs(x, t)."""
    p = pairs(x, t) if pre is None else pre
    x, t = p["x"], p["t"]
    M = x.shape[1]
    dM, kp, inv_n = float(M), kp_of(M, alpha), 1.0 / cnt
    Wd = q.astype(np.float64)[:, :, None, None] * w.astype(np.float64)[None, None]
    live = Wd != 0
    with np.errstate(invalid="ignore"):
        gi = ((sgn(x - t[:, None]) / dM - kp * p["R"]) * inv_n) * Wd[:, None]
        g = np.where(live[:, None], gi, 0.0).astype(np.float32)
        e = p["m"] - t
        terms = np.stack([Wd * p["A"], Wd * p["D"], Wd * p["V"], Wd * (e * e), Wd * np.abs(e), Wd * t, Wd * (t * t)])
        terms = np.where(live[None], terms, 0.0)
    return {"dpred": g, "terms": terms, "live": live, "Wd": Wd}


def finish(tot, M, alpha, cnt, stats_before=None, ens_before=None):
    """the closing launch from the seven totals: loss (f64), stats (8) and ens_out (4), grown from what was there"""
    SA, SD, SV, S2, S1, Sy, Syy = (float(v) for v in tot)
    dM, kp = float(M), kp_of(M, alpha)
    with np.errstate(invalid="ignore"):
        loss = (np.float64(SA) / dM - kp * np.float64(SD)) / cnt
        ss_tot = np.float64(Syy) - np.float64(Sy) * np.float64(Sy) / cnt
        r2 = 1.0 - np.float64(S2) / ss_tot if ss_tot > 0.0 else (1.0 if S2 == 0.0 else 0.0)
    stats = np.zeros(8) if stats_before is None else np.array(stats_before, np.float64)
    ens = np.zeros(4) if ens_before is None else np.array(ens_before, np.float64)
    stats = stats + np.array([S2, S1, Sy, Syy, cnt, loss, r2, 1.0])
    ens = ens + np.array([SA, SD, SV, cnt])
    return float(loss), stats, ens


def run(x, t, alpha, wgt=None, ow=None, ow_row=None, stats_before=None, ens_before=None, pre=None):
    """the whole entry on crop data; the totals are numpy sums (exact data only).  ``pre``: pairs(x, t), to share among alphas"""
    N, M, O, Hc, Wc = np.asarray(x).shape
    q, w, cnt = weights(N, O, Hc, Wc, wgt, ow, ow_row)
    c = cells(x, t, alpha, q, w, cnt, pre)
    with np.errstate(invalid="ignore"):
        tot = c["terms"].reshape(7, -1).sum(axis=1)
    loss, stats, ens = finish(tot, M, alpha, cnt, stats_before, ens_before)
    return dict(c, cnt=cnt, tot=tot, loss=loss, loss_f32=np.float32(loss), stats=stats, ens=ens)


def full_images(dcrop, H, W, oy, ox):
    """(N, M, O, Hc, Wc) -> (N, M, O, H, W): +0 outside the crop"""
    N, M, O, Hc, Wc = dcrop.shape
    out = np.zeros((N, M, O, H, W), np.float32)
    out[:, :, :, oy:oy + Hc, ox:ox + Wc] = dcrop
    return out


def loss_value(x, t, alpha, q, w, cnt):
    """the loss alone, in plain f64 (for finite differences): x (N, M, O, Hc, Wc) f64"""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    M = x.shape[1]
    Wd = q.astype(np.float64)[:, :, None, None] * w.astype(np.float64)[None, None]
    A = np.abs(x - t[:, None]).sum(axis=1)
    D = sum(np.abs(x[:, i] - x[:, j]) for i in range(M) for j in range(i + 1, M))
    tt = np.where(Wd != 0, 1.0, 0.0)
    return float(((Wd * A * tt).sum() / M - kp_of(M, alpha) * (Wd * D * tt).sum()) / cnt)


# ------------------------------------------------------------------------------ exact totals and the any-order bound
def exact_totals(x, t, q, w):
    """(values, bounds-free magnitudes, roundings inside one term) of the seven totals over live cells, as Fractions.
    Roundings inside a term, beyond ensemble_model.exact_cell's counts for A (M), D (P) and V (3 M): the product with Wd is one
    more; m = S^ / M carries M - 1 additions and the division, m - t one, the square one: (m-t)^2 -> 2 (M + 1) + 1,
    |m-t| -> M + 1; t, t^2 exact, their product with Wd one."""
    x = np.asarray(x, np.float32)
    N, M, O, Hc, Wc = x.shape
    P = M * (M - 1) // 2
    vals, mags = [Fraction(0)] * 7, [Fraction(0)] * 7
    n_live = 0
    for n in range(N):
        for o in range(O):
            for cy in range(Hc):
                for cx in range(Wc):
                    Wd = Fraction(float(q[n, o])) * Fraction(float(w[cy, cx]))
                    if Wd == 0:
                        continue
                    n_live += 1
                    X = [Fraction(float(v)) for v in x[n, :, o, cy, cx]]
                    T = Fraction(float(t[n, o, cy, cx]))
                    S, sabs = sum(X), sum(abs(v) for v in X)
                    m, mm = S / M, sabs / M + abs(T)
                    v = [sum(abs(a - T) for a in X), sum(abs(X[i] - X[j]) for i in range(M) for j in range(i + 1, M)),
                         sum((M * a - S) ** 2 for a in X), (m - T) ** 2, abs(m - T), T, T * T]
                    g = [sum(abs(a) + abs(T) for a in X), sum(abs(X[i]) + abs(X[j]) for i in range(M) for j in range(i + 1, M)),
                         sum((M * abs(a) + sabs) ** 2 for a in X), mm * mm, mm, abs(T), T * T]
                    for k in range(7):
                        vals[k] += Wd * v[k]
                        mags[k] += Wd * g[k]
    return vals, mags, [M + 1, P + 1, 3 * M + 1, 2 * (M + 1) + 2, M + 2, 1, 1], n_live


def total_bounds(x, t, q, w):
    """per total: (exact value, bound of ANY summation order) -- gamma(n_live - 1 + roundings inside a term) * magnitude"""
    vals, mags, rnd, n_live = exact_totals(x, t, q, w)
    return [(vals[k], EM.gamma(n_live - 1 + rnd[k]) * mags[k]) for k in range(7)]


def order_bounds(terms, live):
    """per total: (math.fsum of the model's terms, the bound of ANY summation order of THOSE terms): the kernel's per-cell terms
    have the model's bits (one f64 operation each, the same order), so two sums of them differ from their exact sum by at most
    gamma(n - 1) * sum |term| each; gamma(n) here, one rounding more for fsum's own result.  Cheap where the `fractions` walk of
    total_bounds is not (tens of thousands of cells)."""
    import math
    n = int(np.asarray(live).sum())
    out = []
    for k in range(7):
        t = np.asarray(terms[k], np.float64).reshape(-1)
        out.append((math.fsum(t), float(EM.gamma(n)) * math.fsum(np.abs(t))))
    return out
