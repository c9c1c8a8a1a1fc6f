"""The model of nint_ens_accum (include/nint.h) and of inference.ensemble_from_sums: numpy f64 in the kernel's
documented order, python `fractions` for the exact values, brute force for the derived statistics.  No GPU, no library.

Per cell (sample, output, crop pixel), x_i = (double)member i, t = (double)target, one f64 operation per product and sum:
    S = ((0 + x_0) + x_1) + ... + x_{M-1}         E = S - M*t
    A = sum_i |x_i - t|,  V = sum_i (M*x_i - S)^2    (i ascending, from 0.0)
    D = sum_{i<j} |x_i - x_j|                        ((i, j) lexicographic, from 0.0)
    r = #{i : x_i < t};  bin M + 1 instead where t or any x_i is NaN
numpy's elementwise f64 operations are single IEEE operations (no contraction), so `cells` gives the kernel's bits on any data;
a map cell then grows from its stored value by the slot's samples in ascending n; a sample row is a sum over the crop in
another order than the kernel's tree, equal only where the sums are exact (integer data)."""
from fractions import Fraction

import numpy as np

PIX, SAMPLE = 7, 8
U64 = 2.0 ** -53


def cells(x, t):
    """x (N, M, O, Hc, Wc) f32 members on the crop, t (N, O, Hc, Wc) f32 -> dict of (N, O, Hc, Wc) arrays: E, V, A, D (f64),
    rank (int64, M + 1 for a NaN cell)"""
    x, t = np.asarray(x, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    M = x.shape[1]
    dM = float(M)
    with np.errstate(invalid="ignore"):
        S, A = np.zeros_like(t), np.zeros_like(t)
        r = np.zeros(t.shape, np.int64)
        bad = np.isnan(t)
        for i in range(M):
            S = S + x[:, i]
            A = A + np.abs(x[:, i] - t)
            r += x[:, i] < t
            bad |= np.isnan(x[:, i])
        V, D = np.zeros_like(t), np.zeros_like(t)
        for i in range(M):
            dv = dM * x[:, i] - S
            V = V + dv * dv
            for j in range(i + 1, M):
                D = D + np.abs(x[:, i] - x[:, j])
        E = S - dM * t
    return {"E": E, "V": V, "A": A, "D": D, "S": S, "t": t, "rank": np.where(bad, M + 1, r)}


def sums(x, t, slot, nslots, row_w, pix_before, hist_before):
    """nint_ens_accum: pix (S, 7, O, Hc, Wc) grown from pix_before in sample order, sample (N, O, 8), rank_hist (S, O, M + 2)
    grown from hist_before, mean (N, O, Hc, Wc) f32.  slot: N ints in [-1, nslots) or None."""
    c = cells(x, t)
    N, M = np.asarray(x).shape[:2]
    sl = np.zeros(N, np.int64) if slot is None else np.asarray(slot, np.int64)
    assert sl.shape == (N,) and sl.min() >= -1 and sl.max() < nslots
    Hc = c["t"].shape[2]
    rw = (np.ones(Hc) if row_w is None else np.asarray(row_w, np.float64))[None, None, :, None]
    with np.errstate(invalid="ignore"):
        EE, tt = c["E"] * c["E"], c["t"] * c["t"]
        terms = np.stack([EE, c["V"], c["A"], c["D"], c["E"], c["t"], tt])                     # (7, N, O, Hc, Wc)
        pix = np.array(pix_before, np.float64, copy=True)
        hist = np.array(hist_before, np.int64, copy=True)
        for n in range(N):
            if sl[n] >= 0:
                pix[sl[n]] = pix[sl[n]] + terms[:, n]
                for o in range(terms.shape[2]):
                    hist[sl[n], o] += np.bincount(c["rank"][n, o].reshape(-1), minlength=M + 2)
        st = np.stack([EE, c["V"], c["A"], c["D"], rw * EE, rw * c["V"], rw * c["A"], rw * c["D"]])
        sample = np.ascontiguousarray(st.sum(axis=(3, 4)).transpose(1, 2, 0))
        mean = (c["S"] / float(M)).astype(np.float32)
    return {"pix": pix, "sample": sample, "rank_hist": hist, "mean": mean, "terms": terms, "sample_terms": st}


# ------------------------------------------------------------------------------ exact values and the any-order bound
def exact_cell(xs, t, rw=1.0):
    """One cell in exact arithmetic: xs (M f32 values), t.  Returns (values, magnitudes, roundings) of the seven map terms
    [E^2, V, A, D, E, t, t^2] as Fractions / ints.

    magnitude: the term with every ingredient replaced by its absolute value (what the rounding errors scale with);
    roundings: the f64 operations inside the term that may round.  With u = 2^-53 and g(k) = k u / (1 - k u):
      E   = x_0 + ... + x_{M-1} - M t: M + 1 exact operands (M t: a 24-bit by a 7-bit integer), M additions;
            |E^ - E| <= g(M) mE, mE = sum |x_i| + M |t|.
      E^2 : one product more, and the error of E^ enters twice: 2 M + 1, magnitude mE^2.
      V   = sum_i (M x_i - S)^2: M x_i exact, S^ carries M - 1 roundings, the subtraction 1, the square as above: 2 M + 1
            per term of magnitude (M |x_i| + sum |x|)^2; M - 1 additions join the M terms: 3 M in all.
      A   = sum_i |x_i - t|: one rounding per difference, M - 1 additions: M; magnitude sum (|x_i| + |t|).
      D   = sum of P = M (M - 1) / 2 differences: one rounding per difference, P - 1 additions: P; magnitude
            sum (|x_i| + |x_j|).
      t, t^2: exact in f64 (a 24-bit significand squared has 48 bits): 0."""
    M = len(xs)
    X = [Fraction(float(v)) for v in xs]
    T = Fraction(float(t))
    S = sum(X)
    sabs = sum(abs(v) for v in X)
    E = S - M * T
    mE = sabs + M * abs(T)
    P = M * (M - 1) // 2
    vals = [E * E, sum((M * v - S) ** 2 for v in X), sum(abs(v - T) for v in X),
            sum(abs(X[i] - X[j]) for i in range(M) for j in range(i + 1, M)), E, T, T * T]
    mags = [mE * mE, sum((M * abs(v) + sabs) ** 2 for v in X), sum(abs(v) + abs(T) for v in X),
            sum(abs(X[i]) + abs(X[j]) for i in range(M) for j in range(i + 1, M)), mE, abs(T), T * T]
    return vals, mags, [2 * M + 1, 3 * M, M, P, M, 0, 0]


def gamma(k):
    return Fraction(k) * Fraction(U64) / (1 - Fraction(k) * Fraction(U64))


# ------------------------------------------------------------------------------ the derived statistics, by brute force
def brute_stats(x, t):
    """x (n, M) members, t (n) targets, any reals: the statistics ensemble_from_sums derives, straight from their definitions"""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    n, M = x.shape
    mean = x.mean(axis=1)
    mse = float(((mean - t) ** 2).mean())
    var = float(x.var(axis=1, ddof=1).mean())
    a = np.abs(x - t[:, None]).mean(axis=1)
    pair = np.abs(x[:, :, None] - x[:, None, :]).sum(axis=(1, 2))             # every ordered pair: 2 D
    fair = float((a - pair / (2.0 * M * (M - 1))).mean())
    plain = float((a - pair / (2.0 * M * M)).mean())
    ss_tot = float(((t - t.mean()) ** 2).sum())
    return {"rmse_mean": mse ** 0.5, "spread": var ** 0.5, "spread_skill": ((M + 1.0) / M) ** 0.5 * var ** 0.5 / mse ** 0.5,
            "crps_fair": fair, "crps": plain, "bias": float((mean - t).mean()),
            "r2_mean": 1.0 - float(((mean - t) ** 2).sum()) / ss_tot}


# ------------------------------------------------------------------------------ test data
def int_data(rng, N, M, O, H, W, oy, ox, Hc, Wc):
    """Integer members and targets in [-8, 8] on which every f64 sum of the rule is exact in any order (|E| <= 16 M, V <=
    M (16 M)^2, D <= 16 M^2 / 2: far below 2^53 times any count used here).  pred (N, M, O, H, W) f32, NaN outside the crop;
    y (N, O, Hc, Wc).  Planted: ties x_i == t, cells with t below and above every member, identical members."""
    pred = np.full((N, M, O, H, W), np.nan, np.float32)
    x = rng.integers(-6, 7, (N, M, O, Hc, Wc)).astype(np.float32)
    y = rng.integers(-6, 7, (N, O, Hc, Wc)).astype(np.float32)
    y[:, :, 0, 0] = x[:, 0, :, 0, 0]                      # a tie with member 0
    y[:, :, 0, 1] = -8.0                                  # below every member: rank 0
    y[:, :, 0, 2] = 8.0                                   # above every member: rank M
    x[:, :, :, 1, 0] = x[:, :1, :, 1, 0]                  # identical members
    y[:, :, 1, 1] = x[:, :, :, 1, 1].max(axis=1)          # ties with the largest member(s)
    pred[:, :, :, oy:oy + Hc, ox:ox + Wc] = x
    return pred, x, y


def dyadic_rows(Hc):
    return (1 + (np.arange(Hc) % 8)) / 8.0
