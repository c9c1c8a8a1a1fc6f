"""The model of nint_spec_accum (include/nint.h): numpy f64 for the five planes with a given table, exact
integer / `fractions` arithmetic for the values the kernel approximates, and the operation count of the documented order.  No
GPU, no library.

For a crop row f[0..Wc) and the table tw (Wc, 2):  F_k = sum_x f[x] (tw[j, 0] + i tw[j, 1]), j = (k x) mod Wc, 0 <= k < K = Wc // 2
+ 1.  With Y the target's transform, P_i member i's, S = sum_i P_i and w the row's weight, a row adds
    YY = w |Y|^2    PP = w sum_i |P_i|^2    CR = w Re(S conj Y)    CI = w Im(S conj Y)    SS = w |S|^2
to entry (slot, plane, o, k).  `planes` forms the row transforms by a matrix product -- another order than the kernel's chain,
so its bits are the kernel's only where every sum is exact (integer data with an integer table).  `exact_planes` forms the same
values without any rounding from the table's and the data's own f64 values, as integers on a common power-of-two scale."""
from fractions import Fraction

import numpy as np

PLANES = 5
YY, PP, CR, CI, SS = range(5)
U64 = 2.0 ** -53


def index_matrix(Wc):
    """(K, Wc) int: j = (k x) mod Wc"""
    K = Wc // 2 + 1
    return (np.arange(K)[:, None] * np.arange(Wc)[None, :]) % Wc


def transform(f, tw):
    """f (..., Wc) -> (re, im) each (..., K): F_k with the given table, in f64 by a matrix product"""
    f, tw = np.asarray(f, np.float64), np.asarray(tw, np.float64)
    J = index_matrix(f.shape[-1])
    return f @ tw[J, 0].T, f @ tw[J, 1].T


def planes(x, t, tw, row_w=None):
    """x (N, M, O, Hc, Wc) members on the crop, t (N, O, Hc, Wc) -> (N, 5, O, K) f64: each sample's five sums over its rows"""
    x, t = np.asarray(x, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    Hc = t.shape[2]
    w = (np.ones(Hc) if row_w is None else np.asarray(row_w, np.float64))[None, None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        Yr, Yi = transform(t, tw)                                       # (N, O, Hc, K)
        Pr, Pi = transform(x, tw)                                       # (N, M, O, Hc, K)
        Sr, Si = Pr.sum(axis=1), Pi.sum(axis=1)
        rows = np.stack([w * (Yr * Yr + Yi * Yi), w * (Pr * Pr + Pi * Pi).sum(axis=1), w * (Sr * Yr + Si * Yi),
                         w * (Si * Yr - Sr * Yi), w * (Sr * Sr + Si * Si)], axis=1)   # (N, 5, O, Hc, K)
        return rows.sum(axis=3)


def sums(x, t, tw, slot, nslots, row_w, spec_before):
    """nint_spec_accum: spec (nslots, 5, O, K) grown from spec_before by the samples in ascending n; slot None = all 0"""
    per = planes(x, t, tw, row_w)
    N = per.shape[0]
    sl = np.zeros(N, np.int64) if slot is None else np.asarray(slot, np.int64)
    assert sl.shape == (N,) and sl.min() >= -1 and sl.max() < nslots
    spec = np.array(spec_before, np.float64, copy=True)
    with np.errstate(invalid="ignore"):
        for n in range(N):
            if sl[n] >= 0:
                spec[sl[n]] = spec[sl[n]] + per[n]
    return spec


# ------------------------------------------------------------------------------ exact values and the any-order bound
def _ints(a, bits):
    """the f64 array a times 2^bits as python integers (an object array); refuses a value that is no integer on that scale"""
    v = np.ldexp(np.asarray(a, np.float64), bits)
    assert np.isfinite(v).all() and (v == np.rint(v)).all(), f"not exact on the 2^-{bits} scale"
    return np.array([int(z) for z in v.ravel()], dtype=object).reshape(v.shape)


def exact_planes(x, t, tw, row_w=None, data_bits=80, table_bits=64, weight_bits=60):
    """The five sums of every sample in exact arithmetic, from the f64 values of the table, the f32 data and the weights.
    Returns (values, magnitudes), each an (N, 5, O, K) object array of Fractions; a magnitude is the value's expression with
    every table entry and datum replaced by its absolute value -- what the rounding errors of any evaluation order scale with.
    Everything is an integer on the scale 2^-(weight_bits + 2 (data_bits + table_bits)); the scales are asserted to be exact."""
    x, t = np.asarray(x, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    N, M, O, Hc, Wc = x.shape
    J = index_matrix(Wc)
    T = _ints(tw, table_bits)
    Er, Ei = T[J, 0].T, T[J, 1].T                                       # (Wc, K)
    X, Y = _ints(x, data_bits), _ints(t, data_bits)
    w = _ints(np.ones(Hc) if row_w is None else row_w, weight_bits)
    assert all(v >= 0 for v in w)
    w = w[None, None, :, None]

    def five(Yr, Yi, Pr, Pi, sign):
        Sr, Si = Pr.sum(axis=1), Pi.sum(axis=1)
        rows = [w * (Yr * Yr + Yi * Yi), w * (Pr * Pr + Pi * Pi).sum(axis=1), w * (Sr * Yr + Si * Yi),
                w * (Si * Yr + sign * (Sr * Yi)), w * (Sr * Sr + Si * Si)]
        return np.stack([r.sum(axis=2) for r in rows], axis=1)          # (N, 5, O, K)

    val = five(np.dot(Y, Er), np.dot(Y, Ei), np.dot(X, Er), np.dot(X, Ei), -1)
    aX, aY, aEr, aEi = abs(X), abs(Y), abs(Er), abs(Ei)
    mag = five(np.dot(aY, aEr), np.dot(aY, aEi), np.dot(aX, aEr), np.dot(aX, aEi), +1)
    scale = 2 ** (weight_bits + 2 * (data_bits + table_bits))
    frac = np.vectorize(lambda v: Fraction(int(v), scale), otypes=[object])
    return frac(val), frac(mag)


def n_ops(Wc, M, Hc, n_samples):
    """An upper count of the roundings that any single product f * tw * f' * tw' * w passes through on its way into an entry,
    in the order include/nint.h documents:
      a transform component is a chain of Wc fused multiply-adds: Wc roundings;
      S = sum_i P_i: M additions more (Wc + M);  pp = sum_i (Pr^2 + Pi^2): 2 Wc + 1 for a square, 1 for the pair, M additions;
      a row term is a product of two such components (their roundings add), the product itself, the sum of the two products
      and the weight: at most 2 (Wc + M) + 3 (SS; the others carry fewer);
      the rows of a sample: ceil(Hc / R) + R - 1 <= Hc additions, whatever R is;  the samples of a slot: one addition each.
    With u = 2^-53 and gamma(k) = k u / (1 - k u):  |got - exact| <= gamma(n_ops) * (|stored value| + sum of the magnitudes)."""
    return 2 * (Wc + M) + 3 + Hc + n_samples


def gamma(k):
    return Fraction(k) * Fraction(U64) / (1 - Fraction(k) * Fraction(U64))


# ------------------------------------------------------------------------------ the reference table
def reference_twiddles(Wc):
    """(cos, -sin)(2 pi j / Wc) in numpy.longdouble, (Wc, 2), and the mask of the components that are exact (whole quarter
    turns), where the true value is 0 or +-1"""
    ld = np.longdouble
    pi = ld("3.14159265358979323846264338327950288")
    j = np.arange(Wc, dtype=ld)
    a = 2 * pi * j / ld(Wc)
    ref = np.stack([np.cos(a), -np.sin(a)], axis=1)
    quarter = (4 * np.arange(Wc)) % Wc == 0
    exact = np.zeros((Wc, 2), bool)
    exact[quarter] = True
    q = (4 * np.arange(Wc)) // Wc
    ref[quarter, 0] = np.array([1, 0, -1, 0], dtype=ld)[q[quarter]]
    ref[quarter, 1] = np.array([0, -1, 0, 1], dtype=ld)[q[quarter]]
    return ref, exact


# ------------------------------------------------------------------------------ test data
def int_table(rng, Wc):
    """an integer-valued table in [-3, 3]: the kernel is then a map of integers to integers"""
    return rng.integers(-3, 4, (Wc, 2)).astype(np.float64)


def int_data(rng, N, M, O, H, W, oy, ox, Hc, Wc):
    """integer members and targets in [-8, 8]: pred (N, M, O, H, W) f32 with NaN outside the crop, x (N, M, O, Hc, Wc), y (N, O, Hc, Wc)"""
    pred = np.full((N, M, O, H, W), np.nan, np.float32)
    x = rng.integers(-8, 9, (N, M, O, Hc, Wc)).astype(np.float32)
    y = rng.integers(-8, 9, (N, O, Hc, Wc)).astype(np.float32)
    pred[:, :, :, oy:oy + Hc, ox:ox + Wc] = x
    return pred, x, y


def dyadic_rows(Hc):
    return (1 + (np.arange(Hc) % 8)) / 8.0


def int_magnitude_bound(Wc, Hc, M, N, before=8):
    """the largest magnitude any partial sum of the integer cases can reach, in units of the weights' 1/8: a transform component
    is at most 8 * 3 * Wc, S at most M times that, a row term at most 2 (M * 24 Wc)^2 * 8, an entry Hc * N of them plus the
    stored integer.  Must stay far below 2^53 for every f64 sum to be exact in any order."""
    f = 24 * Wc
    return 8 * before + Hc * N * 8 * 2 * (M * f) ** 2
