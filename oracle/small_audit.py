"""f64 references and derived error bounds for the kernels of ``csrc/pointwise.hip``, ``csrc/head.hip`` and ``csrc/pack.hip`` around the gate GEMMs: the 1x1
head, the crop + MSE + L1 loss, their fused form, flat Adam, the layout packers, the preproc and the evaluation skill sums
(TEST INFRASTRUCTURE ONLY; numpy / torch-CPU, no GPU).

Every reference is computed from the values the kernel READS as they are stored (bf16 inputs upcast exactly, like
``oracle/stored_audit.py``), and every comparator looks at every element: nothing is skipped, masked or budgeted.  A
comparator returns the largest ``|got - ref| / bound`` and raises ``AuditError`` naming the worst element when it
exceeds 1 (a zero bound means equality).

Error model: ``U = 2^-24`` is the f32 unit roundoff, ``gamma(k) = k U / (1 - k U)`` bounds ``k`` accumulated roundings
(Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1), one round-to-nearest to bf16 (8 significand bits) moves a value by
at most half an ulp of its binade, ``halfulp_bf16``.  Where a kernel is a chain of individually rounded operations (Adam) the bound is carried through
the chain as a running error bound by ``_E``: a value ``v`` and a bound ``e`` on the distance of the kernel's f32
register from it; each f32 operation adds ``U (|v| + e)``.  No constant here comes from a run.
"""
from __future__ import annotations

import numpy as np

__all__ = ["U", "U64", "halfulp_bf16", "gamma", "AuditError", "ratio", "check_equal", "bf16_round", "decode_bf16",
           "head_fwd", "head_bwd_dh", "loss", "check_loss_scalar", "check_stats", "head_loss_fused", "adam",
           "pack_btchw", "unpack_halo", "pack_compact", "unpack_compact", "unfold_dx", "preproc", "make_geom",
           "SKILL_PIX", "SKILL_SAMPLE", "skill_terms", "skill_sums", "skill_head_pred", "skill_audit", "skill_int_data",
           "skill_head_int_data", "skill_slots"]

U = 2.0 ** -24
U64 = 2.0 ** -53      # the f64 unit roundoff (the skill sums)
SUM_RTOL = 1e-12      # double-precision sums of at most a few 1e5 terms (the tolerance tests/test_gpu_small_kernels.py uses)


def gamma(k: int, u: float = U) -> float:
    return k * u / (1.0 - k * u)


class AuditError(AssertionError):
    pass


def ratio(got, ref, bound, what: str = "") -> float:
    """max over EVERY element of |got - ref| / bound (0/0 = 0, x/0 = inf); raises AuditError above 1 or on a non-finite
    value."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if got.shape != ref.shape or ref.shape != bound.shape:
        raise AuditError(f"{what}: shapes {got.shape} / {ref.shape} / {bound.shape}")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AuditError(f"{what}: element {tuple(int(j) for j in i)}: got {got[i]!r}, reference {ref[i]!r}, "
                         f"bound {bound[i]!r} (ratio {worst:.3g}); {int((r > 1).sum())} of {r.size} elements outside")
    return worst


def check_equal(got, ref, what: str = "") -> None:
    """bit-for-bit equality of two arrays of one dtype (-0.0 == +0.0 is not granted: compare the bytes)"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        raise AuditError(f"{what}: {got.dtype}{got.shape} against {ref.dtype}{ref.shape}")
    bad = got.view(np.uint8).reshape(got.shape + (-1,)) != ref.view(np.uint8).reshape(ref.shape + (-1,))
    bad = bad.any(axis=-1)
    if bad.any():
        i = tuple(int(j) for j in np.argwhere(bad)[0])
        raise AuditError(f"{what}: element {i}: got {got[i]!r}, expected {ref[i]!r}; {int(bad.sum())} of {bad.size} differ")


def bf16_round(x) -> np.ndarray:
    """f32 -> nearest bf16 (ties to even) -> f32, the conversion of ``(__bf16)f`` (finite values)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def halfulp_bf16(x) -> np.ndarray:
    """Half an ulp of bf16 in the binade of |x|: 2^(floor(log2 |x|) - 8), i.e. 2^-9 times the power of two ABOVE |x|.
    It lies between 2^-9 |x| (x just below a power of two) and 2^-8 |x| (x a power of two); 2^-9 |x| itself cannot hold in
    general: 1.00388 rounds to 1.0, a move of 2^-8.01 |x| (tests/test_small_audit_cpu.py shows it on torch's own
    conversion)."""
    x = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        return np.where(x > 0, np.exp2(np.floor(np.log2(np.where(x > 0, x, 1.0))) - 8.0), 0.0)


def decode_bf16(raw_u16) -> np.ndarray:
    """stored bf16 bit patterns (uint16) -> f32, exact"""
    return (np.ascontiguousarray(raw_u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def make_geom(H: int, W: int, P: int):
    """(H, W, P, Hh, Wh) of include/nint.h: rows rounded up to 8, columns to 32, plus the halo on both sides"""
    return H, W, P, (H + 7) // 8 * 8 + 2 * P, (W + 31) // 32 * 32 + 2 * P


# --------------------------------------------------------------------------- 1x1 head
def head_fwd(h, w, b):
    """pred[n][o][y][x] = b[o] + sum_c w[o][c] h[n][y][x][c] in f64 from the stored h (N, H, W, Ch), w (O, Ch), b (O) or
    None.  Returns (pred, bound), both (N, O, H, W).

    Bound: the kernels (head_fwd_kernel, head_fwd_wide_kernel, phase 1 of head_loss_fused_kernel) start the accumulator
    at b[o] and add Ch products, one after the other; the staged kernels add further products with a zero weight, which
    change nothing.  Whatever the order, and whether a product is rounded on its own or fused into the add, every term
    passes through at most Ch + 1 roundings (its own product and the Ch adds), so
    ``|pred - ref| <= gamma(Ch + 1) (|b| + sum_c |w h|)`` (Higham 3.1 / 3.3)."""
    h, w = np.asarray(h, np.float64), np.asarray(w, np.float64)
    Ch = w.shape[1]
    bb = np.zeros(w.shape[0]) if b is None else np.asarray(b, np.float64)
    pred = np.einsum("nyxc,oc->noyx", h, w) + bb[None, :, None, None]
    mag = np.einsum("nyxc,oc->noyx", np.abs(h), np.abs(w)) + np.abs(bb)[None, :, None, None]
    return pred, gamma(Ch + 1) * mag


def head_bwd_dh(w, dpred, Chp: int, bf16: bool, dpred_err=None):
    """dh[n][y][x][c] = sum_o w[o][c] dpred[n][o][y][x] in f64; channels [Ch, Chp) are exactly 0 (bound 0).  Returns
    (dh, bound), both (N, H, W, Chp).

    Bound: the accumulator starts at 0 and adds O products (head_bwd_dh_kernel, head_bwd_dh_wide_kernel, phase 2 of the
    fused kernel): at most O roundings per term, ``gamma(O) sum_o |w| |dpred|``.  ``dpred_err`` (fused kernel: the
    kernel's own dpred is only known to within that bound) enters as ``sum_o |w| err`` and through the magnitudes the
    roundings act on.  bf16 storage rounds the f32 register once, to nearest: half a bf16 ulp of its
    magnitude, which is at most ``|ref|`` plus the f32 bound (``halfulp_bf16``)."""
    w, dpred = np.asarray(w, np.float64), np.asarray(dpred, np.float64)
    O, Ch = w.shape
    N, _, H, W = dpred.shape
    err = np.zeros_like(dpred) if dpred_err is None else np.asarray(dpred_err, np.float64)
    ref = np.zeros((N, H, W, Chp))
    bound = np.zeros((N, H, W, Chp))
    ref[..., :Ch] = np.einsum("noyx,oc->nyxc", dpred, w)
    prop = np.einsum("noyx,oc->nyxc", err, np.abs(w))
    bound[..., :Ch] = prop + gamma(O) * np.einsum("noyx,oc->nyxc", np.abs(dpred) + err, np.abs(w))
    if bf16:
        bound[..., :Ch] += halfulp_bf16(np.abs(ref[..., :Ch]) + bound[..., :Ch])
    return ref, bound


# --------------------------------------------------------------------------- loss
def _r2(s0: float, y64: np.ndarray) -> float:
    """sklearn.metrics.r2_score of one batch: 1 - ss_res / ss_tot with ss_tot about the mean; a constant target has
    ss_tot = 0 and scores 1 when the residual is 0 as well, else 0"""
    if y64.min() == y64.max():
        return 1.0 if s0 == 0.0 else 0.0
    return 1.0 - s0 / float(np.sum((y64 - y64.mean()) ** 2))


def loss(pred, y, oy: int, ox: int):
    """MSE + L1 (both means) of pred (N, O, H, W) f32 cropped to y (N, O, Hc, Wc) f32 at (oy, ox).

    The operation is DEFINED on ``d = pred - y`` formed in f32 (loss_partial_kernel: ``const float d = pred[i] - t``;
    numpy's f32 subtraction gives the same bits), everything after that is double: s0 = sum d^2, s1 = sum |d|,
    s2 = sum y, s3 = sum y^2 in f64.  ``dpred = (float)((2.0 * d + sign(d)) * (1.0 / n))`` with sign(0) = 0 is
    reproducible bit for bit: ``2.0 * d`` is exact in double, so contracting it into the add cannot change the sum; one
    rounding for the add, one for the product, one to f32 -- the same three IEEE operations numpy performs.  Outside the
    crop dpred is +0.  Returns a dict: dpred (f32, exact), sums (s0, s1, s2, s3, n), abs (the sums of the terms'
    magnitudes, what SUM_RTOL is relative to), loss (f64), r2, r2_tol.

    r2_tol: the kernel forms ``ss_tot = s3 - s2^2 / n`` from sums that are each good to SUM_RTOL of their terms'
    magnitudes, so ``|d ss_tot| <= delta = SUM_RTOL (s3 + 2 S2^2 / n) + 2^-51 (s3 + S2^2 / n)`` with S2 = sum |y| (three
    double roundings), and ``r2 = 1 - q``, ``q = s0 / ss_tot``, moves by at most ``q (SUM_RTOL + delta / ss_tot) /
    (1 - delta / ss_tot) + 2^-51 (1 + q)``.  A constant target leaves no tolerance: the kernel must take the ``ss_tot <= 0``
    branch and add exactly 1 or 0 (its one-pass ss_tot is exactly 0 whenever n y^2 is exact in double, e.g. y = 0.5)."""
    pred, y = np.asarray(pred, np.float32), np.asarray(y, np.float32)
    N, O, H, W = pred.shape
    Hc, Wc = y.shape[2:]
    d = pred[:, :, oy:oy + Hc, ox:ox + Wc] - y                      # f32, the definition
    d64, y64 = d.astype(np.float64), y.astype(np.float64)
    n = float(N * O * Hc * Wc)
    s0, s1, s2, s3 = float(np.sum(d64 * d64)), float(np.sum(np.abs(d64))), float(np.sum(y64)), float(np.sum(y64 * y64))
    inv_n = 1.0 / n
    dp = np.zeros(pred.shape, np.float32)
    dp[:, :, oy:oy + Hc, ox:ox + Wc] = ((2.0 * d64 + np.sign(d64)) * inv_n).astype(np.float32)
    S2 = float(np.sum(np.abs(y64)))
    r2 = _r2(s0, y64)
    r2_tol = 0.0
    if y64.min() != y64.max():
        ss = float(np.sum((y64 - y64.mean()) ** 2))
        delta = SUM_RTOL * (s3 + 2 * S2 * S2 / n) + 2.0 ** -51 * (s3 + S2 * S2 / n)
        q = s0 / ss
        r2_tol = q * (SUM_RTOL + delta / ss) / (1.0 - delta / ss) + 2.0 ** -51 * (1.0 + q)
    return {"dpred": dp, "sums": np.array([s0, s1, s2, s3, n]), "abs": np.array([s0, s1, S2, s3, n]),
            "loss": s0 / n + s1 / n, "r2": r2, "r2_tol": r2_tol}


def check_loss_scalar(got_f32, loss64: float, extra: float = 0.0, what: str = "loss") -> float:
    """The f32 loss is the double ``s0 / n + s1 / n`` (good to SUM_RTOL) rounded once: within one f32 ulp of the f64 value
    (half an ulp for the rounding, the rest for the double sums' order).  ``extra``: what the caller's inputs add."""
    ulp = float(np.spacing(np.float32(abs(loss64))))
    return ratio(np.float64(got_f32), np.float64(loss64), np.float64(ulp + extra), what)


def check_stats(before, after, refs, sum_tol=None, what: str = "stats") -> float:
    """``stats[0..7]`` after the calls ``refs`` (a list of loss() dicts, in call order) were accumulated onto ``before``:
    [0..4] += (s0, s1, s2, s3, n), [5] += loss, [6] += r2, [7] += 1.  Double sums: SUM_RTOL of the summed magnitudes (for
    the signed sum s2 that is sum |y|, the quantity its rounding is relative to; for the others the sum itself); the count
    and the call counter are exact; r2 by loss()'s r2_tol.  ``sum_tol`` (8 values) is added where the sums' inputs carry a
    bound of their own (fused kernel)."""
    before, after = np.asarray(before, np.float64), np.asarray(after, np.float64)
    ref, mag, tol = before.copy(), np.abs(before), np.zeros(8)
    for r in refs:
        ref[:5] += r["sums"]
        mag[:5] += r["abs"]
        ref[5] += r["loss"]; mag[5] += abs(r["loss"])
        ref[6] += r["r2"]; tol[6] += r["r2_tol"]
        ref[7] += 1.0
    tol[:4] += SUM_RTOL * mag[:4]
    tol[5] += 2 * SUM_RTOL * mag[5]
    tol[6] += 2.0 ** -52 * len(refs) * (np.abs(ref[6]) + 1.0) if tol[6] > 0 else 0.0
    if sum_tol is not None:
        tol += np.asarray(sum_tol, np.float64)
    return ratio(after, ref, tol, what)


# --------------------------------------------------------------------------- fused head + loss
def head_loss_fused(h, w, b, y, oy: int, ox: int, Chp: int, bf16: bool):
    """nint_head_loss_fused from the stored h (N, H, W, Ch): pred in f64, d_ref = pred - y in f64 on the crop,
    dpred_ref = (2 d_ref + sign(d_ref)) / n, dh_ref = w^T dpred_ref.  Returns a dict of (ref, bound) pairs and the
    loss() style sums with their tolerances.

    With E the head-forward bound of the pixel, the kernel's f32 ``d = p - t`` is within
    ``Ed = E + U (|d_ref| + E)`` of d_ref (t is a stored value; the subtraction rounds once).  Then
    ``|dpred - dpred_ref| <= (2 Ed + 2 [|d_ref| <= Ed]) / n + U (|dpred_ref| + that)``: the slope 2, a sign that may
    legitimately differ only where d_ref is within Ed of zero (a jump of at most 2), and the final rounding of the double
    product to f32 (the double operations themselves add 2^-52 relative, counted inside that last term's U).  No element
    is left out: where the sign is in doubt the bound is wide, everywhere else it is tight.  dh: head_bwd_dh's bound with
    that dpred error propagated through ``sum_o |w| err``.  The sums: ``|d^2 - d_ref^2| <= 2 |d_ref| Ed + Ed^2`` and
    ``||d| - |d_ref|| <= Ed`` per term on top of SUM_RTOL; s2, s3 and n do not depend on the head."""
    y32 = np.asarray(y, np.float32)
    y64 = y32.astype(np.float64)
    pred, E = head_fwd(h, w, b)
    N, O, H, W = pred.shape
    Hc, Wc = y64.shape[2:]
    n = float(N * O * Hc * Wc)
    crop = (slice(None), slice(None), slice(oy, oy + Hc), slice(ox, ox + Wc))
    d = pred[crop] - y64
    Ed = E[crop] + U * (np.abs(d) + E[crop])
    dp, dpb = np.zeros_like(pred), np.zeros_like(pred)
    dp[crop] = (2.0 * d + np.sign(d)) / n
    core = (2.0 * Ed + 2.0 * (np.abs(d) <= Ed)) / n
    dpb[crop] = core + U * (np.abs(dp[crop]) + core)
    dh, dhb = head_bwd_dh(w, dp, Chp, bf16, dpred_err=dpb)
    s0, s1, s2, s3 = float(np.sum(d * d)), float(np.sum(np.abs(d))), float(np.sum(y64)), float(np.sum(y64 * y64))
    t0, t1 = float(np.sum(2 * np.abs(d) * Ed + Ed * Ed)), float(np.sum(Ed))
    S2 = float(np.sum(np.abs(y64)))
    lossv = s0 / n + s1 / n
    r2, r2_tol = _r2(s0, y64), 0.0
    if y64.min() != y64.max():
        ss = float(np.sum((y64 - y64.mean()) ** 2))
        delta = SUM_RTOL * (s3 + 2 * S2 * S2 / n) + 2.0 ** -51 * (s3 + S2 * S2 / n)
        q = s0 / ss
        r2_tol = (q * (SUM_RTOL + delta / ss) + t0 / ss) / (1.0 - delta / ss) + 2.0 ** -51 * (1.0 + q)
    ref = {"dpred": dp, "sums": np.array([s0, s1, s2, s3, n]), "abs": np.array([s0, s1, S2, s3, n]), "loss": lossv,
           "r2": r2, "r2_tol": r2_tol}
    sum_tol = np.array([t0, t1, 0, 0, 0, (t0 + t1) / n, 0, 0])
    return {"pred": (pred, E), "dpred": (dp, dpb), "dh": (dh, dhb), "loss": ref, "sum_tol": sum_tol,
            "loss_extra": (t0 + t1) / n}


# --------------------------------------------------------------------------- Adam
class _E:
    """running error bound: v = the real value, e >= |kernel's f32 register - v|"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape) if np.ndim(v) else np.float64(e)

    @staticmethod
    def host(x: float) -> "_E":
        """a double scalar of the host cast to f32: one rounding"""
        return _E(np.float64(x), U * abs(x))

    def _rn(self, exact=False) -> "_E":
        """one round-to-nearest of a result whose magnitude is at most |v| + e (none where ``exact``)"""
        return _E(self.v, self.e + np.where(exact, 0.0, U * (np.abs(self.v) + self.e)))

    def _zero(self):
        return (self.v == 0) & (self.e == 0)

    # (a sum with an operand that is exactly zero is the other operand: no rounding)
    def __add__(self, o): return _E(self.v + o.v, self.e + o.e)._rn(self._zero() | o._zero())
    def __sub__(self, o): return _E(self.v - o.v, self.e + o.e)._rn(self._zero() | o._zero())
    def __neg__(self): return _E(-self.v, self.e)
    def __mul__(self, o): return _E(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)._rn()

    def __truediv__(self, o):
        q = self.v / o.v
        return _E(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))._rn()

    def sqrt(self) -> "_E":
        """sqrt is monotone: the register lies in [sqrt(max(v - e, 0)), sqrt(v + e)]"""
        s = np.sqrt(self.v)
        return _E(s, np.maximum(np.sqrt(self.v + self.e) - s, s - np.sqrt(np.maximum(self.v - self.e, 0.0))))._rn()


def adam(p, g, m, v, lr: float, beta1: float, beta2: float, eps: float, step: int, grad_scale: float = 1.0):
    """One step of ``torch.optim.Adam`` on float64 CPU tensors, from the f32 (p, m, v) stored BEFORE the step (so bounds
    are per step and never compound) and the pre-scaled gradient ``g * grad_scale``; ``step`` is the number of this step
    (the optimizer state is loaded with step - 1).  Returns {"p": (ref, bound), "m": ..., "v": ...}.

    Bounds count the roundings of adam_flat_kernel and nint_adam_flat, one per ``__f*_rn`` and one per host scalar cast to
    f32 (step_size = lr / bc1, 1 - beta1, beta2, 1 - beta2, sqrt(bc2), eps; grad_scale is passed as a float already):
      gr = g * grad_scale                                   1 rounding
      m' = m + w1 (gr - m)              (w1 < 0.5)          cast w1; sub, mul, add
      m' = gr - (gr - m) (1 - w1)       (else)              cast w1; sub, the f32 ``1.f - w1``, mul, sub
      v' = v b2 + (w2 gr) gr                                casts b2, w2; mul, mul, mul, add
      denom = sqrt(v') / sqrt_bc2 + eps                     casts sqrt_bc2, eps; sqrt, div, add
      p' = p + (-step_size m') / denom                      cast step_size; mul, div, add
    carried as running error bounds (``_E``), m' and v' entering the last two lines with the bounds just derived.  The two
    lerp forms are the same real function, so one reference serves both; which one the kernel runs changes only the
    bound.  Zero gradient on zero state: every product is an exact zero, denom = eps, p' = p: bound 0."""
    import torch
    p32, g32, m32, v32 = (np.asarray(a, np.float32) for a in (p, g, m, v))
    gs = float(np.float32(grad_scale))
    tp = torch.from_numpy(p32.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(beta1, beta2), eps=eps)
    tm, tv = torch.from_numpy(m32.astype(np.float64)), torch.from_numpy(v32.astype(np.float64))
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": tm, "exp_avg_sq": tv}
    tp.grad = torch.from_numpy(g32.astype(np.float64) * gs)
    opt.step()
    p_ref, m_ref, v_ref = tp.detach().numpy(), tm.numpy(), tv.numpy()
    # the kernel's chain on the real values
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    w1 = _E.host(1.0 - beta1)
    gr = _E(g32) * _E(np.float64(gs))
    M = _E(m32)
    if float(np.float32(1.0 - beta1)) < 0.5:
        Mn = M + w1 * (gr - M)
    else:
        Mn = gr - (gr - M) * (_E(np.float64(1.0)) - w1)
    Vn = _E(v32) * _E.host(beta2) + (_E.host(1.0 - beta2) * gr) * gr
    denom = Vn.sqrt() / _E.host(np.sqrt(bc2)) + _E.host(eps)
    Pn = _E(p32) + ((-_E.host(lr / bc1)) * Mn) / denom
    return {"p": (p_ref, Pn.e + np.abs(Pn.v - p_ref)), "m": (m_ref, Mn.e + np.abs(Mn.v - m_ref)),
            "v": (v_ref, Vn.e + np.abs(Vn.v - v_ref))}


# --------------------------------------------------------------------------- layout kernels (exact)
def _fold(x, kf: int):
    """(..., C, H, W) -> (..., kf*C, H, W): channel kx*C + c of pixel x = channel c of pixel x + kx - kf//2, 0 outside"""
    if kf <= 1:
        return x
    W = x.shape[-1]
    pad = np.zeros(x.shape[:-1] + (W + 2 * (kf // 2),), x.dtype)
    pad[..., kf // 2:kf // 2 + W] = x
    return np.concatenate([pad[..., kx:kx + W] for kx in range(kf)], axis=-3)


def pack_btchw(x, Cp: int, geom, kf: int = 1, bf16: bool = False) -> np.ndarray:
    """nint_pack_btchw / nint_pack_btchw_xfold onto a ZERO slab: x (B, T, C, H, W) f32 -> the slab as f32 values
    (T*B, Hh, Wh, Cp), image t*B + b, interior at [P:P+H, P:P+W], folded when kf > 1, rounded to bf16 (nearest even) when
    the slab is bf16; halo, slack and channels [kf*C, Cp) zero.  Exact."""
    x = np.asarray(x, np.float32)
    B, T, C, H, W = x.shape
    gH, gW, P, Hh, Wh = geom
    assert (gH, gW) == (H, W) and Cp >= kf * C
    f = _fold(x, kf).transpose(1, 0, 3, 4, 2).reshape(T * B, H, W, kf * C)
    out = np.zeros((T * B, Hh, Wh, Cp), np.float32)
    out[:, P:P + H, P:P + W, :kf * C] = bf16_round(f) if bf16 else f
    return out


def unpack_halo(slab, n0: int, N: int, C: int, geom) -> np.ndarray:
    """nint_unpack_halo: decoded slab (Nimg, Hh, Wh, Cp) -> (N, C, H, W) f32 of images [n0, n0 + N).  Exact."""
    H, W, P = geom[:3]
    return np.ascontiguousarray(np.asarray(slab, np.float32)[n0:n0 + N, P:P + H, P:P + W, :C].transpose(0, 3, 1, 2))


def pack_compact(x, Cp: int, bf16: bool = False) -> np.ndarray:
    """nint_pack_compact: (N, C, H, W) f32 -> (N, H, W, Cp) values, channel padding zero, bf16 rounded once.  Exact."""
    x = np.asarray(x, np.float32)
    N, C, H, W = x.shape
    out = np.zeros((N, H, W, Cp), np.float32)
    out[..., :C] = x.transpose(0, 2, 3, 1)
    return bf16_round(out) if bf16 else out


def unpack_compact(slab, C: int) -> np.ndarray:
    """nint_unpack_compact: decoded (N, H, W, Cp) -> (N, C, H, W) f32.  Exact."""
    return np.ascontiguousarray(np.asarray(slab, np.float32)[..., :C].transpose(0, 3, 1, 2))


def unfold_dx(G, C: int, k: int):
    """nint_unfold_dx: dx[n][c][y][x] = sum_kx G[n][y][x - kx + k//2][kx*C + c] over the taps inside the row, from the
    stored (decoded) G (N, H, W, Cp).  Returns (ref f64, bound): the kernel adds the k terms to a zero accumulator in f32,
    at most k roundings per term: ``gamma(k) sum |G|``."""
    G = np.asarray(G, np.float64)
    N, H, W, _ = G.shape
    ref, mag = np.zeros((N, C, H, W)), np.zeros((N, C, H, W))
    for kx in range(k):
        for x in range(W):
            xs = x - kx + k // 2
            if 0 <= xs < W:
                t = G[:, :, xs, kx * C:(kx + 1) * C].transpose(0, 2, 1)
                ref[:, :, :, x] += t
                mag[:, :, :, x] += np.abs(t)
    return ref, gamma(k) * mag


# --------------------------------------------------------------------------- preproc (exact)
def preproc(srcs, nstatic: int, mean, std, t0, T: int, Hp: int, Wp: int, mode: int) -> np.ndarray:
    """nint_preproc_fuse_pad_static_batch: srcs = records (steps, lev_i, H, W) f32, the last ``nstatic`` of them
    time-invariant ((1, lev_i, H, W), read at step 0); sample b reads steps [t0[b], t0[b] + T).  Output (B, T, C, Hp, Wp)
    f32, exact: ``(x - mean[cs]) / std[cs]`` in f32 (no fast-math: the division is correctly rounded, numpy's is too) with
    cs the SOURCE channel read:
      longitude: cyclic, xs = (xp - pl) mod W, pl = (Wp - W) // 2;
      latitude, pt = (Hp - H) // 2, pb = Hp - H - pt:  top halo row j < pt reads row 1 + j (mode 0) or pt - j (mode 1),
      bottom halo row j reads row H - pb - 1 + j (mode 0) or H - 2 - j (mode 1); in mode 0 the halo rows of channel c come
      from channel C - 1 - c, values, mean and std alike (the reference's np.fliplr on the channel axis)."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    srcs = [np.asarray(s, np.float32) for s in srcs]
    H, W = srcs[0].shape[2:]
    C = sum(s.shape[1] for s in srcs)
    B = len(t0)
    pl, pt = (Wp - W) // 2, (Hp - H) // 2
    pb = Hp - H - pt
    xs = (np.arange(Wp) - pl) % W
    ys, flip = np.zeros(Hp, np.int64), np.zeros(Hp, bool)
    for yp in range(Hp):
        if yp < pt:
            ys[yp], flip[yp] = (1 + yp, True) if mode == 0 else (pt - yp, False)
        elif yp < pt + H:
            ys[yp] = yp - pt
        else:
            j = yp - pt - H
            ys[yp], flip[yp] = (H - pb - 1 + j, True) if mode == 0 else (H - 2 - j, False)
    out = np.zeros((B, T, C, Hp, Wp), np.float32)
    cflip = np.arange(C)[::-1]
    for b in range(B):
        for t in range(T):
            fused = np.concatenate([s[0 if i >= len(srcs) - nstatic else t0[b] + t] for i, s in enumerate(srcs)], axis=0)
            z = (fused - mean[:, None, None]) / std[:, None, None]            # f32, z-scored before it is padded
            for yp in range(Hp):
                row = z[cflip, ys[yp]] if flip[yp] else z[:, ys[yp]]
                out[b, t, :, yp, :] = row[:, xs]
    return out


# --------------------------------------------------------------------------- evaluation: skill sums
SKILL_PIX, SKILL_SAMPLE = 5, 8     # include/nint.h NINT_SKILL_PIX / NINT_SKILL_SAMPLE


def skill_terms(pred, y, oy: int, ox: int, row_w=None):
    """The f64 terms of nint_skill_accum, each formed as csrc/head.hip documents it: ``p = (double)pred`` on the crop,
    ``t = (double)y``, ``d = p - t`` (one f64 subtraction), every product one f64 multiplication of its own.  pred
    (N, O, H, W) f32, y (N, O, Hc, Wc) f32, row_w (Hc) f64 or None (= 1).  Returns the map terms (SKILL_PIX, N, O, Hc, Wc)
    in the order of a slot's planes [t, p, t^2, p^2, d^2] and the sample terms (SKILL_SAMPLE, N, O, Hc, Wc) in the order
    of a sample row [d^2, |d|, t, t^2, p, p^2, rw t, rw p]."""
    pred, y = np.asarray(pred, np.float32), np.asarray(y, np.float32)
    Hc, Wc = y.shape[-2:]
    p = pred[:, :, oy:oy + Hc, ox:ox + Wc].astype(np.float64)
    t = y.astype(np.float64)
    if p.shape != t.shape:
        raise ValueError(f"crop {p.shape} against targets {t.shape}")
    rw = np.ones(Hc) if row_w is None else np.asarray(row_w, np.float64)
    rw = rw[None, None, :, None]
    d = p - t
    dd, tt, pp = d * d, t * t, p * p
    return np.stack([t, p, tt, pp, dd]), np.stack([dd, np.abs(d), t, tt, p, pp, rw * t, rw * p])


def _slots(slot, N: int):
    return np.zeros(N, np.int64) if slot is None else np.asarray(slot, np.int64)


def skill_sums(pred, y, oy: int, ox: int, slot, nslots: int, row_w, pix_before):
    """nint_skill_accum in f64 numpy.  slot: N ints in [-1, nslots) or None (all 0); pix_before (S, SKILL_PIX, O, Hc, Wc)
    f64 with S >= nslots (further slots are carried through untouched).  A map cell grows in the kernel's documented
    order -- the stored value, then the slot's samples n ascending, one f64 addition each -- so ``pix`` is what the kernel
    must return bit for bit on ANY data as long as every term is a single f64 operation; a sample row is numpy's sum
    over the crop (another order than the kernel's tree: equal only where the sums are exact).  Returns a dict:
    pix, sample (N, O, SKILL_SAMPLE); pix_abs, sample_abs = the sums of the addends' magnitudes (the stored value
    included); pix_n, sample_n = the number of addends (a stored value of exactly 0 adds no rounding and is not
    counted)."""
    mt, st = skill_terms(pred, y, oy, ox, row_w)
    N = mt.shape[1]
    sl = _slots(slot, N)
    if sl.shape != (N,) or sl.min() < -1 or sl.max() >= nslots:
        raise ValueError("slot")
    pix = np.array(pix_before, np.float64, copy=True)
    mag = np.abs(pix)
    cnt = (pix != 0).astype(np.int64)
    for n in range(N):
        if sl[n] >= 0:
            pix[sl[n]] = pix[sl[n]] + mt[:, n]
            mag[sl[n]] += np.abs(mt[:, n])
            cnt[sl[n]] += 1
    sample = st.sum(axis=(3, 4)).transpose(1, 2, 0)
    return {"pix": pix, "sample": np.ascontiguousarray(sample), "pix_abs": mag,
            "sample_abs": np.ascontiguousarray(np.abs(st).sum(axis=(3, 4)).transpose(1, 2, 0)), "pix_n": cnt,
            "sample_n": st.shape[3] * st.shape[4]}


def skill_head_pred(h, w, b) -> np.ndarray:
    """The prediction nint_head_skill_accum forms from h (N, Hc, Wc, Ch) -- the stored values on the crop -- w (O, Ch) and
    b (O) or None, for data on which every partial sum of the head is exact in f32 (skill_head_int_data): the f64 result
    IS the f32 one, whatever the order and whether or not a product is fused into its add.  Raises where that does not
    hold.  Returns (N, O, Hc, Wc) f32."""
    pred, _ = head_fwd(h, w, b)
    p32 = pred.astype(np.float32)
    mag = np.einsum("nyxc,oc->noyx", np.abs(np.asarray(h, np.float64)), np.abs(np.asarray(w, np.float64)))
    mag = mag + (0.0 if b is None else np.abs(np.asarray(b, np.float64))[None, :, None, None])
    # h integers and w, b multiples of 1/4: every product and every partial sum, in any order, is a multiple of 1/4 of
    # magnitude at most mag; below 2^24 / 4 all of them are f32 numbers, and a fused multiply-add rounds nothing either
    h64, w4 = np.asarray(h, np.float64), 4.0 * np.asarray(w, np.float64)
    b4 = np.zeros(1) if b is None else 4.0 * np.asarray(b, np.float64)
    if not (np.array_equal(h64, np.rint(h64)) and np.array_equal(w4, np.rint(w4)) and np.array_equal(b4, np.rint(b4))
            and 4.0 * float(mag.max()) < 2.0 ** 24):
        raise ValueError("the head's partial sums are not exact in f32 on this data")
    assert np.array_equal(p32.astype(np.float64), pred)
    return p32


def skill_audit(pred, y, oy: int, ox: int, slot, nslots: int, row_w, pix_before, pix_got, sample_got, what: str = "skill"):
    """Any-order audit of nint_skill_accum's results on arbitrary f32 data.  The error of every map cell and every sample
    row is taken against the EXACT sum of its f64 addends: ``math.fsum(addends + [-got])`` is the correctly rounded value of
    ``sum - got``, so the reference carries no rounding of its own.  Bound: ``gamma(n - 1, U64) * sum |addends|`` with n
    the number of addends -- a cell's non-zero stored value and the slot's samples, Hc * Wc for a sample row -- which holds
    for every summation order (Higham 4.4), tree, chain or split into calls alike; n <= 1 leaves no freedom: equality.
    Raises AuditError naming the worst element; returns (worst map ratio, worst row ratio)."""
    import math
    mt, st = skill_terms(pred, y, oy, ox, row_w)
    N, O = mt.shape[1:3]
    sl = _slots(slot, N)
    before = np.asarray(pix_before, np.float64)
    pix_got, sample_got = np.asarray(pix_got, np.float64), np.asarray(sample_got, np.float64)
    if pix_got.shape != before.shape or sample_got.shape != (N, O, SKILL_SAMPLE):
        raise AuditError(f"{what}: shapes {pix_got.shape} / {sample_got.shape}")
    worst = [0.0, 0.0]

    def one(addends, got, idx, k):
        n = len(addends)
        err = abs(math.fsum(addends + [-got])) if math.isfinite(got) else math.inf
        bound = gamma(max(n - 1, 0), U64) * math.fsum(abs(a) for a in addends)
        if err > bound:
            raise AuditError(f"{what}: {'map cell' if k == 0 else 'sample row'} {idx}: got {got!r}, exact sum "
                             f"{math.fsum(addends)!r}, |error| {err:.3e} over the bound {bound:.3e} of {n} addends")
        if err > 0:
            worst[k] = max(worst[k], err / bound)

    for s in range(before.shape[0]):
        members = [n for n in range(N) if sl[n] == s]
        if not members:
            check_equal(pix_got[s], before[s], f"{what}: slot {s} has no sample in the call")
            continue
        cols = mt[:, members].transpose(0, 2, 3, 4, 1).reshape(before[s].size, len(members)).tolist()
        b0, g0 = before[s].reshape(-1).tolist(), pix_got[s].reshape(-1).tolist()
        for i, (c, b, g) in enumerate(zip(cols, b0, g0)):
            one(([b] if b != 0 else []) + c, g, (s,) + tuple(int(j) for j in np.unravel_index(i, before.shape[1:])), 0)
    rows = st.transpose(1, 2, 0, 3, 4).reshape(N, O, SKILL_SAMPLE, -1)
    for n in range(N):
        for o in range(O):
            for k in range(SKILL_SAMPLE):
                one(rows[n, o, k].tolist(), float(sample_got[n, o, k]), (n, o, k), 1)
    return worst[0], worst[1]


def skill_slots(N: int) -> list:
    """slot[n] = (7 n mod 13) - 1: twelve slots in non-monotone order, and -1 (out of the maps) at n = 0, 13, ..."""
    return [(7 * n) % 13 - 1 for n in range(N)]


def skill_int_data(rng, N: int, O: int, H: int, W: int, oy: int, ox: int, Hc: int, Wc: int, S: int):
    """Data on which every skill sum is exact in ANY order: pred and y integer-valued f32 in [-8, 8] (pred NaN outside the
    crop window: never to be read), row_w = k / 8 with k in 1..16, pix_before integer-valued in [-1000, 1000].  Every
    addend is then a multiple of 1/8 and the magnitudes of a cell or row sum far below 2^53 / 8, so every partial sum is
    representable.  Returns (pred, y, row_w, pix_before (S, SKILL_PIX, O, Hc, Wc))."""
    pred = np.full((N, O, H, W), np.nan, np.float32)
    pred[:, :, oy:oy + Hc, ox:ox + Wc] = rng.integers(-8, 9, (N, O, Hc, Wc))
    y = rng.integers(-8, 9, (N, O, Hc, Wc)).astype(np.float32)
    row_w = rng.integers(1, 17, Hc).astype(np.float64) / 8.0
    before = rng.integers(-1000, 1001, (S, SKILL_PIX, O, Hc, Wc)).astype(np.float64)
    return pred, y, row_w, before


def skill_head_int_data(rng, n0: int, N: int, Ch: int, Chp: int, O: int, geom, oy: int, ox: int, Hc: int, Wc: int, bias=True):
    """A hidden-state slab and head on which nint_head_skill_accum is exact in any order, with or without FMA: h
    integer-valued in [-4, 4] (exact in bf16) on the crop window of images [n0, n0 + N), w = k / 4 with |k| <= 8, b an
    integer in [-8, 8]: every head partial sum is a multiple of 1/4 below 2^11.  Everything the kernel must not read is
    NaN -- the images below n0, the halo ring, the slack, the interior outside the crop window -- except the channel
    padding [Ch, Chp) of the crop's pixels, which is zero as every producer of a slab leaves it.  Returns (slab
    (n0 + N, Hh, Wh, Chp) f32 values, h (N, Hc, Wc, Ch) of the crop, w, b or None)."""
    H, W, P, Hh, Wh = geom
    slab = np.full((n0 + N, Hh, Wh, Chp), np.nan, np.float32)
    h = rng.integers(-4, 5, (N, Hc, Wc, Ch)).astype(np.float32)
    win = slab[n0:, P + oy:P + oy + Hc, P + ox:P + ox + Wc]
    win[..., :Ch] = h
    win[..., Ch:] = 0
    w = (rng.integers(-8, 9, (O, Ch)) / 4.0).astype(np.float32)
    b = rng.integers(-8, 9, O).astype(np.float32) if bias else None
    return slab, h, w, b
