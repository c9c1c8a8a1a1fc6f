"""Host-side f64 model of the guarded Adam step's control arithmetic (include/nint.h, ``nint_adam_flat_guarded``) and the
comparator of its ``state`` buffer (TEST INFRASTRUCTURE ONLY; numpy, no GPU).  Same conventions as ``oracle/small_audit.py``:
a comparator raises ``AuditError`` naming what is outside its bound and returns the largest ``error / bound`` it saw.

The arithmetic, all in f64, ``gs`` the f32 ``grad_scale`` as stored:
    S         = sum (double)g[i]^2
    norm      = gs * sqrt(S)
    coef      = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1         (torch.nn.utils.clip_grad_norm_; 1 for a NaN norm)
    s         = (float)(gs * coef)
    apply     = isfinite(S) or not skip_nonfinite
    step      = applied + 1;  step_size = (float)(lr / (1 - beta1^step));  sqrt_bc2 = (float)sqrt(1 - beta2^step)
    counters  applied += apply; skipped += !apply; clipped += finite and coef < 1; calls += 1;
              finite S: sum_norm += norm, finite += 1, max_norm = max(max_norm, norm)

Bounds (none comes from a run):
    S                    |S - fsum| <= n 2^-53 S: every square of an f32 is exact in f64, so what is left is a fixed-order sum of
                         n non-negative terms, at most n - 1 roundings of at most 2^-53 S each
    norm, coef, sum_norm 8 * 2^-52 relative to the f64 host value formed from the S read back: a handful of f64 operations
                         (sqrt, multiply, add, divide) at an ulp each
    s, step_size, sqrt_bc2   one f32 ulp of the host's cast (the device's f64 pow / sqrt / divide may sit an f64 ulp from the
                         host's, which can move the f32 rounding by one step, no more); coef == 1: s == gs exactly
    apply and the counters   exact
"""
from __future__ import annotations

import math

import numpy as np

from oracle import small_audit as SM

STATE = 16
(APPLIED, SKIPPED, CLIPPED, CALLS, SUM_NORM, FINITE, MAX_NORM, S_, NORM, COEF, SCALE, STEP_SIZE, SQRT_BC2, APPLY) = range(14)
REL64 = 8 * 2.0 ** -52


def sum_squares(g) -> float:
    """the exactly rounded f64 sum of the squares of f32 data (math.fsum; the squares are exact)"""
    g64 = np.asarray(g, np.float32).astype(np.float64).ravel()
    sq = g64 * g64
    if not np.isfinite(sq).all():
        return float("nan") if np.isnan(sq).any() else float("inf")
    return math.fsum(sq.tolist())


def control(S: float, gs, max_norm: float, skip_nonfinite: bool, applied: float, lr: float, beta1: float, beta2: float) -> dict:
    """the step's scalars in f64 from the sum of squares S"""
    gs = float(np.float32(gs))
    norm = gs * math.sqrt(S) if S >= 0 else float("nan")        # (sqrt of inf is inf, of NaN NaN)
    coef = 1.0
    if max_norm > 0:
        c = max_norm / (norm + 1e-6)
        coef = c if c < 1.0 else 1.0
    finite = math.isfinite(S)
    step = applied + 1.0
    return {"norm": norm, "coef": coef, "s": float(np.float32(gs * coef)), "finite": finite,
            "apply": finite or not skip_nonfinite, "step": step,
            "step_size": float(np.float32(lr / (1.0 - beta1 ** step))),
            "sqrt_bc2": float(np.float32(math.sqrt(1.0 - beta2 ** step)))}


def _close(got: float, ref: float, bound: float, what: str) -> float:
    if not (math.isfinite(got) and math.isfinite(ref)):
        if (math.isnan(got) and math.isnan(ref)) or got == ref:
            return 0.0
        raise SM.AuditError(f"{what}: got {got!r}, reference {ref!r}")
    err = abs(got - ref)
    if err == 0:
        return 0.0
    if not err <= bound:
        raise SM.AuditError(f"{what}: got {got!r}, reference {ref!r}, bound {bound!r} (ratio {err / bound if bound else math.inf:.3g})")
    return err / bound


def _ulp32(x: float) -> float:
    return float(np.spacing(np.abs(np.float32(x))))


def check_state(state, g, n: int, gs, max_norm: float, skip_nonfinite: bool, lr: float, beta1: float, beta2: float,
                before=None) -> float:
    """``state`` (NINT_OPT_STATE doubles read back after one call) against the model, from the gradient ``g[:n]`` the call
    read and the ``state`` it found (``before``; None = zeros).  Returns the largest error / bound."""
    st = np.asarray(state, np.float64)
    b4 = np.zeros(STATE) if before is None else np.asarray(before, np.float64)
    if st.shape != (STATE,) or b4.shape != (STATE,):
        raise SM.AuditError(f"state: shapes {st.shape} / {b4.shape}")
    gs = float(np.float32(gs))
    S_ref = sum_squares(np.asarray(g).ravel()[:n])
    S = float(st[S_])
    worst = _close(S, S_ref, n * 2.0 ** -53 * abs(S_ref), "S") if math.isfinite(S_ref) else 0.0
    if not math.isfinite(S_ref) and math.isfinite(S):
        raise SM.AuditError(f"S: got {S!r} for a gradient that is not finite")
    c = control(S, gs, max_norm, skip_nonfinite, float(b4[APPLIED]), lr, beta1, beta2)      # from the S read back
    worst = max(worst, _close(float(st[NORM]), c["norm"], REL64 * abs(c["norm"]), "norm"))
    worst = max(worst, _close(float(st[COEF]), c["coef"], REL64 * abs(c["coef"]), "coef"))
    if not float(st[COEF]) <= 1.0:
        raise SM.AuditError(f"coef: {float(st[COEF])!r} above 1")
    worst = max(worst, _close(float(st[SCALE]), c["s"], _ulp32(c["s"]), "s"))
    if float(st[COEF]) == 1.0 and float(st[SCALE]) != gs:
        raise SM.AuditError(f"s: coef == 1 but s = {float(st[SCALE])!r} is not grad_scale {gs!r}")
    worst = max(worst, _close(float(st[STEP_SIZE]), c["step_size"], _ulp32(c["step_size"]), "step_size"))
    worst = max(worst, _close(float(st[SQRT_BC2]), c["sqrt_bc2"], _ulp32(c["sqrt_bc2"]), "sqrt_bc2"))
    for k, name in ((SCALE, "s"), (STEP_SIZE, "step_size"), (SQRT_BC2, "sqrt_bc2")):
        if math.isfinite(st[k]) and float(np.float32(st[k])) != float(st[k]):
            raise SM.AuditError(f"{name}: {float(st[k])!r} is not an f32 value")
    apply, finite = c["apply"], c["finite"]
    clipped = finite and float(st[COEF]) < 1.0              # (the device's own coef: no disagreement at the boundary)
    exact = {APPLY: 1.0 if apply else 0.0, APPLIED: b4[APPLIED] + (1.0 if apply else 0.0),
             SKIPPED: b4[SKIPPED] + (0.0 if apply else 1.0), CLIPPED: b4[CLIPPED] + (1.0 if clipped else 0.0),
             CALLS: b4[CALLS] + 1.0, FINITE: b4[FINITE] + (1.0 if finite else 0.0),
             MAX_NORM: max(b4[MAX_NORM], float(st[NORM])) if finite else b4[MAX_NORM], 14: 0.0, 15: 0.0}
    names = {APPLY: "apply", APPLIED: "applied", SKIPPED: "skipped", CLIPPED: "clipped", CALLS: "calls", FINITE: "finite calls",
             MAX_NORM: "max_norm", 14: "state[14]", 15: "state[15]"}
    for k, want in exact.items():
        if float(st[k]) != float(want):
            raise SM.AuditError(f"{names[k]}: got {float(st[k])!r}, expected {float(want)!r}")
    want_sum = b4[SUM_NORM] + (c["norm"] if finite else 0.0)
    worst = max(worst, _close(float(st[SUM_NORM]), float(want_sum), REL64 * abs(want_sum), "sum of norms"))
    return worst
