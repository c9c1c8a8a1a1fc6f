"""Host-side f64 model of the grouped AdamW step (include/nint.h, ``nint_adam_flat_groups[_guarded]``) and the comparator of
its result (TEST INFRASTRUCTURE ONLY; numpy, no GPU).  Same conventions as ``tests/grad_clip_model.py``.

The arithmetic per element i of group k = (begin, end, lr, wd), all in f64 from the f32 values stored before the step:
    d    = (float)(1 - lr * wd)                         the decay multiplier, rounded to f32 once (1.0 without decay)
    p    = p * d                                        torch.optim.AdamW's ``param.mul_(1 - lr * weight_decay)``
    g'   = g * grad_scale
    m'   = m + (1 - beta1) (g' - m);   v' = beta2 v + (1 - beta2) g'^2
    p'   = p - (lr / (1 - beta1^step)) m' / (sqrt(v') / sqrt(1 - beta2^step) + eps)
Elements in no group keep p, m and v.

Bounds (none comes from a run): the device forms pd = fl32(p * d) with ONE f32 multiply -- an exactly rounded product, which
the host reproduces bit for bit -- and then runs nint_adam_flat's element update on pd.  So per group the Adam audit of
``oracle/small_audit.py`` applies to (pd, g, m, v) with its own running bounds, and the reference moves from pd to the
unrounded product: one half-ulp of pd, the "one half-ulp term for the decay multiply".  m and v never see the decay.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import small_audit as SM

f32, f64 = np.float32, np.float64


def decay_multiplier(lr: float, wd: float) -> float:
    """(float)(1 - lr * wd) as an f64 value"""
    return float(f32(1.0 - lr * wd))


def grouped_adamw(p, g, m, v, groups, beta1: float, beta2: float, eps: float, step: int, grad_scale: float = 1.0):
    """One grouped step in f64: new (p, m, v) as f64 arrays.  ``groups``: [(begin, end, lr, wd)]."""
    p, g, m, v = (np.asarray(a, f32).astype(f64).copy() for a in (p, g, m, v))
    gs = float(f32(grad_scale))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    for b, e, lr, wd in groups:
        s = slice(b, e)
        pd = p[s] * decay_multiplier(lr, wd)
        gr = g[s] * gs
        m[s] = m[s] + (1.0 - beta1) * (gr - m[s])
        v[s] = beta2 * v[s] + (1.0 - beta2) * gr * gr
        p[s] = pd - (lr / bc1) * m[s] / (np.sqrt(v[s]) / math.sqrt(bc2) + eps)
    return p, m, v


def check_table(groups, n: int):
    """the table's own rules (nint.h): sorted, non-empty, tiling one range inside [0, n)"""
    assert groups and groups[0][0] >= 0 and groups[-1][1] <= n
    for k, (b, e, lr, wd) in enumerate(groups):
        assert e > b and (k == 0 or b == groups[k - 1][1]) and lr >= 0 and wd >= 0


def audit(after, before, groups, beta1: float, beta2: float, eps: float, step: int, grad_scale: float, step_sizes=None,
          what: str = "") -> float:
    """``after`` = (p, m, v) read back, ``before`` = (p, g, m, v) as stored before the call.  Inside every group: within the
    Adam audit's bound around the f64 AdamW value; outside the groups: bit-unchanged.  ``grad_scale``: the scale the body
    used (the device's s for a guarded step).  Returns the worst error / bound; raises SM.AuditError."""
    p0, g0, m0, v0 = (np.asarray(a, f32) for a in before)
    n = p0.size
    check_table(groups, n)
    inside = np.zeros(n, bool)
    worst = 0.0
    for k, (b, e, lr, wd) in enumerate(groups):
        s = slice(b, e)
        inside[s] = True
        d = decay_multiplier(lr, wd)
        exact = p0[s].astype(f64) * d                    # (a product of two f32 values: exact in f64)
        pd = exact.astype(f32)                           # the device's one rounding
        ref = SM.adam(pd, g0[s], m0[s], v0[s], lr, beta1, beta2, eps, step, grad_scale)
        for a, key in zip(after, "pmv"):
            r, bound = ref[key]
            if key == "p":
                r = r + (exact - pd.astype(f64))         # AdamW's value starts from the unrounded product ...
                bound = bound + 0.5 * np.spacing(np.abs(pd)).astype(f64)      # ... half an ulp of pd away
            err = np.abs(np.asarray(a, f32)[s].astype(f64) - r)
            # (the margin of tests/test_gpu_grad_clip.py for a guarded step's device-side f64 pow / sqrt / divide)
            bad = ~(err <= bound * (1.0 + 2.0 ** -20))
            ratio = float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))))
            worst = max(worst, ratio)
            if bad.any():
                i = int(np.argmax(bad))
                raise SM.AuditError(f"{what}: group {k} {key}[{b + i}]: got {np.asarray(a, f32)[s][i]!r}, reference {r[i]!r}, "
                                    f"bound {bound[i]!r}")
    for a, b0, key in zip(after, (p0, m0, v0), "pmv"):
        SM.check_equal(np.asarray(a, f32)[~inside], b0[~inside], f"{what}: {key} outside the groups")
    return worst
