"""Host-side f64 model of the configurable loss (include/nint.h, the ``_spec`` entries) and the cases its tests use (TEST
INFRASTRUCTURE ONLY; numpy / torch-CPU).  Shaped like ``tests/weighted_loss_model.py``: ``loss`` returns the dict that
``oracle/small_audit.py``'s comparators (``ratio``, ``check_stats``, ``check_loss_scalar``) take.

The arithmetic, per crop element with ``w = wgt[cy][cx]`` (1 without a map), ``q = ow[o]`` (1 without output weights; the
sequence form is the plain one on ``(B, T*O, H, W)`` with ``ow[t*O + o]``), ``Wd = (double)q * (double)w`` and ``d = p - y``
formed in f32:
    cnt   = N * osum * wsum        (osum: the f64 sum of the f32 ow, or O; wsum: the f64 sum of the f32 map, or Hc * Wc)
    H(d)  = 0.5 d^2 if |d| <= delta else delta (|d| - 0.5 delta);   C(d) = clamp(d, -delta, delta) by comparisons (NaN stays)
    loss  = a (S2 / cnt) + b (S1 / cnt) + c (SH / cnt), left to right, a term whose coefficient is 0 left OUT
    dpred = (float)(((a (2.0 d) + b sgn(d) + c C(d)) * (1.0 / cnt)) * Wd), f64, left to right, terms left out alike; +0 outside
            the crop and where Wd == 0 (such an element enters nothing: its target may be NaN)
    stats [0..4] += S2, S1, sum Wd y, sum Wd y^2, cnt; [5] += loss; [6] += the weighted R2 with Wd; [7] += 1"""
from __future__ import annotations

import numpy as np
import torch

import weighted_loss_model as WM
from oracle import small_audit as SM

f32 = np.float32
DELTA = 0.75                          # the cases' Huber threshold: exactly representable, d ~ N(0, 1) puts 55 % below it


class Spec:
    """coefficients, threshold and the f32 output weights (None: 1 everywhere) of one case"""

    def __init__(self, mse=1.0, l1=1.0, huber=0.0, delta=1.0, ow=None):
        self.a, self.b, self.c, self.delta = float(mse), float(l1), float(huber), float(delta)
        self.ow = None if ow is None else np.ascontiguousarray(ow, dtype=f32)

    @property
    def osum(self) -> float:
        """what the caller passes by value: the f64 sum of the vector as stored in f32"""
        return 0.0 if self.ow is None else float(self.ow.astype(np.float64).sum())

    def __repr__(self):
        return f"Spec({self.a}, {self.b}, {self.c}, delta={self.delta}, ow={None if self.ow is None else self.ow.tolist()})"


def seq_weights(step, out) -> np.ndarray:
    """the device vector of a sequence case: f32(step[t]) * f32(out[o]) rounded to f32, index t*O + o"""
    return (np.asarray(step, f32)[:, None] * np.asarray(out, f32)[None, :]).astype(f32).reshape(-1)


def cnt_of(N: int, O: int, sp: Spec, w, Hc: int, Wc: int) -> float:
    """N * (osum or O) * (wsum or Hc * Wc), left to right in f64 (nint.h)"""
    return float(N) * (sp.osum if sp.ow is not None else float(O)) * (WM.wsum_of(w) if w is not None else float(Hc) * Wc)


def weights_of(sp: Spec, w, O: int, Hc: int, Wc: int) -> np.ndarray:
    """Wd (O, Hc, Wc) f64 = (double)q * (double)w"""
    q = np.ones(O) if sp.ow is None else sp.ow.astype(np.float64)
    assert q.shape == (O,)
    wm = np.ones((Hc, Wc)) if w is None else np.asarray(w, f32).astype(np.float64)
    return q[:, None, None] * wm[None]


def huber(d64, delta: float):
    ad = np.abs(d64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(ad <= delta, (0.5 * d64) * d64, delta * (ad - 0.5 * delta))


def clamp(d64, delta: float):
    """dH/dd by comparisons: a NaN d fails both and stays NaN (np.clip / fmin / fmax would hide it)"""
    with np.errstate(invalid="ignore"):
        return np.where(d64 > delta, delta, np.where(d64 < -delta, -delta, d64))


def sgn(d64):
    """sign with sgn(0) = sgn(NaN) = 0: the kernels' (d > 0 ? 1 : (d < 0 ? -1 : 0))"""
    with np.errstate(invalid="ignore"):
        return np.where(d64 > 0, 1.0, np.where(d64 < 0, -1.0, 0.0))


def mix(sp: Spec, t2, t1, th):
    """a*t2 + b*t1 + c*th, left to right, a term whose coefficient is 0 left out (floats or arrays)"""
    out = None
    for co, t in ((sp.a, t2), (sp.b, t1), (sp.c, th)):
        if co != 0.0:
            out = co * t if out is None else out + co * t
    return out


def grad64(sp: Spec, d64, inv: float, Wd):
    """d loss / d pred in f64, the kernels' left-to-right expression (before the one rounding to f32)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (mix(sp, 2.0 * d64, sgn(d64), clamp(d64, sp.delta)) * inv) * Wd


def loss(pred, y, w, sp: Spec, oy: int, ox: int):
    """The spec loss of pred (N, O, H, W) f32 cropped to y (N, O, Hc, Wc) f32 at (oy, ox), map w (Hc, Wc) f32 or None:
    small_audit.loss's dict (dpred f32 -- bit-exact --, sums, abs, loss, r2, r2_tol) plus ``sh`` (the Huber sum) and
    ``dpred64``.  Every sum in f64 from d formed in f32."""
    pred, y = np.asarray(pred, f32), np.asarray(y, f32)
    N, O, H, W = pred.shape
    Hc, Wc = y.shape[2:]
    with np.errstate(invalid="ignore"):
        d = pred[:, :, oy:oy + Hc, ox:ox + Wc] - y                  # f32, the definition
    d64, y64 = d.astype(np.float64), y.astype(np.float64)
    Wd = np.broadcast_to(weights_of(sp, w, O, Hc, Wc)[None], d64.shape)
    cnt = cnt_of(N, O, sp, w, Hc, Wc)
    out = WM._sums(d64, y64, Wd, cnt)                               # s0..s3, their magnitudes, the weighted R2 and its tolerance
    live = Wd > 0
    with np.errstate(invalid="ignore", over="ignore"):
        sh = float(np.sum(np.where(live, Wd * huber(d64, sp.delta), 0.0))) if sp.c != 0.0 else 0.0
    s0, s1 = out["sums"][0], out["sums"][1]
    out["sh"] = sh
    with np.errstate(invalid="ignore"):
        out["loss"] = float(mix(sp, s0 / cnt, s1 / cnt, sh / cnt))
    g = np.where(live, grad64(sp, d64, 1.0 / cnt, Wd), 0.0)
    dp64 = np.zeros(pred.shape)
    dp64[:, :, oy:oy + Hc, ox:ox + Wc] = g
    out["dpred64"] = dp64
    with np.errstate(over="ignore", invalid="ignore"):
        out["dpred"] = dp64.astype(f32)
    return out


def loss_torch(pred, y, w, sp: Spec, oy: int, ox: int):
    """the same loss as a torch expression (any dtype, autograd): what the oracle fit loop minimises.  pred (N, O, H, W)
    -- the sequence form is (B, T*O, H, W) with sp.ow over t*O + o --, y anything that reshapes to (N, O, Hc, Wc)."""
    Hc, Wc = y.shape[-2], y.shape[-1]
    N, O = pred.shape[0], pred.shape[1]
    Wt = torch.as_tensor(weights_of(sp, w, O, Hc, Wc)).to(pred.dtype)
    d = pred[..., oy:oy + Hc, ox:ox + Wc] - y.reshape(N, O, Hc, Wc)
    d = torch.where(Wt > 0, d, torch.zeros_like(d))                 # an element of weight 0 enters nothing, NaN target or not
    cnt = cnt_of(N, O, sp, w, Hc, Wc)
    ad = d.abs()
    hub = torch.where(ad <= sp.delta, 0.5 * d * d, sp.delta * (ad - 0.5 * sp.delta))
    return mix(sp, (Wt * d * d).sum() / cnt, (Wt * ad).sum() / cnt, (Wt * hub).sum() / cnt)


def head_loss_fused(h, wh, b, y, w, sp: Spec, oy: int, ox: int):
    """The fused head + spec loss pass in f64 from the stored h (N, H, W, Ch): pred = wh . h + b, d = pred - y on the crop,
    dpred (0 outside the crop and under a zero weight), dh = wh^T dpred (N, H, W, Ch).  Returns (dpred, dh, loss)."""
    y64 = np.asarray(y, f32).astype(np.float64)
    pred, _ = SM.head_fwd(h, wh, b)
    N, O, H, W = pred.shape
    Hc, Wc = y64.shape[2:]
    cnt = cnt_of(N, O, sp, w, Hc, Wc)
    crop = (slice(None), slice(None), slice(oy, oy + Hc), slice(ox, ox + Wc))
    Wd = np.broadcast_to(weights_of(sp, w, O, Hc, Wc)[None], y64.shape)
    with np.errstate(invalid="ignore"):
        d = np.where(Wd > 0, pred[crop] - y64, 0.0)
    dp = np.zeros_like(pred)
    dp[crop] = grad64(sp, d, 1.0 / cnt, Wd)
    dh = np.einsum("noyx,oc->nyxc", dp, np.asarray(wh, np.float64))
    s2, s1 = float(np.sum(Wd * d * d)), float(np.sum(Wd * np.abs(d)))
    sh = float(np.sum(Wd * huber(d, sp.delta)))
    return dp, dh, float(mix(sp, s2 / cnt, s1 / cnt, sh / cnt))


# --------------------------------------------------------------------------- the cases
MIXES = {"mse": (1.0, 0.0, 0.0), "l1": (0.0, 1.0, 0.0), "huber": (0.0, 0.0, 1.0), "mix": (0.5, 2.0, 1.5), "default": (1.0, 1.0, 0.0)}
STEP_W = np.array([0.0, 0.5, 1.0], f32)              # T = 3: the first step dropped, the second discounted


def output_weights(O: int) -> np.ndarray:
    """The cases' f32 output weights: values that are not powers of two, every third output (from the second) switched off, so
    that at least half stay on; a single output cannot be switched off and carries 0.75."""
    q = (0.75 + 0.375 * (np.arange(O) % 5)).astype(f32)
    q[1::3] = 0.0
    assert 2 * int((q > 0).sum()) >= O and (O < 2 or (q == 0).any()), (O, q)
    return q


def build_case(shape, seed: int, with_map: bool, with_ow: bool, mix_name: str = "mix", delta: float = DELTA, steps: int = 0):
    """One case of the plain entry: pred (N, O, H, W), y (N, O, Hc, Wc) with d ~ N(0, 1), the map of weighted_loss_model.wmap or
    None, a Spec (``steps`` = T > 0: O = T * O' and the weights are seq_weights(STEP_W, output_weights(O'))), and the planted
    elements.  Asserts that no such case can pass for a trivial reason:
      * each Huber branch holds at least 20 % of the live elements;
      * at least half of the outputs (and of the steps) keep a weight, and -- wherever there are two or more -- at least one
        of each is zero;
      * on live elements there are d == +delta and d == -delta exactly in f32, d == +0, and d one ulp above delta."""
    N, O, H, W, oy, ox, Hc, Wc = shape
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(f32)
    pred = rng.standard_normal((N, O, H, W)).astype(f32)
    d = rng.standard_normal((N, O, Hc, Wc)).astype(f32)
    pred[:, :, oy:oy + Hc, ox:ox + Wc] = y + d
    w = WM.wmap(Hc, Wc) if with_map else None
    ow = None
    if with_ow:
        if steps:
            assert O % steps == 0 and steps == STEP_W.shape[0]
            ow = seq_weights(STEP_W, output_weights(O // steps))
            assert 2 * int((STEP_W > 0).sum()) >= steps and (STEP_W == 0).any()
        else:
            ow = output_weights(O)
    sp = Spec(*MIXES[mix_name], delta=delta, ow=ow)
    Wd = weights_of(sp, w, O, Hc, Wc)
    # the planted elements: the first four live cells of the first live output, sample 0
    o_live = int(np.argmax(Wd.reshape(O, -1).max(axis=1) > 0))
    cells = np.argwhere(Wd[o_live] > 0)[:4]
    assert len(cells) == 4
    above = np.nextafter(f32(delta), f32(np.inf))
    plant = {"plus": (0.25, 1.0), "minus": (0.25, -0.5), "zero": (0.25, 0.25), "above": (-0.25, float(f32(-0.25) + above))}
    assert delta == 0.75 or not plant                                # (the planted values are written for delta = 0.75)
    where = {}
    for (name, (yv, pv)), (cy, cx) in zip(plant.items(), cells):
        y[0, o_live, cy, cx], pred[0, o_live, oy + cy, ox + cx] = yv, pv
        where[name] = (0, o_live, int(cy), int(cx))
    dd = pred[:, :, oy:oy + Hc, ox:ox + Wc] - y
    g = lambda k: dd[where[k]]
    assert g("plus") == f32(delta) and g("minus") == f32(-delta) and g("zero") == 0 and not np.signbit(g("zero"))
    assert g("above") == above and above > delta
    live = np.broadcast_to(Wd[None] > 0, dd.shape)
    quad = float((np.abs(dd[live]) <= delta).mean())
    assert 0.2 <= quad <= 0.8, quad                                  # both Huber branches hold >= 20 % of the live elements
    return {"pred": pred, "y": y, "w": w, "spec": sp, "where": where, "shape": shape}


# the plain entry's shapes (N, O, H, W, oy, ox, Hc, Wc): an asymmetric crop, one full image, and more elements than the
# 256 x 1024 threads of one pass (the grid-stride loop runs)
PLAIN_SHAPES = [(2, 3, 12, 20, 2, 3, 7, 13), (1, 1, 9, 9, 0, 0, 9, 9), (2, 5, 168, 160, 4, 8, 150, 140)]
SEQ_SHAPE = (2, 9, 12, 20, 1, 2, 10, 16)             # the sequence form: B = 2, T = 3, O = 3 as (B, T*O, H, W)
# (mix, map, output weights): each single term, the mix of all three, with and without map and output weights
PLAIN_CASES = [("mse", False, False), ("l1", True, False), ("huber", False, True), ("mix", True, True), ("mix", False, False)]
SEED = 70


def plain_cases():
    """every (shape, mix, map, ow, steps) the GPU test of the plain entry runs, the sequence form (step weights) last"""
    out = [(s, m, wm, ow, 0) for s in PLAIN_SHAPES for m, wm, ow in PLAIN_CASES]
    return out + [(SEQ_SHAPE, "mix", True, True, 3), (SEQ_SHAPE, "huber", False, True, 3)]
