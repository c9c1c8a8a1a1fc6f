"""The training loss as a per-cell weighted mean: cos-latitude area weights, masks, or their product.

The fit loop minimises ``mean((y-p)^2) + mean(|y-p|)`` over the crop (reference train.py:102,105).  On a regular lat-lon
grid that gives a polar row the weight of an equatorial row with many times its area, and it cannot leave out cells
without valid data.  With a weight map ``w`` (f32, ``(Hc, Wc)``, non-negative, shared by every sample, output and time
step) the loss is

    loss = sum(w * d^2) / cnt + sum(w * |d|) / cnt,    d = p - y,    cnt = N * O * sum(w)

and a cell of weight 0 is skipped: its target may be NaN.  ``include/nint.h`` (the ``_weighted`` entries) carries the exact
arithmetic.  Three ways in: ``FusedTrainer(loss_weights=...)`` (the fused step), ``CropMSEL1Loss`` (an ``nn.Module`` for a
torch training loop) and ``train.py --lat-weighted-loss / --loss-weights``.

Under data parallelism the map is NOT broadcast: every rank has to be given the same one (``train.py`` builds it
deterministically on every rank).

``LossSpec`` opens the other three axes of that loss -- which penalty, which output, which step:

    loss = mse * mean_w(d^2) + l1 * mean_w(|d|) + huber * mean_w(HuberLoss_delta(d))

a weighted mean whose weight is the product of the cell's (the map above), the output's (``output_weights``) and, with the
sequence loss, the step's (``step_weights``: spin-up steps discounted or dropped).  A coefficient of 0 takes its term out, a
weight of 0 its element (a NaN target is harmless there).  ``include/nint.h`` (the ``_spec`` entries) carries the exact
arithmetic.  Ways in: ``FusedTrainer(loss=LossSpec(...))``, ``CropLoss`` and ``train.py --loss-mix / --huber-delta /
--output-weights / --spinup-steps``.  Like the map, a spec is NOT broadcast between data-parallel ranks: every rank has to be
given the same one (``train.py`` builds it from the command line on every rank)."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import NINT_LOSS_SCRATCH_FLOATS, NINT_LOSS_SPEC_SCRATCH_FLOATS, check, ptr, stream_ptr

__all__ = ["grid_latitudes", "cos_latitude_weights", "validate_loss_weights", "CropMSEL1Loss", "LossSpec", "CropLoss", "EnsembleLoss"]


def grid_latitudes(H: int) -> np.ndarray:
    """Cell-centre latitudes in degrees of the ``H`` rows of a global grid, south to north (f64)."""
    return -90.0 + (np.arange(H) + 0.5) * (180.0 / H)


def cos_latitude_weights(lat_degrees, Wc: Optional[int] = None) -> np.ndarray:
    """``cos(deg2rad(lat))`` as f32: the ``(Hc,)`` row weights, or with ``Wc`` the ``(Hc, Wc)`` map (rows broadcast)."""
    row = np.cos(np.deg2rad(np.asarray(lat_degrees, np.float64))).astype(np.float32)
    if row.ndim != 1:
        raise ValueError("lat_degrees must be a vector of row latitudes")
    return row if Wc is None else np.ascontiguousarray(np.broadcast_to(row[:, None], (row.shape[0], int(Wc))))


def validate_loss_weights(weights, crop: Optional[Tuple[int, int]] = None) -> Tuple[np.ndarray, Optional[float]]:
    """Host-side check of a weight map.  ``weights``: ``(Hc, Wc)`` array or tensor, or a ``(Hc,)`` vector of row weights.
    Returns ``(w, wsum)``: the f32 array -- a vector stays a vector until ``crop = (Hc, Wc)`` is known and is then expanded
    to rows -- and the f64 sum of the f32 map (None while it is still a vector).  ValueError for a negative, NaN or inf
    value, an all-zero map, more than two dimensions or a shape that does not match ``crop``."""
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w64 = np.asarray(weights, np.float64)
    if w64.ndim not in (1, 2) or w64.size == 0:
        raise ValueError(f"loss weights must be (Hc, Wc) or (Hc,), got shape {w64.shape}")
    if not np.isfinite(w64).all():
        raise ValueError("loss weights must be finite (mask a cell with weight 0, not NaN)")
    if (w64 < 0).any():
        raise ValueError("loss weights must be non-negative")
    with np.errstate(over="ignore"):
        w = w64.astype(np.float32)
    if not np.isfinite(w).all():
        raise ValueError("loss weights overflow f32")
    if not (w > 0).any():
        raise ValueError("loss weights are all zero: nothing to fit")
    if crop is not None:
        Hc, Wc = int(crop[0]), int(crop[1])
        if w.ndim == 1:
            if w.shape[0] != Hc:
                raise ValueError(f"{w.shape[0]} row weights for a crop of {Hc} rows")
            w = np.broadcast_to(w[:, None], (Hc, Wc))
        elif w.shape != (Hc, Wc):
            raise ValueError(f"loss weights {w.shape} do not match the target's crop {(Hc, Wc)}")
    w = np.ascontiguousarray(w)
    return w, (float(w.astype(np.float64).sum()) if w.ndim == 2 else None)


class DeviceWeights:
    """A validated map on its way to the device: the f32 ``(Hc, Wc)`` tensor and the f64 ``wsum``, formed at the first call
    that knows the crop and the device (a ``(Hc,)`` vector is expanded there)."""

    def __init__(self, weights):
        self.host, _ = validate_loss_weights(weights)
        self.map: Optional[torch.Tensor] = None
        self.wsum: Optional[float] = None

    def on(self, device, Hc: int, Wc: int) -> Tuple[torch.Tensor, float]:
        if self.map is None or self.map.device != device or tuple(self.map.shape) != (Hc, Wc):
            w, wsum = validate_loss_weights(self.host, (Hc, Wc))
            self.map = torch.from_numpy(w).to(device)
            self.wsum = wsum
        return self.map, self.wsum


def crop_loss_launch(pred, y, dpred, scratch, stats, N, O, H, W, oy, ox, Hc, Wc, weights=None, spec=None):
    """The stand-alone loss launch on device tensors, and the one place that chooses its entry: ``nint_loss_crop_spec``
    with a ``spec`` (a _lib.NintLossSpec; ``scratch`` then of NINT_LOSS_SPEC_SCRATCH_FLOATS floats), else
    ``nint_loss_mse_l1_crop_weighted`` with ``weights = (wgt, wsum)``, else ``nint_loss_mse_l1_crop``.  ``dpred`` and
    ``stats`` may be None."""
    wgt, wsum = weights if weights is not None else (None, 0.0)
    if spec is not None:
        name, extra = "nint_loss_crop_spec", (ptr(wgt), wsum, C.byref(spec))
    elif weights is not None:
        name, extra = "nint_loss_mse_l1_crop_weighted", (ptr(wgt), wsum)
    else:
        name, extra = "nint_loss_mse_l1_crop", ()
    check(getattr(_lib.load(), name)(ptr(pred), ptr(y), *extra, ptr(dpred), ptr(scratch), ptr(stats), N, O, H, W, oy, ox, Hc, Wc,
                                     stream_ptr()), name)


class _CropLoss(torch.autograd.Function):
    """crop_loss_launch as an autograd function: ``spec`` None runs the MSE + L1 entries, with or without the map"""

    @staticmethod
    def forward(ctx, pred, y, wgt, wsum, spec, oy, ox):
        N, O, H, W = pred.shape
        Hc, Wc = y.shape[-2], y.shape[-1]
        p = pred.detach().float().contiguous()
        yv = y.detach().float().contiguous()
        if yv.numel() != N * O * Hc * Wc:
            raise ValueError(f"target {tuple(y.shape)} does not match the prediction {tuple(pred.shape)}")
        scratch = torch.empty(NINT_LOSS_SCRATCH_FLOATS if spec is None else NINT_LOSS_SPEC_SCRATCH_FLOATS, dtype=torch.float32,
                              device=p.device)
        dpred = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        crop_loss_launch(p, yv, dpred, scratch, None, N, O, H, W, oy, ox, Hc, Wc, None if wgt is None else (wgt, wsum), spec)
        ctx.dpred = dpred
        ctx.dtype = pred.dtype
        return scratch[0].clone()

    @staticmethod
    def backward(ctx, upstream):
        g = None if ctx.dpred is None else (ctx.dpred * upstream).to(ctx.dtype)
        return g, None, None, None, None, None, None


class CropMSEL1Loss(torch.nn.Module):
    """``MSELoss + L1Loss`` of the reference fit loop (train.py:102,105) with the crop inside and an optional weight map, for
    users who keep a torch training loop: ``loss = criterion(y, pred)`` -- the reference's argument order -- with the
    UNCROPPED ``pred (B, O, H, W)`` on the device and ``y (B, [O,] Hc, Wc)``.  The crop window starts at ``halo = (oy, ox)``.
    The forward is one loss launch (``nint_loss_mse_l1_crop_weighted`` with a map, ``nint_loss_mse_l1_crop`` without), which
    also writes d loss / d pred; backward returns that times the upstream gradient.  ``y`` receives NO gradient.
    ``weights``: see ``validate_loss_weights``; every data-parallel rank must be given the same map."""

    def __init__(self, halo: Tuple[int, int] = (5, 5), weights=None):
        super().__init__()
        self.halo = (int(halo[0]), int(halo[1]))
        self._weights = None if weights is None else DeviceWeights(weights)

    def forward(self, y: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
        if pred.dim() != 4 or pred.device.type != "cuda":
            raise _lib.NintError("CropMSEL1Loss needs the uncropped prediction (B, O, H, W) on the MI355X (cuda)")
        wgt, wsum = (None, 0.0) if self._weights is None else self._weights.on(pred.device, y.shape[-2], y.shape[-1])
        return _CropLoss.apply(pred, y, wgt, wsum, None, self.halo[0], self.halo[1])


def _weight_vector(values, what: str) -> np.ndarray:
    """a vector of output or step weights as f32: finite, non-negative, not all zero (ValueError otherwise)"""
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    v64 = np.asarray(values, np.float64)
    if v64.ndim != 1 or v64.size == 0:
        raise ValueError(f"{what} must be a vector, got shape {v64.shape}")
    if not np.isfinite(v64).all():
        raise ValueError(f"{what} must be finite (switch an entry off with weight 0, not NaN)")
    if (v64 < 0).any():
        raise ValueError(f"{what} must be non-negative")
    with np.errstate(over="ignore"):
        v = v64.astype(np.float32)
    if not np.isfinite(v).all():
        raise ValueError(f"{what} overflow f32")
    if not (v > 0).any():
        raise ValueError(f"{what} are all zero: nothing to fit")
    return np.ascontiguousarray(v)


class LossSpec:
    """The configurable training loss (``nint_loss_spec``): ``mse * MSE + l1 * L1 + huber * HuberLoss(delta)`` as weighted
    means over the crop, with a weight per output (``output_weights``, shape ``(O,)``) and, under the sequence loss, per step
    (``step_weights``, shape ``(T,)``).  The default ``LossSpec()`` is the reference's ``MSELoss + L1Loss``.

    Validated here on the host -- ValueError for a negative, NaN or inf coefficient, all coefficients zero, a ``delta`` that
    is not finite and > 0 while ``huber`` is on, weights that are negative, non-finite or all zero; the lengths against ``O``
    and ``T`` at the first call that knows them.  Both vectors are stored as f32; the device vector is
    ``f32(step[t]) * f32(out[o])`` rounded to f32 on the host (index ``t*O + o``; the outputs alone without the sequence
    loss), and ``osum`` the f64 sum of that stored vector.  ``step_weights`` without the sequence loss is a ValueError.
    Not broadcast between data-parallel ranks: every rank must be given the same spec."""

    def __init__(self, mse: float = 1.0, l1: float = 1.0, huber: float = 0.0, delta: float = 1.0, output_weights=None,
                 step_weights=None):
        self.mse, self.l1, self.huber, self.delta = float(mse), float(l1), float(huber), float(delta)
        for name in ("mse", "l1", "huber"):
            v = getattr(self, name)
            if not math.isfinite(v) or v < 0:
                raise ValueError(f"loss coefficient {name} = {v!r}: must be finite and >= 0")
        if self.mse == 0 and self.l1 == 0 and self.huber == 0:
            raise ValueError("all loss coefficients are zero: nothing to fit")
        if self.huber != 0 and not (math.isfinite(self.delta) and self.delta > 0):
            raise ValueError(f"huber delta = {self.delta!r}: must be finite and > 0")
        self.output_weights = None if output_weights is None else _weight_vector(output_weights, "output weights")
        self.step_weights = None if step_weights is None else _weight_vector(step_weights, "step weights")
        self._key = None
        self._vec: Optional[torch.Tensor] = None
        self._c = None

    def host_vector(self, O: int, T: Optional[int] = None) -> Optional[np.ndarray]:
        """The weight vector the device reads, f32: ``(O,)`` for a last-step loss (``T`` None), ``(T*O,)`` with index
        ``t*O + o`` for the sequence loss; None when neither kind of weight is set.  Checks the lengths."""
        if self.step_weights is not None and T is None:
            raise ValueError("step_weights need the sequence loss (a target at every step of the window)")
        if self.output_weights is not None and self.output_weights.shape[0] != O:
            raise ValueError(f"{self.output_weights.shape[0]} output weights for {O} outputs")
        if self.step_weights is not None and self.step_weights.shape[0] != T:
            raise ValueError(f"{self.step_weights.shape[0]} step weights for a window of {T} steps")
        if self.output_weights is None and self.step_weights is None:
            return None
        out = self.output_weights if self.output_weights is not None else np.ones(O, np.float32)
        if T is None:
            return out
        step = self.step_weights if self.step_weights is not None else np.ones(T, np.float32)
        vec = np.ascontiguousarray((step[:, None] * out[None, :]).astype(np.float32).reshape(-1))   # f32 * f32, rounded to f32
        if not np.isfinite(vec).all() or not (vec > 0).any():
            raise ValueError("the products of step and output weights overflow f32 or are all zero")
        return vec

    def on(self, device, O: int, T: Optional[int] = None):
        """the ``nint_loss_spec`` for a call with ``O`` outputs (and ``T`` steps under the sequence loss) on ``device``"""
        key = (str(device), int(O), None if T is None else int(T))
        if self._key != key:
            vec = self.host_vector(int(O), None if T is None else int(T))
            c = _lib.NintLossSpec()
            c.mse, c.l1, c.huber, c.delta = self.mse, self.l1, self.huber, self.delta
            if vec is None:
                self._vec, c.ow, c.now, c.osum = None, None, 0, 0.0
            else:
                self._vec = torch.from_numpy(vec).to(device)
                c.ow, c.now, c.osum = self._vec.data_ptr(), vec.shape[0], float(vec.astype(np.float64).sum())
            self._c, self._key = c, key
        return self._c

    def __repr__(self):
        return (f"LossSpec(mse={self.mse}, l1={self.l1}, huber={self.huber}, delta={self.delta}, "
                f"output_weights={None if self.output_weights is None else self.output_weights.tolist()}, "
                f"step_weights={None if self.step_weights is None else self.step_weights.tolist()})")


class CropLoss(torch.nn.Module):
    """``CropMSEL1Loss`` with the configurable loss: ``loss = criterion(y, pred)`` with the UNCROPPED ``pred (B, O, H, W)`` on
    the device and ``y (B, [O,] Hc, Wc)``; ``spec`` a ``LossSpec`` (None: the default mix, MSE + L1) and ``weights`` the
    optional per-cell map.  The forward is ONE launch of ``nint_loss_crop_spec``, which also writes d loss / d pred;
    backward returns that times the upstream gradient.  ``y`` receives NO gradient.  A spec with ``step_weights`` is refused
    (ValueError): one prediction has no steps.  Every data-parallel rank must be given the same spec and map."""

    def __init__(self, halo: Tuple[int, int] = (5, 5), spec: Optional[LossSpec] = None, weights=None):
        super().__init__()
        self.halo = (int(halo[0]), int(halo[1]))
        if spec is not None and not isinstance(spec, LossSpec):
            raise TypeError("spec must be a LossSpec or None")
        self.spec = LossSpec() if spec is None else spec
        self._weights = None if weights is None else DeviceWeights(weights)

    def forward(self, y: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
        if pred.dim() != 4 or pred.device.type != "cuda":
            raise _lib.NintError("CropLoss needs the uncropped prediction (B, O, H, W) on the MI355X (cuda)")
        wgt, wsum = (None, 0.0) if self._weights is None else self._weights.on(pred.device, y.shape[-2], y.shape[-1])
        return _CropLoss.apply(pred, y, wgt, wsum, self.spec.on(pred.device, pred.shape[1]), self.halo[0], self.halo[1])


class EnsSpecOn(NamedTuple):
    """EnsembleLoss.on: what SeqEngine.ens_loss takes -- alpha, the (rows, O) output-weight table on the device and its host copy"""
    alpha: float
    ow: Optional[torch.Tensor]
    ow_host: Optional[np.ndarray]


class EnsembleLoss:
    """The training loss of an ensemble (``nint_ens_loss``): the almost-fair CRPS over the M member lanes of a
    sample,

        loss = mean_w( (1/M) sum_i |x_i - y|  -  (M - 1 + alpha) / (M^2 (M - 1)) sum_{i<j} |x_i - x_j| )

    ``alpha = 1`` is the fair CRPS (unbiased in M), ``alpha = 0`` the plain one, in between the "almost fair" mix that keeps a
    member from drifting freely.  ``output_weights`` (O,) and, with the sequence loss, ``step_weights`` (T,) weight the terms as
    in ``LossSpec``: the device table is ``f32(step[t]) * f32(out[o])`` rounded to f32, one row per step.  Validated here on the
    host (ValueError: alpha outside [0, 1] or not finite; weights negative, non-finite or all zero); the lengths at the first
    call that knows O and T.  Not broadcast between data-parallel ranks."""

    def __init__(self, alpha: float = 1.0, output_weights=None, step_weights=None):
        self.alpha = float(alpha)
        if not (math.isfinite(self.alpha) and 0.0 <= self.alpha <= 1.0):
            raise ValueError(f"EnsembleLoss: alpha = {alpha!r} must lie in [0, 1]")
        self.output_weights = None if output_weights is None else _weight_vector(output_weights, "output weights")
        self.step_weights = None if step_weights is None else _weight_vector(step_weights, "step weights")
        self._key, self._on = None, None

    def host_table(self, O: int, T: Optional[int] = None) -> Optional[np.ndarray]:
        """the f32 table the device reads: (1, O) for the last-step loss (``T`` None), (T, O) for the sequence loss; None when
        no weight is set.  Checks the lengths (LossSpec.host_vector's rules)."""
        vec = LossSpec(output_weights=self.output_weights, step_weights=self.step_weights).host_vector(O, T)
        return None if vec is None else np.ascontiguousarray(vec.reshape(1 if T is None else T, O))

    def on(self, device, O: int, T: Optional[int] = None) -> EnsSpecOn:
        key = (str(device), int(O), None if T is None else int(T))
        if self._key != key:
            tab = self.host_table(int(O), None if T is None else int(T))
            self._on = EnsSpecOn(self.alpha, None if tab is None else torch.from_numpy(tab).to(device), tab)
            self._key = key
        return self._on

    def __repr__(self):
        return (f"EnsembleLoss(alpha={self.alpha}, "
                f"output_weights={None if self.output_weights is None else self.output_weights.tolist()}, "
                f"step_weights={None if self.step_weights is None else self.step_weights.tolist()})")
