"""Inference helpers around the HIP forward path, mirroring the reference's analysis notebook:
test-set prediction with de-normalisation (test.ipynb cell 8, :257-300), the one-at-a-time
(OAT) input-perturbation sweep (test.ipynb cell 56, :2433-2461) and the evaluation cells -- R2 per
window and per grid cell, time-mean maps, cos-latitude weighted means (:377-385, :462-485, :605, :630,
:684-693, :796-803) -- from f64 sums kept on the device (`evaluate_skill`, `SkillAccumulator`,
`skill_from_sums`).  Forward only, `torch.no_grad()`."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields
from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._lib import NINT_ENS_MAX_M, NINT_ENS_PIX, NINT_ENS_SAMPLE, NINT_SKILL_PIX, NINT_SKILL_SAMPLE, NINT_SPEC_MAX_W, NINT_SPEC_PLANES


@torch.no_grad()
def predict(net, dataset, batch_size: int = 8, halo: Tuple[int, int] = (5, 5), indices: Sequence[int] = None):
    """Returns (GTs, PDs[, HSs]) in physical units: crop `[halo:halo+H]`, squeeze, `p * y_std + y_mean`
    (test.ipynb cell 8).  HSs (per-step head outputs) only when `net.return_sequence` is set."""
    net.eval()
    idx = list(range(len(dataset))) if indices is None else list(indices)
    H, W = dataset.grid
    gts, pds, hss = [], [], []
    for s in range(0, len(idx), batch_size):
        X, y = dataset.device_batch(idx[s:s + batch_size])
        out = net(X)
        pred, hs = (out if isinstance(out, tuple) else (out, None))
        p = pred[:, :, halo[0]:halo[0] + H, halo[1]:halo[1] + W]
        gts.append(y.cpu().numpy().reshape(p.shape) * dataset.y_std + dataset.y_mean)
        pds.append(p.cpu().numpy() * dataset.y_std + dataset.y_mean)
        if hs is not None:
            hss.append(hs[:, :, halo[0]:halo[0] + H, halo[1]:halo[1] + W].cpu().numpy() * dataset.y_std + dataset.y_mean)
    res = (np.concatenate(gts), np.concatenate(pds))
    return res + (np.concatenate(hss),) if hss else res


@torch.no_grad()
def oat_sensitivity(net, dataset, num_ftrs: int = 5, perturbed_values: float = 0.05, batch_size: int = 8,
                    halo: Tuple[int, int] = (5, 5), indices: Sequence[int] = None) -> np.ndarray:
    """One-at-a-time sweep (test.ipynb cell 56): for feature i, `X[:, :, i] *= 1 + perturbed_values` on the
    normalised, padded input, forward, crop, de-normalise.  Returns (num_ftrs, N, O, H, W)."""
    net.eval()
    idx = list(range(len(dataset))) if indices is None else list(indices)
    H, W = dataset.grid
    outs = []
    for i in range(num_ftrs):
        pds = []
        for s in range(0, len(idx), batch_size):
            X, _ = dataset.device_batch(idx[s:s + batch_size])
            X[:, :, i] *= (1 + perturbed_values)
            out = net(X)
            pred = out[0] if isinstance(out, tuple) else out
            p = pred[:, :, halo[0]:halo[0] + H, halo[1]:halo[1] + W]
            pds.append(p.cpu().numpy() * dataset.y_std + dataset.y_mean)
        outs.append(np.concatenate(pds))
    return np.stack(outs)


# ------------------------------------------------------------------------------ test-period skill from device-side sums
@dataclass
class SkillReport:
    """What the notebook's evaluation cells compute, in physical units.  Maps are (O, Hc, Wc) over the chosen slots' samples;
    per-sample series are in evaluation order."""
    r2_spatial: np.ndarray               # R2 per grid cell over time (test.ipynb:462-485)
    rmse: np.ndarray
    bias: np.ndarray                     # mean of p - y
    pearson: np.ndarray                  # nan where the target or the prediction is constant over time (as np.corrcoef)
    mean_gt: np.ndarray                  # time-mean maps (:605, :630)
    mean_pd: np.ndarray
    r2_temporal: np.ndarray              # (N): R2 per window, outputs pooled (:377-385, the notebook's flatten())
    r2_temporal_per_output: np.ndarray   # (N, O)
    loss: np.ndarray                     # (N): MSE + L1 in z-score units (train.py:102,105)
    global_mean_gt: np.ndarray           # (N, O): row-weighted (cos latitude) mean over the grid (:796-803)
    global_mean_pd: np.ndarray
    r2: float                            # pooled over every sample, output and grid cell
    count: float                         # samples behind the maps

    def arrays(self) -> dict:
        return {f.name: np.asarray(getattr(self, f.name)) for f in fields(self)}


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker's product with Veltkamp's split): the rounded product and its rounding error"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _centred(sqq, sq, n):
    """sum (q - mean q)^2 = sum q^2 - (sum q)^2 / n from f64 sums of n terms.  (sum q)^2 / n is formed in double-double
    arithmetic: where the target barely varies (a tracer that is zero in six of a group's seven windows) the difference is 1e-5 of
    sum q^2 and R2 is -1e4 ... -1e5, so the two roundings of the plain f64 expression alone would move R2 by 1e-7; the sums
    themselves are exact or nearly so there (few f32 values and their squares add without rounding in f64).
    A result below the rounding error that the n additions behind each sum may have left, (n + 4) eps sum q^2, is taken as exactly
    0: a constant q then counts as constant for any n; in exact arithmetic only values that agree to about 1e-7 relative fall
    under it."""
    sqq, sq = np.asarray(sqq, dtype=np.float64), np.asarray(sq, dtype=np.float64)
    n = float(n)
    p, e = _two_prod(sq, sq)
    hi = p / n
    ph, pe = _two_prod(hi, np.float64(n))
    lo = (((p - ph) - pe) + e) / n                      # (sum q)^2 / n = hi + lo to ~1e-32 relative
    tot = (sqq - hi) - lo
    return np.where(tot > (n + 4.0) * np.finfo(np.float64).eps * sqq, tot, 0.0)


def _r2(ss_res, ss_tot):
    """1 - ss_res / ss_tot with sklearn's constant-target convention: ss_tot == 0 gives 1.0 when ss_res == 0, else 0.0"""
    ss_res, ss_tot = np.asarray(ss_res, dtype=np.float64), np.asarray(ss_tot, dtype=np.float64)
    ok = ss_tot > 0
    return np.where(ok, 1.0 - ss_res / np.where(ok, ss_tot, 1.0), np.where(ss_res == 0, 1.0, 0.0))


def skill_from_sums(pix, counts, sample, row_w=None, y_mean: float = 0.0, y_std: float = 1.0,
                    slots: Optional[Sequence[int]] = None) -> SkillReport:
    """The f64 sums of nint_skill_accum / nint_head_skill_accum (z-score units) -> a SkillReport in physical units
    (value * y_std + y_mean).  Pure numpy f64; needs no GPU.

    pix (nslots, 5, O, Hc, Wc): per slot and grid cell sum y, sum p, sum y^2, sum p^2, sum (y-p)^2; counts (nslots): samples
    per slot; sample (N, O, 8): per sample and output sum (y-p)^2, sum |y-p|, sum y, sum y^2, sum p, sum p^2, sum row_w*y,
    sum row_w*p over the grid; row_w (Hc) the row weights the last two were formed with (None: 1).  `slots`: the union of
    slots behind the maps (None: all) -- the slots partition the samples, so a union is the sum of its slots' planes.

    The statistics are formed in z-score units and de-normalised analytically: R2 and r do not change under the affine map,
    means shift and scale, rmse and bias scale -- which keeps sum y^2 - (sum y)^2 / n free of the cancellation that physical
    units (mean >> spread) would bring.

    R2 follows sklearn's constant-target convention everywhere (as loss_final_kernel does): ss_tot == 0 gives 1.0 when
    ss_res == 0, else 0.0; an ss_tot below the rounding error of its own computation counts as 0 (_centred).  The notebook's vectorised r_squared_spatial (test.ipynb:480-485) yields nan / -inf there; its
    r2_score loop (:462-470) yields these values."""
    pix = np.asarray(pix, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    sample = np.asarray(sample, dtype=np.float64)
    nslots, npl, O, Hc, Wc = pix.shape
    assert npl == NINT_SKILL_PIX and counts.shape == (nslots,) and sample.shape[1:] == (O, NINT_SKILL_SAMPLE)
    sel = list(range(nslots)) if slots is None else [int(v) for v in slots]
    sy, sp, syy, spp, sdd = pix[sel].sum(axis=0)
    n = float(counts[sel].sum())
    sig, mu = float(y_std), float(y_mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / n if n > 0 else np.nan
        tot_y, tot_p = (_centred(syy, sy, n), _centred(spp, sp, n)) if n > 0 else (syy * np.nan, spp * np.nan)
        cov = 0.5 * (syy + spp - sdd) - sy * sp * inv                     # sum y p from (y-p)^2 = y^2 + p^2 - 2 y p
        pearson = np.where((tot_y > 0) & (tot_p > 0), cov / np.sqrt(np.where(tot_y > 0, tot_y, 1.0) * np.where(tot_p > 0, tot_p, 1.0)), np.nan)
        rep = dict(r2_spatial=_r2(sdd, tot_y), rmse=sig * np.sqrt(sdd * inv), bias=sig * (sp - sy) * inv, pearson=pearson,
                   mean_gt=mu + sig * sy * inv, mean_pd=mu + sig * sp * inv)
    # per sample, over the grid
    npx = float(Hc * Wc)
    d2, d1, ty, tyy = sample[..., 0], sample[..., 1], sample[..., 2], sample[..., 3]
    rep["r2_temporal_per_output"] = _r2(d2, _centred(tyy, ty, npx))
    rep["r2_temporal"] = _r2(d2.sum(axis=1), _centred(tyy.sum(axis=1), ty.sum(axis=1), O * npx))
    rep["loss"] = d2.sum(axis=1) / (O * npx) + d1.sum(axis=1) / (O * npx)
    wsum = Wc * (float(Hc) if row_w is None else float(np.asarray(row_w, dtype=np.float64).sum()))
    rep["global_mean_gt"] = mu + sig * sample[..., 6] / wsum
    rep["global_mean_pd"] = mu + sig * sample[..., 7] / wsum
    nall = sample.shape[0] * O * npx
    rep["r2"] = float(_r2(d2.sum(), _centred(tyy.sum(), ty.sum(), nall))) if nall else float("nan")
    return SkillReport(count=n, **rep)


class SkillAccumulator:
    """Device-side accumulators of one evaluation: `pix` (nslots, 5, O, Hc, Wc) f64, the per-sample sums of every batch seen
    (a growing (n_samples, O, 8) table) and the kernels' scratch.  `lat`: Hc latitudes in degrees, row_w = cos(deg2rad(lat))
    (test.ipynb:796); None = uniform weights.  `halo`: (oy, ox) of the crop inside the model grid; None = centred.
    The slots of a sample are host knowledge, so the per-slot sample counts are counted on the host; `counts` hands them out
    as an f64 device tensor (what a data-parallel reduction would add up with `pix`)."""

    def __init__(self, O: int, Hc: int, Wc: int, nslots: int = 1, lat=None, device="cuda", halo: Optional[Tuple[int, int]] = None):
        from . import _lib
        self.lib = _lib.load()
        self.O, self.Hc, self.Wc, self.nslots = int(O), int(Hc), int(Wc), int(nslots)
        if self.nslots < 1:
            raise ValueError("nslots must be >= 1")
        self.device = torch.device(device)
        self.halo = None if halo is None else (int(halo[0]), int(halo[1]))
        self.row_w_host = None
        self.row_w = None
        if lat is not None:
            lat = np.asarray(lat, dtype=np.float64)
            if lat.shape != (self.Hc,):
                raise ValueError(f"lat: expected {self.Hc} latitudes, got {lat.shape}")
            self.row_w_host = np.cos(np.deg2rad(lat))
            self.row_w = torch.from_numpy(self.row_w_host).to(self.device)   # f64 on the device too
        self.pix = torch.zeros(self.nslots, NINT_SKILL_PIX, self.O, self.Hc, self.Wc, dtype=torch.float64, device=self.device)
        self._counts = np.zeros(self.nslots, dtype=np.float64)
        self._rows = []
        self._scratch = None

    @property
    def counts(self) -> torch.Tensor:
        return torch.from_numpy(self._counts.copy()).to(self.device)

    @property
    def n_samples(self) -> int:
        return sum(int(r.shape[0]) for r in self._rows)

    def scratch_for(self, N: int) -> torch.Tensor:
        need = self.lib.nint_skill_scratch_bytes(int(N), self.O, self.Hc, self.Wc) // 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        return self._scratch

    def _slots(self, slots, N: int):
        sl = [0] * N if slots is None else [int(v) for v in slots]
        if len(sl) != N or any(v < -1 or v >= self.nslots for v in sl):
            raise ValueError(f"slots: {N} values in [-1, {self.nslots}) expected")
        return sl

    def _count(self, sl):
        for v in sl:
            if v >= 0:
                self._counts[v] += 1.0

    def update(self, eng, ws, w, b, y, slots=None, pred_out=None):
        """One batch through the fused pass (SeqEngine.head_skill) after eng.forward(ws, X)."""
        sl = self._slots(slots, ws.B)
        self._rows.append(eng.head_skill(ws, w, b, y, sl, self, pred_out=pred_out))
        self._count(sl)

    def update_from_pred(self, pred: torch.Tensor, y: torch.Tensor, halo: Tuple[int, int], slots=None):
        """One batch from a prediction (N, O, H, W) that is already in memory (nint_skill_accum)."""
        from ._lib import check, ptr, stream_ptr
        pv = pred.detach().float().contiguous()
        N, O, H, W = pv.shape
        yv = y.detach().float().contiguous()
        assert O == self.O and yv.numel() == N * O * self.Hc * self.Wc, "target must be (N,[O,]Hc,Wc)"
        sl = self._slots(slots, N)
        sample = torch.empty(N, O, NINT_SKILL_SAMPLE, dtype=torch.float64, device=self.device)
        scratch = self.scratch_for(N)
        check(self.lib.nint_skill_accum(ptr(pv), ptr(yv), (C.c_int32 * N)(*sl), self.nslots, ptr(self.row_w), ptr(self.pix),
                                        ptr(sample), ptr(scratch), scratch.numel() * 8, N, O, H, W, int(halo[0]), int(halo[1]),
                                        self.Hc, self.Wc, stream_ptr()), "nint_skill_accum")
        self._rows.append(sample)
        self._count(sl)

    def sums(self):
        """(pix, counts, sample) as numpy f64: ONE device-to-host read"""
        rows = torch.cat(self._rows) if self._rows else torch.empty(0, self.O, NINT_SKILL_SAMPLE, dtype=torch.float64, device=self.device)
        flat = torch.cat([self.pix.reshape(-1), rows.reshape(-1)]).cpu().numpy()
        return (flat[:self.pix.numel()].reshape(tuple(self.pix.shape)), self._counts.copy(),
                flat[self.pix.numel():].reshape(-1, self.O, NINT_SKILL_SAMPLE))

    def report(self, y_mean: float = 0.0, y_std: float = 1.0, slots: Optional[Sequence[int]] = None) -> SkillReport:
        pix, counts, sample = self.sums()
        return skill_from_sums(pix, counts, sample, self.row_w_host, y_mean, y_std, slots)


@torch.no_grad()
def evaluate_skill(net, dataset, batch_size: int = 8, halo: Tuple[int, int] = (5, 5), indices: Sequence[int] = None,
                   groups: Union[None, Sequence[int], Callable[[int], int]] = None, lat=None, return_predictions: bool = False):
    """Test-period skill without gathering the predictions: per batch forward + ONE pass that applies the head to the last
    hidden state and folds the result into f64 sums on the device (no host synchronisation in the loop, one read at the end).
    Returns the SkillAccumulator -- `.report(dataset.y_mean, dataset.y_std[, slots])` gives the notebook's quantities for all
    samples or a union of groups -- and, with `return_predictions`, the z-score-unit crop (N, O, Hc, Wc) as a device tensor.

    `groups`: the slot of each dataset index (an int array indexed by dataset index, or a callable), e.g. the month of the
    window's target step; -1 keeps a sample out of the maps.  None: one slot.
    The last step's prediction only: the sums are additive, so per-step (`return_sequence`) skill and a data-parallel
    reduction can be added on top."""
    net.eval()
    dev = next(net.parameters()).device
    eng = net._engine(dev)
    idx = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    slot_of = (lambda i: 0) if groups is None else (groups if callable(groups) else (lambda i: int(groups[i])))
    slots_all = [int(slot_of(i)) for i in idx]
    nslots = max([v for v in slots_all if v >= 0], default=0) + 1
    Hc, Wc = dataset.grid
    O = net.conv.weight.shape[0]
    acc = SkillAccumulator(O, Hc, Wc, nslots=nslots, lat=lat, device=dev, halo=halo)
    preds = torch.empty(len(idx), O, Hc, Wc, dtype=torch.float32, device=dev) if return_predictions else None
    for s in range(0, len(idx), batch_size):
        X, y = dataset.slab_batch(idx[s:s + batch_size])
        B, T, _, H, W = X.shape
        with eng.window(B, T, H, W, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, X, residual=_residual(net))
            acc.update(eng, ws, net.conv.weight, net.conv.bias, y, slots_all[s:s + B], pred_out=None if preds is None else preds[s:s + B])
    return (acc, preds) if return_predictions else acc


# ------------------------------------------------------------------------------ roll-forward inference with carried state
@torch.no_grad()
def predict_stream(net, dataset, lanes: int = 1, halo: Tuple[int, int] = (5, 5), skill: Optional[SkillAccumulator] = None,
                   closed_loop: bool = False, spinup: int = 1):
    """Walk the dataset's period ONCE: non-overlapping chunks of `dataset.seq_len` steps with the state carried on the device
    (`net(X, state, return_state="device")`), the head applied at every step (head_forward_seq) -- where `predict` runs
    every record step seq_len times, once per sliding window it falls into.

    Returns (pred, steps, dropped): `pred` (N, O, Hc, Wc) f32 on the device, the cropped per-step predictions in z-score
    units in time order; `steps` (N,) int64 numpy, the record step each belongs to; `dropped`, the number of steps at the
    end of the period that fill no chunk (reported, not predicted).

    `lanes` > 1 cuts the period into that many contiguous segments that run as one batch.  EACH SEGMENT STARTS FROM THE ZERO
    STATE, so the first steps of every segment but the first see less history than with lanes = 1; the steps of the chunks
    that fill no full row of lanes are dropped too.

    `skill`: a SkillAccumulator (O, Hc, Wc of the dataset's grid) that every chunk's steps are folded into
    (update_from_pred, time steps as samples, slot 0) against the tracer at the same steps.

    `closed_loop` (a ``ConvLSTM(feedback=True)``): the model runs on its own prediction.  The first chunk
    takes its first `spinup` >= 1 steps from the dataset (the spin-up on analysis data) and feeds the head's output back
    from step `spinup` on; every later chunk is fed from its step 0, from the head of the carried state -- so the walk
    equals ONE closed-loop window over the whole period, bit for bit.  (A residual head, DESIGN.md 4.22: a later chunk's
    step 0 receives the previous chunk's last prediction through the pack instead, and is fed from its step 1 -- the same
    bits: the pack rounds as the feedback launch does.)  With `lanes` > 1 every lane spins up on its own
    first chunk (the lanes' first chunks are one batch)."""
    from .dataset import stateful_schedule
    if closed_loop:
        if not getattr(net, "feedback", False):
            raise ValueError("predict_stream(closed_loop=True) needs a ConvLSTM built with feedback=True")
        if isinstance(spinup, bool) or int(spinup) != spinup or spinup < 1:
            raise ValueError(f"predict_stream: spinup must be an integer >= 1 (step 0 has no prediction to be fed), got {spinup!r}")
    net.eval()
    T = dataset.seq_len
    Hc, Wc = dataset.grid
    sched, _ = stateful_schedule(len(dataset), T, lanes)
    K, B = sched.shape
    n_steps = len(dataset) + T - 1                        # record steps the period's windows cover
    dropped = n_steps - K * B * T
    O = net.conv.weight.shape[0]
    dev = next(net.parameters()).device
    eng = net._engine(dev)
    out = torch.empty(B, K * T, O, Hc, Wc, dtype=torch.float32, device=dev)
    dv = dataset._device_arrays() if skill is not None else None
    state, last, res = None, None, _residual(net)
    for k in range(K):
        X, _ = dataset.slab_batch(sched[k])
        _, _, _, H, W = X.shape
        with eng.window(B, T, H, W, False, state is not None) as ws:
            net._pack_weights(eng)
            if state is not None:
                eng.load_state(ws, state)
            fb = (net.conv.weight, net.conv.bias, int(spinup) if k == 0 else 0) if closed_loop else None
            if fb is not None and k > 0 and res:
                # residual head: a chunk cannot be fed at its step 0 (the base of that value lies in the chunk before), so the
                # previous chunk's last prediction is packed into the feedback channels of step 0 -- the pack rounds exactly
                # as the feedback kernel does -- and the chunk is fed from step 1.  The chunk travels as an f32 tensor for that
                # (device_batch: the same values the slab fill writes, through the pack kernel).
                X, _ = dataset.device_batch(sched[k])
                X[:, 0, X.shape[2] - O:] = last
                fb = (net.conv.weight, net.conv.bias, 1)
            eng.forward(ws, X, feedback=fb, residual=res)
            state = eng.save_state(ws, state)
            seq = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias)             # (B, T*O, H, W), channel t*O + o
            last = seq[:, (T - 1) * O:]                 # p_{T-1} on the whole grid: what the next chunk's step 0 is fed
        out[:, k * T:(k + 1) * T] = seq.view(B, T, O, H, W)[:, :, :, halo[0]:halo[0] + Hc, halo[1]:halo[1] + Wc]
        if skill is not None:
            t0s = [int(dataset.first[int(i)]) for i in sched[k]]
            y = _step_targets(dataset, dv, t0s, T)                                # (B, T, L, Hc, Wc)
            skill.update_from_pred(seq.view(B * T, O, H, W), y.reshape(B * T, O, Hc, Wc), halo)
    first = int(dataset.first[0])
    steps = np.concatenate([first + int(sched[0, b]) + np.arange(K * T, dtype=np.int64) for b in range(B)])
    return out.view(B * K * T, O, Hc, Wc), steps, dropped


def _residual(net):
    """SeqEngine.forward's ``residual`` argument for a model: its number of head outputs if it has a residual head, else False"""
    return net.conv.weight.shape[0] if getattr(net, "residual", False) else False


def _step_targets(dataset, dv, t0s, T):
    """z-scored tracer at every step of the windows starting at record steps t0s: (B, T, L, H, W) on the device"""
    from . import _lib
    from ._lib import check, ptr, stream_ptr
    H, W = dataset.grid
    B, L = len(t0s), dataset.levels
    y = torch.empty(B, T, L, H, W, dtype=torch.float32, device=dataset.device)
    yptr = (C.c_void_p * 1)(dv["y"].data_ptr())
    ylev = (C.c_int * 1)(L)
    tl = (C.c_int * B)(*t0s)
    check(_lib.load().nint_preproc_fuse_pad_batch(yptr, ylev, 1, ptr(dv["ymean"]), ptr(dv["ystd"]), tl, B, ptr(y), T, H, W, H, W, 1,
                                                  stream_ptr()), "target z-score")
    return y


# ------------------------------------------------------------------------------ closed-loop roll-out skill by lead time
@torch.no_grad()
def rollout_skill(net, dataset, starts: Sequence[int], horizon: int, spinup: int, batch_size: int = 8, lat=None,
                  halo: Optional[Tuple[int, int]] = None, spectrum: Optional["SpectrumAccumulator"] = None) -> SkillAccumulator:
    """Skill of the free-running model by LEAD TIME.  From every record step in `starts` a window of
    `spinup + horizon` steps runs closed loop from step `spinup` (``ConvLSTM(feedback=True)``; the first `spinup` steps see
    the dataset's input, the rest the model's own prediction in the feedback channels).  The prediction made `j` steps into
    the free run -- the head's output at window step spinup + j, against the tracer of that record step -- is folded into
    slot j of the returned SkillAccumulator (update_from_pred, targets from the record), so
    ``acc.report(dataset.y_mean, dataset.y_std, slots=[j])`` is the skill at lead time j, 0 <= j < horizon.

    `starts`: record steps (not dataset indices), each with start + spinup + horizon <= the record's length, and >= 1 for a
    ``tracer_input`` dataset.  `halo`: the crop's offset inside the model grid (None: centred).
    `spectrum`: a SpectrumAccumulator(O, Hc, Wc, M=1, nslots=horizon, halo=halo) that is filled from the same per-step head
    output, slot j = lead time j; a mismatch is a ValueError before any device work.  None: nothing changes."""
    from .dataset import SlabBatch
    if not getattr(net, "feedback", False):
        raise ValueError("rollout_skill needs a ConvLSTM built with feedback=True")
    horizon, spinup = int(horizon), int(spinup)
    if horizon < 1 or spinup < 1:
        raise ValueError(f"rollout_skill: horizon and spinup must be >= 1, got {(horizon, spinup)}")
    T = spinup + horizon
    starts = [int(v) for v in starts]
    n_steps = int(dataset.yraw.shape[0])
    lo = 1 if getattr(dataset, "tracer_input", False) else 0
    if not starts or min(starts) < lo or max(starts) + T > n_steps:
        raise ValueError(f"rollout_skill: every start must lie in [{lo}, {n_steps - T}] for windows of {T} steps in a record of {n_steps}")
    if spectrum is not None:
        spectrum._check_rollout("rollout_skill", net.conv.weight.shape[0], dataset.grid[0], dataset.grid[1], 1, horizon, halo)
    net.eval()
    dev = next(net.parameters()).device
    eng = net._engine(dev)
    Hc, Wc = dataset.grid
    O = net.conv.weight.shape[0]
    if O != dataset.levels:
        raise ValueError(f"rollout_skill: the head has {O} outputs, the record's tracer {dataset.levels} levels")
    acc = SkillAccumulator(O, Hc, Wc, nslots=horizon, lat=lat, device=dev, halo=halo)
    dv = dataset._device_arrays()
    for s in range(0, len(starts), batch_size):
        t0s = starts[s:s + batch_size]
        X = SlabBatch(dataset, np.asarray(t0s), T)
        B, _, _, H, W = X.shape
        oy, ox = ((H - Hc) // 2, (W - Wc) // 2) if halo is None else halo
        with eng.window(B, T, H, W, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, spinup), residual=_residual(net))
            seq = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(B, T, O, H, W)
        y = _step_targets(dataset, dv, t0s, T)                                    # (B, T, L, Hc, Wc)
        free = seq[:, spinup:].reshape(B * horizon, O, H, W)
        slots = [j for _ in range(B) for j in range(horizon)]
        acc.update_from_pred(free, y[:, spinup:].reshape(B * horizon, O, Hc, Wc), (oy, ox), slots)
        if spectrum is not None:
            spectrum.update_from_pred(free, y[:, spinup:].reshape(B * horizon, O, Hc, Wc), (oy, ox), slots)
    return acc


def lead_time_r2(acc: SkillAccumulator) -> np.ndarray:
    """R2 per slot of an accumulator, every output and grid cell of the slot's samples pooled (rollout_skill: per lead time):
    1 - sum (y-p)^2 / (sum y^2 - (sum y)^2 / n) from the slot's f64 planes; nan for an empty slot"""
    pix, counts, _ = acc.sums()
    out = np.full(acc.nslots, np.nan)
    for j in range(acc.nslots):
        n = counts[j] * acc.O * acc.Hc * acc.Wc
        if n > 0:
            out[j] = float(_r2(pix[j, 4].sum(), _centred(pix[j, 2].sum(), pix[j, 0].sum(), n)))
    return out


# ------------------------------------------------------------------------------ ensemble statistics from device-side sums
@dataclass
class EnsembleReport:
    """Ensemble verification from the sums of nint_ens_accum, in z-score units; the `_phys` fields are the
    same figures times `scale` (y_std), where a scale applies -- ratios, R2 and the histogram have none.  Scalars pool every
    sample, output and grid cell of the chosen slots; maps are (O, Hc, Wc); the cos-latitude means are one row per sample
    of those slots, (n, O), in the order the samples were folded in."""
    rmse_mean: float                     # sqrt(mean (ensemble mean - y)^2)
    spread: float                        # sqrt(mean unbiased member variance)
    spread_skill: float                  # sqrt((M+1)/M) * spread / rmse_mean: 1 for a reliable ensemble
    crps_fair: float                     # mean over cells of A / M - D / (M (M - 1)): the fair CRPS (unbiased in the ensemble size)
    crps: float                          # the plain form: A/M - D/M^2
    bias: float                          # mean (ensemble mean - y)
    r2_mean: float                       # R2 of the ensemble mean
    rmse_mean_map: np.ndarray
    spread_map: np.ndarray
    spread_skill_map: np.ndarray
    crps_fair_map: np.ndarray
    coslat_mse_mean: np.ndarray          # row-weighted (cos latitude) means over the grid, per sample and output
    coslat_variance: np.ndarray
    coslat_crps_fair: np.ndarray
    coslat_crps: np.ndarray
    rank_hist: np.ndarray                # (O, M + 2) int64: bins 0..M the target's rank, bin M + 1 the NaN cells
    rmse_mean_phys: float
    spread_phys: float
    crps_fair_phys: float
    crps_phys: float
    bias_phys: float
    members: int
    count: float                         # samples behind the maps
    scale: float

    def arrays(self) -> dict:
        return {f.name: np.asarray(getattr(self, f.name)) for f in fields(self)}


def ensemble_from_sums(pix, counts, sample, rank_hist, M: int, row_w=None, y_mean: float = 0.0, y_std: float = 1.0,
                       slots: Optional[Sequence[int]] = None, sample_slots: Optional[Sequence[int]] = None) -> EnsembleReport:
    """The sums of nint_ens_accum -> an EnsembleReport.  Pure numpy f64; needs no GPU.

    pix (nslots, 7, O, Hc, Wc): per slot and cell sum E^2, sum V, sum A, sum D, sum E, sum t, sum t^2, where per sample
    S = sum_i x_i, E = S - M t, V = sum_i (M x_i - S)^2, A = sum_i |x_i - t|, D = sum_{i<j} |x_i - x_j|; counts (nslots):
    samples per slot; sample (N, O, 8): sum E^2, V, A, D over the grid, then the same weighted by row_w (Hc; None: 1);
    rank_hist (nslots, O, M + 2).  Every division the kernel left out happens here, over n values:
      MSE of the ensemble mean = sum E^2 / M^2 / n          mean variance = sum V / (M^2 (M - 1)) / n   (1/(M-1) sum (x_i - mean)^2)
      fair CRPS = (sum A / M - sum D / (M (M - 1))) / n     plain CRPS    = (sum A / M - sum D / M^2) / n
      bias = sum E / M / n                                  R2 = 1 - (sum E^2 / M^2) / (sum t^2 - (sum t)^2 / n)
    `slots`: the union of slots behind the maps and scalars (None: all); `sample_slots` (N): the slot of each sample row,
    which restricts the cos-latitude rows to that union (None: every row).  y_mean shifts no figure reported here."""
    pix, counts, sample = np.asarray(pix, np.float64), np.asarray(counts, np.float64), np.asarray(sample, np.float64)
    rank_hist = np.asarray(rank_hist, np.int64)
    M = int(M)
    nslots, npl, O, Hc, Wc = pix.shape
    if not 2 <= M <= NINT_ENS_MAX_M:
        raise ValueError(f"ensemble_from_sums: members must lie in [2, {NINT_ENS_MAX_M}], got {M}")
    assert npl == NINT_ENS_PIX and counts.shape == (nslots,) and sample.shape[1:] == (O, NINT_ENS_SAMPLE)
    assert rank_hist.shape == (nslots, O, M + 2)
    sel = list(range(nslots)) if slots is None else [int(v) for v in slots]
    see, sv, sa, sd, se, st, stt = pix[sel].sum(axis=0)
    n = float(counts[sel].sum())
    m2, m2m1, mm1 = float(M * M), float(M * M * (M - 1)), float(M * (M - 1))
    kappa = np.sqrt((M + 1.0) / M)
    sig = float(y_std)

    def figures(see, sv, sa, sd, cnt):
        """(rmse, spread, ratio, fair CRPS, plain CRPS) of sums over cnt values; arrays or scalars"""
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / cnt if cnt > 0 else np.nan
            rmse, spread = np.sqrt(see / m2 * inv), np.sqrt(sv / m2m1 * inv)
            return rmse, spread, kappa * spread / rmse, (sa / M - sd / mm1) * inv, (sa / M - sd / m2) * inv

    rmse_map, spread_map, ratio_map, fair_map, _ = figures(see, sv, sa, sd, n)
    ncell = n * O * Hc * Wc
    rmse, spread, ratio, fair, plain = (float(v) for v in figures(see.sum(), sv.sum(), sa.sum(), sd.sum(), ncell))
    bias = float(se.sum() / M / ncell) if ncell > 0 else float("nan")
    r2 = float(_r2(see.sum() / m2, _centred(stt.sum(), st.sum(), ncell))) if ncell > 0 else float("nan")
    rows = sample if sample_slots is None else sample[[i for i, s in enumerate(sample_slots) if int(s) in sel]]
    wsum = Wc * (float(Hc) if row_w is None else float(np.asarray(row_w, dtype=np.float64).sum()))
    return EnsembleReport(
        rmse_mean=rmse, spread=spread, spread_skill=ratio, crps_fair=fair, crps=plain, bias=bias, r2_mean=r2,
        rmse_mean_map=rmse_map, spread_map=spread_map, spread_skill_map=ratio_map, crps_fair_map=fair_map,
        coslat_mse_mean=rows[..., 4] / m2 / wsum, coslat_variance=rows[..., 5] / m2m1 / wsum,
        coslat_crps_fair=(rows[..., 6] / M - rows[..., 7] / mm1) / wsum, coslat_crps=(rows[..., 6] / M - rows[..., 7] / m2) / wsum,
        rank_hist=rank_hist[sel].sum(axis=0), rmse_mean_phys=sig * rmse, spread_phys=sig * spread, crps_fair_phys=sig * fair,
        crps_phys=sig * plain, bias_phys=sig * bias, members=M, count=n, scale=sig)


class EnsembleAccumulator:
    """Device-side accumulators of one ensemble evaluation (nint_ens_accum): `pix` (nslots, 7, O, Hc, Wc) f64, `rank_hist`
    (nslots, O, M + 2) int64, the per-sample sums of every batch seen (a growing (n_samples, O, 8) table) and the kernel's
    scratch.  `lat`, `halo`: as SkillAccumulator's.  The sums are additive: a data-parallel reduction adds the ranks' `pix`,
    `rank_hist` and `counts`."""

    def __init__(self, O: int, Hc: int, Wc: int, M: int, nslots: int = 1, lat=None, device="cuda", halo: Optional[Tuple[int, int]] = None):
        from . import _lib
        self.O, self.Hc, self.Wc, self.M, self.nslots = int(O), int(Hc), int(Wc), int(M), int(nslots)
        if self.nslots < 1:
            raise ValueError("nslots must be >= 1")
        if not 2 <= self.M <= NINT_ENS_MAX_M:
            raise ValueError(f"EnsembleAccumulator: members must lie in [2, {NINT_ENS_MAX_M}], got {self.M}")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.halo = None if halo is None else (int(halo[0]), int(halo[1]))
        self.row_w_host = None
        self.row_w = None
        if lat is not None:
            lat = np.asarray(lat, dtype=np.float64)
            if lat.shape != (self.Hc,):
                raise ValueError(f"lat: expected {self.Hc} latitudes, got {lat.shape}")
            self.row_w_host = np.cos(np.deg2rad(lat))
            self.row_w = torch.from_numpy(self.row_w_host).to(self.device)
        self.pix = torch.zeros(self.nslots, NINT_ENS_PIX, self.O, self.Hc, self.Wc, dtype=torch.float64, device=self.device)
        self.rank_hist = torch.zeros(self.nslots, self.O, self.M + 2, dtype=torch.int64, device=self.device)
        self._counts = np.zeros(self.nslots, dtype=np.float64)
        self._rows, self._row_slots = [], []
        self._scratch = None

    @property
    def counts(self) -> torch.Tensor:
        return torch.from_numpy(self._counts.copy()).to(self.device)

    @property
    def n_samples(self) -> int:
        return len(self._row_slots)

    def scratch_for(self, N: int) -> torch.Tensor:
        need = self.lib.nint_ens_scratch_bytes(int(N), self.M, self.O, self.Hc, self.Wc) // 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        return self._scratch

    def update(self, pred: torch.Tensor, sample_off: Sequence[int], member_stride: int, y: torch.Tensor, slots=None,
               mean_out: Optional[torch.Tensor] = None):
        """Fold one batch in.  `pred`: a contiguous f32 device tensor whose last three dimensions are (O, H, W); member i of
        sample n is the image at element sample_off[n] + i * member_stride of it, read in place.  `y` (N, O, Hc, Wc) f32."""
        from ._lib import check, ptr, stream_ptr
        if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() < 3 or pred.shape[-3] != self.O:
            raise ValueError(f"EnsembleAccumulator.update: pred must be a contiguous f32 tensor (..., {self.O}, H, W)")
        H, W = int(pred.shape[-2]), int(pred.shape[-1])
        off = [int(v) for v in sample_off]
        N, stride = len(off), int(member_stride)
        if N < 1 or stride < 0 or min(off) < 0 or max(off) + (self.M - 1) * stride + self.O * H * W > pred.numel():
            raise ValueError("EnsembleAccumulator.update: a member image lies outside pred")
        oy, ox = ((H - self.Hc) // 2, (W - self.Wc) // 2) if self.halo is None else self.halo
        yv = y.detach().float().contiguous()
        if yv.numel() != N * self.O * self.Hc * self.Wc:
            raise ValueError("EnsembleAccumulator.update: target must be (N, O, Hc, Wc)")
        sl = [0] * N if slots is None else [int(v) for v in slots]
        if len(sl) != N or any(v < -1 or v >= self.nslots for v in sl):
            raise ValueError(f"slots: {N} values in [-1, {self.nslots}) expected")
        if mean_out is not None and (mean_out.dtype != torch.float32 or not mean_out.is_contiguous()
                                     or mean_out.numel() != yv.numel()):
            raise ValueError("EnsembleAccumulator.update: mean_out must be a contiguous f32 (N, O, Hc, Wc)")
        sample = torch.empty(N, self.O, NINT_ENS_SAMPLE, dtype=torch.float64, device=self.device)
        scratch = self.scratch_for(N)
        check(self.lib.nint_ens_accum(ptr(pred), (C.c_int64 * N)(*off), stride, self.M, ptr(yv), (C.c_int32 * N)(*sl), self.nslots,
                                      ptr(self.row_w), ptr(self.pix), ptr(sample), ptr(self.rank_hist), ptr(mean_out), ptr(scratch),
                                      scratch.numel() * 8, N, self.O, H, W, int(oy), int(ox), self.Hc, self.Wc, stream_ptr()),
              "nint_ens_accum")
        self._rows.append(sample)
        self._row_slots += sl
        for v in sl:
            if v >= 0:
                self._counts[v] += 1.0

    def sums(self):
        """(pix, counts, sample, rank_hist) as numpy: ONE device-to-host read (the int64 counts travel as their bits)"""
        rows = torch.cat(self._rows) if self._rows else torch.empty(0, self.O, NINT_ENS_SAMPLE, dtype=torch.float64, device=self.device)
        flat = torch.cat([self.pix.reshape(-1), rows.reshape(-1), self.rank_hist.reshape(-1).view(torch.float64)]).cpu().numpy()
        a, b = self.pix.numel(), self.pix.numel() + rows.numel()
        return (flat[:a].reshape(tuple(self.pix.shape)), self._counts.copy(), flat[a:b].reshape(-1, self.O, NINT_ENS_SAMPLE),
                flat[b:].view(np.int64).reshape(tuple(self.rank_hist.shape)).copy())

    def report(self, y_mean: float = 0.0, y_std: float = 1.0, slots: Optional[Sequence[int]] = None) -> EnsembleReport:
        pix, counts, sample, hist = self.sums()
        return ensemble_from_sums(pix, counts, sample, hist, self.M, self.row_w_host, y_mean, y_std, slots, self._row_slots)


LEAD_TIME_COLUMNS = ("rmse_mean", "spread", "spread_skill", "crps_fair", "crps", "bias", "r2_mean")


def lead_time_table(acc: EnsembleAccumulator) -> np.ndarray:
    """The scalars of EnsembleReport per slot of an accumulator (rollout_ensemble: per lead time), z-score units:
    (nslots, 7) in the order of LEAD_TIME_COLUMNS; nan for an empty slot.  One device-to-host read."""
    pix, counts, sample, hist = acc.sums()
    out = np.full((acc.nslots, len(LEAD_TIME_COLUMNS)), np.nan)
    for j in range(acc.nslots):
        if counts[j] > 0:
            rep = ensemble_from_sums(pix, counts, sample, hist, acc.M, acc.row_w_host, slots=[j], sample_slots=acc._row_slots)
            out[j] = [getattr(rep, k) for k in LEAD_TIME_COLUMNS]
    return out


# ------------------------------------------------------------------------------ zonal power spectra from device-side sums
@dataclass
class SpectrumReport:
    """Zonal (along-longitude) power spectra from the sums of nint_spec_accum, z-score units, per output and
    wavenumber: (O, K) arrays, K = Wc // 2 + 1.  The densities are one-sided (the factor 2 for 0 < k < Wc / 2) and normalised
    by Wc^2, the sum of the row weights and the sample count, so a density summed over k is the weighted mean square of the
    field (Parseval).  nan where nothing was folded in."""
    wavenumber: np.ndarray               # (K,) 0 .. Wc // 2
    power_target: np.ndarray             # of the target
    power_member: np.ndarray             # mean over the members of each member's power
    power_mean: np.ndarray               # of the ensemble mean (the prediction for M = 1)
    power_error: np.ndarray              # of (ensemble mean - target)
    ratio_member: np.ndarray             # power_member / power_target: 1 where the members are as sharp as the analysis
    ratio_mean: np.ndarray               # power_mean / power_target: below ratio_member where the members disagree
    coherence: np.ndarray                # |sum S conj Y|^2 / (sum |S|^2 sum |Y|^2), in [0, 1]
    members: int
    width: int
    count: float                         # samples behind the figures

    def arrays(self) -> dict:
        return {f.name: np.asarray(getattr(self, f.name)) for f in fields(self)}


def _one_sided(Wc: int) -> np.ndarray:
    """the weight of each of the K = Wc // 2 + 1 lines in a one-sided spectrum: 1 for k = 0 and the Nyquist line, else 2"""
    c = np.full(Wc // 2 + 1, 2.0)
    c[0] = 1.0
    if Wc % 2 == 0:
        c[-1] = 1.0
    return c


def spectrum_from_sums(spec, counts, M: int, Wc: int, row_w_sum: float, slots: Optional[Sequence[int]] = None) -> SpectrumReport:
    """The sums of nint_spec_accum -> a SpectrumReport.  Pure numpy f64; needs no GPU.

    spec (nslots, 5, O, K): per slot, output and wavenumber the sums over samples and rows of w |Y|^2 (YY), w sum_i |P_i|^2
    (PP), w Re(S conj Y) (CR), w Im(S conj Y) (CI), w |S|^2 (SS) with S = sum_i P_i; counts (nslots): samples per slot;
    row_w_sum: the sum of the row weights (Hc without a table).  With c_k the one-sided factor and
    Z = Wc^2 * row_w_sum * n:  power_target = c YY / Z, power_member = c PP / M / Z, power_mean = c SS / M^2 / Z,
    power_error = c (SS / M^2 + YY - 2 CR / M) / Z, coherence = (CR^2 + CI^2) / (SS YY).  `slots`: the union of slots (None: all)."""
    spec, counts = np.asarray(spec, np.float64), np.asarray(counts, np.float64)
    M, Wc = int(M), int(Wc)
    if not 1 <= M <= NINT_ENS_MAX_M:
        raise ValueError(f"spectrum_from_sums: members must lie in [1, {NINT_ENS_MAX_M}], got {M}")
    if Wc < 2:
        raise ValueError(f"spectrum_from_sums: the width must be >= 2, got {Wc}")
    K = Wc // 2 + 1
    if spec.ndim != 4 or spec.shape[1] != NINT_SPEC_PLANES or spec.shape[3] != K or counts.shape != (spec.shape[0],):
        raise ValueError(f"spectrum_from_sums: spec must be (nslots, {NINT_SPEC_PLANES}, O, {K}) and counts (nslots,), got "
                         f"{spec.shape} and {counts.shape}")
    sel = list(range(spec.shape[0])) if slots is None else [int(v) for v in slots]
    yy, pp, cr, ci, ss = spec[sel].sum(axis=0)
    n = float(counts[sel].sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = _one_sided(Wc) / (float(Wc) * Wc * float(row_w_sum) * n) if n > 0 else np.full(K, np.nan)
        pt, pm, pe = yy * norm, pp / M * norm, ss / (M * M) * norm
        err = (ss / (M * M) + yy - 2.0 * cr / M) * norm
        coh = (cr * cr + ci * ci) / (ss * yy)
        return SpectrumReport(wavenumber=np.arange(K), power_target=pt, power_member=pm, power_mean=pe, power_error=err,
                              ratio_member=pm / pt, ratio_mean=pe / pt, coherence=coh, members=M, width=Wc, count=n)


class SpectrumAccumulator:
    """Device-side accumulator of zonal power spectra (nint_spec_accum): `spec` (nslots, 5, O, K) f64, the uploaded twiddle
    table (nint_spec_twiddles), `row_w` = cos(lat) and the kernel's scratch.  M = 1: a deterministic prediction.  `lat`,
    `halo`: as SkillAccumulator's.  The sums are additive: a data-parallel reduction adds the ranks' `spec` and `counts`."""

    def __init__(self, O: int, Hc: int, Wc: int, M: int = 1, nslots: int = 1, lat=None, device="cuda",
                 halo: Optional[Tuple[int, int]] = None):
        from . import _lib
        self.O, self.Hc, self.Wc, self.M, self.nslots = int(O), int(Hc), int(Wc), int(M), int(nslots)
        if self.nslots < 1:
            raise ValueError("nslots must be >= 1")
        if self.O < 1 or self.Hc < 1:
            raise ValueError(f"SpectrumAccumulator: O and Hc must be >= 1, got {(self.O, self.Hc)}")
        if not 1 <= self.M <= NINT_ENS_MAX_M:
            raise ValueError(f"SpectrumAccumulator: members must lie in [1, {NINT_ENS_MAX_M}], got {self.M}")
        if not 2 <= self.Wc <= NINT_SPEC_MAX_W:
            raise ValueError(f"SpectrumAccumulator: the crop width must lie in [2, {NINT_SPEC_MAX_W}], got {self.Wc}")
        self.K = self.Wc // 2 + 1
        self.row_w_host = None
        if lat is not None:
            lat = np.asarray(lat, dtype=np.float64)
            if lat.shape != (self.Hc,):
                raise ValueError(f"lat: expected {self.Hc} latitudes, got {lat.shape}")
            self.row_w_host = np.cos(np.deg2rad(lat))
        self.halo = None if halo is None else (int(halo[0]), int(halo[1]))
        self.lib = _lib.load()
        self.tw_host = np.empty((self.Wc, 2), dtype=np.float64)
        _lib.check(self.lib.nint_spec_twiddles(self.Wc, self.tw_host.ctypes.data_as(C.POINTER(C.c_double))), "nint_spec_twiddles")
        self.device = torch.device(device)
        self.tw = torch.from_numpy(self.tw_host).to(self.device)
        self.row_w = None if self.row_w_host is None else torch.from_numpy(self.row_w_host).to(self.device)
        self.spec = torch.zeros(self.nslots, NINT_SPEC_PLANES, self.O, self.K, dtype=torch.float64, device=self.device)
        self._counts = np.zeros(self.nslots, dtype=np.float64)
        self._scratch = None

    @property
    def counts(self) -> torch.Tensor:
        return torch.from_numpy(self._counts.copy()).to(self.device)

    @property
    def row_w_sum(self) -> float:
        return float(self.Hc) if self.row_w_host is None else float(self.row_w_host.sum())

    def scratch_for(self, N: int) -> torch.Tensor:
        need = self.lib.nint_spec_scratch_bytes(int(N), self.M, self.O, self.Hc, self.Wc) // 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        return self._scratch

    def update(self, pred: torch.Tensor, sample_off: Sequence[int], member_stride: int, y: torch.Tensor, slots=None,
               halo: Optional[Tuple[int, int]] = None):
        """Fold one batch in.  `pred`, `sample_off`, `member_stride`, `y`, `slots`: EnsembleAccumulator.update's -- member i of
        sample n is the (O, H, W) image at element sample_off[n] + i * member_stride of the contiguous f32 tensor `pred`,
        read in place.  `halo`: the crop's offset for this call (None: the accumulator's)."""
        from ._lib import check, ptr, stream_ptr
        if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() < 3 or pred.shape[-3] != self.O:
            raise ValueError(f"SpectrumAccumulator.update: pred must be a contiguous f32 tensor (..., {self.O}, H, W)")
        H, W = int(pred.shape[-2]), int(pred.shape[-1])
        off = [int(v) for v in sample_off]
        N, stride = len(off), int(member_stride)
        if N < 1 or stride < 0 or min(off) < 0 or max(off) + (self.M - 1) * stride + self.O * H * W > pred.numel():
            raise ValueError("SpectrumAccumulator.update: a member image lies outside pred")
        at = self.halo if halo is None else (int(halo[0]), int(halo[1]))
        oy, ox = ((H - self.Hc) // 2, (W - self.Wc) // 2) if at is None else at
        yv = y.detach().float().contiguous()
        if yv.numel() != N * self.O * self.Hc * self.Wc:
            raise ValueError("SpectrumAccumulator.update: target must be (N, O, Hc, Wc)")
        sl = [0] * N if slots is None else [int(v) for v in slots]
        if len(sl) != N or any(v < -1 or v >= self.nslots for v in sl):
            raise ValueError(f"slots: {N} values in [-1, {self.nslots}) expected")
        scratch = self.scratch_for(N)
        check(self.lib.nint_spec_accum(ptr(pred), (C.c_int64 * N)(*off), stride, self.M, ptr(yv), (C.c_int32 * N)(*sl), self.nslots,
                                       ptr(self.row_w), ptr(self.tw), ptr(self.spec), ptr(scratch), scratch.numel() * 8, N, self.O,
                                       H, W, int(oy), int(ox), self.Hc, self.Wc, stream_ptr()), "nint_spec_accum")
        for v in sl:
            if v >= 0:
                self._counts[v] += 1.0

    def update_from_pred(self, pred: torch.Tensor, y: torch.Tensor, halo: Optional[Tuple[int, int]] = None, slots=None):
        """One batch of deterministic predictions (N, O, H, W) that are already in memory (M = 1)."""
        if self.M != 1:
            raise ValueError(f"SpectrumAccumulator.update_from_pred is for M = 1; this accumulator has {self.M} members")
        pv = pred.detach().float().contiguous()
        if pv.dim() != 4 or pv.shape[1] != self.O:
            raise ValueError(f"SpectrumAccumulator.update_from_pred: pred must be (N, {self.O}, H, W)")
        img = int(pv.shape[1] * pv.shape[2] * pv.shape[3])
        self.update(pv, [n * img for n in range(pv.shape[0])], 0, y, slots, halo)

    def sums(self):
        """(spec, counts) as numpy: ONE device-to-host read"""
        return self.spec.cpu().numpy(), self._counts.copy()

    def report(self, slots: Optional[Sequence[int]] = None) -> SpectrumReport:
        spec, counts = self.sums()
        return spectrum_from_sums(spec, counts, self.M, self.Wc, self.row_w_sum, slots)

    def _check_rollout(self, who: str, O: int, Hc: int, Wc: int, M: int, horizon: int, halo):
        """a roll-out fills this accumulator only if its shapes are the roll-out's; refused before any device work"""
        want = (int(O), int(Hc), int(Wc), int(M), int(horizon), None if halo is None else (int(halo[0]), int(halo[1])))
        have = (self.O, self.Hc, self.Wc, self.M, self.nslots, self.halo)
        if want != have:
            raise ValueError(f"{who}: spectrum must be a SpectrumAccumulator with (O, Hc, Wc, M, nslots, halo) = {want}, got {have}")


LEAD_SPECTRUM_COLUMNS = ("small_scale_ratio_member", "small_scale_ratio_mean", "coherence_cut", "error_small_scale_frac")


def lead_spectrum_from_sums(spec, counts, M: int, Wc: int, kmin: Optional[int] = None) -> np.ndarray:
    """lead_time_spectrum on the raw sums (numpy f64, no device): (nslots, 4) in the order of LEAD_SPECTRUM_COLUMNS"""
    spec, counts = np.asarray(spec, np.float64), np.asarray(counts, np.float64)
    M, Wc = int(M), int(Wc)
    K = Wc // 2 + 1
    kmin = Wc // 8 if kmin is None else int(kmin)
    if not 0 <= kmin < K:
        raise ValueError(f"lead_time_spectrum: kmin must lie in [0, {K}), got {kmin}")
    c = _one_sided(Wc)
    out = np.full((spec.shape[0], len(LEAD_SPECTRUM_COLUMNS)), np.nan)
    for j in range(spec.shape[0]):
        if counts[j] <= 0:
            continue
        yy, pp, cr, ci, ss = spec[j].sum(axis=1)                                  # outputs pooled: (K,)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = c * (ss / (M * M) + yy - 2.0 * cr / M)
            small_y = (c * yy)[kmin:].sum()
            coh = (cr * cr + ci * ci) / (ss * yy)
            below = np.nonzero(coh < 0.5)[0]
            out[j] = [(c * pp)[kmin:].sum() / M / small_y, (c * ss)[kmin:].sum() / (M * M) / small_y,
                      float(below[0]) if below.size else float(K), err[kmin:].sum() / err.sum()]
    return out


def lead_time_spectrum(acc: SpectrumAccumulator, kmin: Optional[int] = None) -> np.ndarray:
    """Small-scale figures per slot of a SpectrumAccumulator (a roll-out: per lead time), outputs pooled: (nslots, 4) in the
    order of LEAD_SPECTRUM_COLUMNS -- the power of the members and of the ensemble mean at k >= kmin (default Wc // 8) over the
    target's, the smallest k whose pooled coherence falls under 0.5 (K if none), and the share of the mean's error power at
    k >= kmin; nan for an empty slot.  One device-to-host read."""
    spec, counts = acc.sums()
    return lead_spectrum_from_sums(spec, counts, acc.M, acc.Wc, kmin)


# ------------------------------------------------------------------------------ ensemble roll-outs by lead time
@torch.no_grad()
def rollout_ensemble(net, dataset, starts: Sequence[int], horizon: int, spinup: int, members: int, ic_noise=0.05,
                     feedback_noise=0.0, seed: int = 0, batch_size: int = 8, lat=None, halo: Optional[Tuple[int, int]] = None,
                     _allow_no_noise: bool = False, spectrum: Optional[SpectrumAccumulator] = None) -> EnsembleAccumulator:
    """Ensemble verification of the free-running model by LEAD TIME.  From every record step in `starts`,
    `members` copies of the window of `spinup + horizon` steps run closed loop from step `spinup` as lanes of one batch --
    lane start_index * members + m -- and differ by their noise alone:
      * `ic_noise` (std, z-score units): the input noise on the tracer channels with draw = 0.  The fed steps
        overwrite it, so it perturbs the spin-up -- the members' initial condition -- only;
      * `feedback_noise`: noise on every fed-back value (``net(..., feedback_noise=)``) with draw = 1.
    Both use `seed` and lane0 = start_index * members with the GLOBAL start index, so the noise of (start, member) does not
    depend on `batch_size`; a batch holds max(1, batch_size // members) starts.  The head runs at every step
    (head_forward_seq), the targets come from the record, and the statistics kernel (nint_ens_accum) reads the members where
    they lie; the prediction made `j` steps into the free run goes to slot j of the returned EnsembleAccumulator:
    ``lead_time_table(acc)``, ``acc.report(dataset.y_mean, dataset.y_std, slots=[j])``.

    `spectrum`: a SpectrumAccumulator(O, Hc, Wc, M=members, nslots=horizon, halo=halo) that is filled from the same members with
    the same offsets; a mismatch is a ValueError before any device work.  None: nothing changes.

    Refused: what rollout_skill refuses, `members` outside [2, 64], a negative or non-finite std, and both noises zero --
    the members would be identical and the ensemble would have no spread."""
    from .dataset import SlabBatch
    from .engine import InputNoise
    if not getattr(net, "feedback", False):
        raise ValueError("rollout_ensemble needs a ConvLSTM built with feedback=True")
    horizon, spinup = int(horizon), int(spinup)
    if horizon < 1 or spinup < 1:
        raise ValueError(f"rollout_ensemble: horizon and spinup must be >= 1, got {(horizon, spinup)}")
    if isinstance(members, bool) or int(members) != members or not 2 <= members <= NINT_ENS_MAX_M:
        raise ValueError(f"rollout_ensemble: members must be an integer in [2, {NINT_ENS_MAX_M}], got {members!r}")
    M, T = int(members), spinup + horizon
    starts = [int(v) for v in starts]
    n_steps = int(dataset.yraw.shape[0])
    lo = 1 if getattr(dataset, "tracer_input", False) else 0
    if not starts or min(starts) < lo or max(starts) + T > n_steps:
        raise ValueError(f"rollout_ensemble: every start must lie in [{lo}, {n_steps - T}] for windows of {T} steps in a record of {n_steps}")
    ic, fbn = InputNoise(ic_noise, seed=seed, draw=0), InputNoise(feedback_noise, seed=seed, draw=1)      # (a bad std or seed: ValueError)
    if not (ic.active or fbn.active or _allow_no_noise):
        raise ValueError("rollout_ensemble: ic_noise and feedback_noise are both zero -- the members would be identical and the "
                         "ensemble would have no spread; give at least one a positive std")
    O = net.conv.weight.shape[0]
    if O != dataset.levels:
        raise ValueError(f"rollout_ensemble: the head has {O} outputs, the record's tracer {dataset.levels} levels")
    if spectrum is not None:
        spectrum._check_rollout("rollout_ensemble", O, dataset.grid[0], dataset.grid[1], M, horizon, halo)
    net.eval()
    dev = next(net.parameters()).device
    eng = net._engine(dev)
    Hc, Wc = dataset.grid
    acc = EnsembleAccumulator(O, Hc, Wc, M, nslots=horizon, lat=lat, device=dev, halo=halo)
    dv = dataset._device_arrays()
    per = max(1, int(batch_size) // M)
    for s in range(0, len(starts), per):
        t0s = starts[s:s + per]
        X = SlabBatch(dataset, np.asarray([t for t in t0s for _ in range(M)]), T)
        B, _, _, H, W = X.shape
        lane = dict(seed=ic.seed, lane0=s * M)
        with eng.window(B, T, H, W, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, spinup), residual=_residual(net),
                        noise=InputNoise(ic.std, draw=0, **lane), feedback_noise=InputNoise(fbn.std, draw=1, **lane))
            seq = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(B, T, O, H, W)
        y = _step_targets(dataset, dv, t0s, T)                                    # (starts, T, L, Hc, Wc)
        img = O * H * W
        off = [((i * M) * T + spinup + j) * img for i in range(len(t0s)) for j in range(horizon)]
        acc.update(seq, off, T * img, y[:, spinup:].reshape(len(t0s) * horizon, O, Hc, Wc),
                   [j for _ in t0s for j in range(horizon)])
        if spectrum is not None:
            spectrum.update(seq, off, T * img, y[:, spinup:].reshape(len(t0s) * horizon, O, Hc, Wc),
                            [j for _ in t0s for j in range(horizon)])
    return acc
