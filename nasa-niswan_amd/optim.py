"""Flat parameter / gradient bucket and the fused Adam step (reference train.py:71,108-110).

``FlatParams`` re-homes every parameter of a module into ONE contiguous f32 buffer (and its
gradient into a second one).  That single bucket is what the HIP Adam kernel updates in one
launch and what RCCL all-reduces in one call under data parallelism: every ConvLSTM weight is
used at every time step, so all gradients become final together at the end of BPTT and there
is nothing to overlap bucket-by-bucket.

``FusedAdam`` subclasses ``torch.optim.Optimizer`` so that ``StepLR`` (train.py:72) drives it
unchanged and ``state_dict()`` is the torch Adam format (``state[i] = {step, exp_avg,
exp_avg_sq}``, ``param_groups``) -- reference checkpoints (utils.py:23-50) interchange.

With ``max_grad_norm`` and / or ``skip_nonfinite`` the step is ``nint_adam_flat_guarded``: the global L2 norm of the bucket,
``torch.nn.utils.clip_grad_norm_``'s coefficient and the decision to drop a non-finite step are all taken on the device, on
the caller's stream, with no host read (include/nint.h has the arithmetic).

Fine-tuning (``weight_decay``, ``freeze_layers``, ``layer_lr_scale``): the optimizer becomes ``torch.optim.AdamW`` over param
groups -- one per ConvLSTM layer that trains plus one for the head, each with its own ``lr`` -- and the step is
``nint_adam_flat_groups[_guarded]``: still one launch of the Adam body, over a table of ranges of the bucket built from
``param_groups``.  Frozen layers are in no group and no range: their weights and moments are never read or written."""
from __future__ import annotations

import ctypes as C
import math
from typing import Iterable, List

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


class FlatParams:
    def __init__(self, module: torch.nn.Module):
        self.params: List[torch.nn.Parameter] = [p for p in module.parameters()]
        if not self.params:
            raise ValueError("module has no parameters")
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.data = torch.empty(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.offsets = []
        off = 0
        for p in self.params:
            k = p.numel()
            self.data[off:off + k].copy_(p.detach().reshape(-1).float())
            p.data = self.data[off:off + k].view(p.shape)        # the parameter now aliases the bucket
            p.grad = self.grad[off:off + k].view(p.shape)        # and so does its .grad
            self.offsets.append(off)
            off += k
        self.numel = n

    def grad_view(self, i: int) -> torch.Tensor:
        p = self.params[i]
        return self.grad[self.offsets[i]:self.offsets[i] + p.numel()].view(p.shape)

    def is_intact(self) -> bool:
        """False once something (``.to()``, ``load_state_dict(assign=True)``...) re-allocated a parameter."""
        base = self.data.data_ptr()
        return all(p.data_ptr() == base + 4 * o for p, o in zip(self.params, self.offsets))


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (eps 1e-8, no weight decay, no amsgrad) in one HIP launch.

    ``max_grad_norm`` (a finite number >= 0; 0 = measure the norm, never clip) and ``skip_nonfinite`` switch the guarded step
    on: three launches, the step's scalars and the applied-step count live in a small device buffer, and ``grad_stats()``
    reports what happened.  Both off (the default): the plain step, unchanged.

    ``weight_decay`` (decoupled, AdamW), ``freeze_layers`` (the first n ConvLSTM layers are not trained: in no group, and
    ``requires_grad_(False)``) and ``layer_lr_scale`` (one factor on ``lr`` per ConvLSTM layer, optionally one more for the
    head; without it the head takes the last layer's) switch the grouped step on.  ``flat`` must then be the bucket of a
    ConvLSTM: (weight, bias) per layer, then the head's.  Decay applies to weights; biases (1-D parameters) get none, whatever
    their group's ``weight_decay`` says -- the torch equivalent is AdamW with the biases in zero-decay groups of their own.
    ``StepLR`` drives every group's ``lr``; ``state_dict()`` is torch AdamW's over the trainable parameters.  All three at
    their defaults: one group, the two plain entries, what this class has always built."""

    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False,
                 weight_decay=0.0, freeze_layers=0, layer_lr_scale=None):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not math.isfinite(max_grad_norm) or max_grad_norm < 0:
                raise ValueError(f"max_grad_norm must be a finite number >= 0 (or None), got {max_grad_norm!r}")
        self.flat = flat
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = max_grad_norm is not None or self.skip_nonfinite
        self.grouped, groups = self._layer_groups(flat, lr, weight_decay, freeze_layers, layer_lr_scale)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        if self.grouped:
            defaults.update(weight_decay=float(weight_decay), decoupled_weight_decay=True)
        super().__init__(groups, defaults)
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self._step = 0          # guarded: the count as of the last state_dict() / load_state_dict(); the live one is on the device
        if self.guarded:
            self._opt_state = torch.zeros(_lib.NINT_OPT_STATE, dtype=torch.float64, device=flat.data.device)
            self._norm_scratch = torch.empty(_lib.NINT_GRAD_NORM_BLOCKS, dtype=torch.float64, device=flat.data.device)
            if self.grouped:       # each group's step size and decay multiplier of the guarded step (nint.h)
                self._group_state = torch.zeros(2 * _lib.NINT_MAX_OPT_GROUPS, dtype=torch.float64, device=flat.data.device)
        self._bind_state()

    def _layer_groups(self, flat, lr, weight_decay, freeze_layers, layer_lr_scale):
        """(grouped?, what torch.optim.Optimizer takes as params): every parameter as one group by default; else one group per
        trained ConvLSTM layer and one for the head, the frozen layers switched off.  ``self.n0`` / ``self.trained``: the
        first trained element of the bucket and the (parameter, offset) pairs behind it."""
        weight_decay, freeze_layers = float(weight_decay), int(freeze_layers)
        if not math.isfinite(weight_decay) or weight_decay < 0:
            raise ValueError(f"weight_decay must be a finite number >= 0, got {weight_decay!r}")
        self.n0, self.trained, self.lr_scales = 0, list(zip(flat.params, flat.offsets)), [1.0]
        if weight_decay == 0 and freeze_layers == 0 and layer_lr_scale is None:
            return False, flat.params
        n = len(flat.params)
        L = (n - 2) // 2
        if n < 4 or n % 2 or L > _lib.NINT_MAX_LAYERS or any(flat.params[2 * l].dim() != 4 or flat.params[2 * l + 1].dim() != 1
                                                             for l in range(L + 1)):
            raise ValueError("weight_decay / freeze_layers / layer_lr_scale need the bucket of a ConvLSTM: (weight, bias) of every "
                             "layer, then the head's")
        if not 0 <= freeze_layers <= L:
            raise ValueError(f"freeze_layers must be in [0, {L}], got {freeze_layers}")
        scale = [1.0] * (L + 1) if layer_lr_scale is None else [float(v) for v in layer_lr_scale]
        if len(scale) == L:
            scale.append(scale[-1])                  # the head goes with the top layer
        if len(scale) != L + 1 or any(not math.isfinite(v) or v < 0 for v in scale):
            raise ValueError(f"layer_lr_scale must hold {L} (or {L + 1}, the head's last) finite factors >= 0, got {layer_lr_scale!r}")
        for p in flat.params[:2 * freeze_layers]:
            p.requires_grad_(False)
        self.n0 = flat.offsets[2 * freeze_layers]
        self.trained = self.trained[2 * freeze_layers:]
        self.lr_scales = scale[freeze_layers:]           # per param group: what a later change of the base lr keeps
        return True, [dict(params=flat.params[2 * l:2 * l + 2], lr=lr * scale[l]) for l in range(freeze_layers, L + 1)]

    def group_table(self):
        """nint_opt_group[] of this step, from ``param_groups`` as they are now (a scheduler may have moved every ``lr``): one
        range per parameter -- a bias never decays --, neighbours with equal (lr, decay) merged.  The ranges tile the trained
        tail of the bucket."""
        off = {id(p): o for p, o in self.trained}
        rows = []
        for g in self.param_groups:
            for p in g["params"]:
                row = [off[id(p)], off[id(p)] + p.numel(), float(g["lr"]), float(g["weight_decay"]) if p.dim() > 1 else 0.0]
                if rows and rows[-1][1] == row[0] and rows[-1][2:] == row[2:]:
                    rows[-1][1] = row[1]
                else:
                    rows.append(row)
        return (_lib.NintOptGroup * len(rows))(*[_lib.NintOptGroup(*r) for r in rows])

    def _bind_state(self):
        for p, off in self.trained:
            k = p.numel()
            self.state[p] = {"step": torch.tensor(float(self._step)),
                             "exp_avg": self.exp_avg[off:off + k].view(p.shape),
                             "exp_avg_sq": self.exp_avg_sq[off:off + k].view(p.shape)}

    def zero_grad(self, set_to_none: bool = False):
        # one memset of the bucket; the .grad views stay aliased (reference call site: train.py:108).
        # The fused trainer never needs it: its backward overwrites the bucket.
        self.flat.grad.zero_()

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        if not self.flat.is_intact():
            raise RuntimeError("a parameter was re-allocated after FlatParams was built; rebuild the optimizer")
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        if self.grouped:
            return self._step_grouped(float(b1), float(b2), float(g["eps"]), float(grad_scale))
        if self.guarded:
            # the step number is state[NINT_OPT_APPLIED] + 1 on the device: a skipped step does not advance it
            check(_lib.load().nint_adam_flat_guarded(
                ptr(self.flat.data), ptr(self.flat.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), self.flat.numel,
                float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(grad_scale), self.max_grad_norm or 0.0,
                int(self.skip_nonfinite), ptr(self._opt_state), ptr(self._norm_scratch), 8 * self._norm_scratch.numel(),
                stream_ptr()), "nint_adam_flat_guarded")
            return None
        self._step += 1
        check(_lib.load().nint_adam_flat(ptr(self.flat.data), ptr(self.flat.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq),
                                         self.flat.numel, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                                         self._step, float(grad_scale), stream_ptr()), "nint_adam_flat")
        for p in self.flat.params:
            self.state[p]["step"] = torch.tensor(float(self._step))
        return None

    def _step_grouped(self, b1: float, b2: float, eps: float, grad_scale: float):
        """the grouped step: the table of this step's ranges, then ONE call -- guarded or plain, as step() chooses"""
        lib, fl, tab = _lib.load(), self.flat, self.group_table()
        if self.guarded:
            check(lib.nint_adam_flat_groups_guarded(
                ptr(fl.data), ptr(fl.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), tab, len(tab), b1, b2, eps, grad_scale,
                self.max_grad_norm or 0.0, int(self.skip_nonfinite), ptr(self._opt_state), ptr(self._group_state),
                ptr(self._norm_scratch), 8 * self._norm_scratch.numel(), stream_ptr()), "nint_adam_flat_groups_guarded")
            return None
        self._step += 1
        check(lib.nint_adam_flat_groups(ptr(fl.data), ptr(fl.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), tab, len(tab), b1, b2,
                                        eps, self._step, grad_scale, stream_ptr()), "nint_adam_flat_groups")
        for p, _ in self.trained:
            self.state[p]["step"] = torch.tensor(float(self._step))
        return None

    def grad_stats(self, reset: bool = False) -> dict:
        """What the guarded steps did, in one device read: ``applied`` (Adam steps taken, the bias-correction count; never
        reset), ``skipped`` (non-finite gradients dropped), ``clipped`` (steps with a coefficient below 1), ``calls``,
        ``mean_norm`` / ``max_norm`` of the scaled gradient over the calls with a finite norm, and the last call's
        ``last_norm`` / ``last_coef``.  ``reset=True`` zeroes everything but ``applied`` afterwards (per-epoch figures)."""
        if not self.guarded:
            raise RuntimeError("grad_stats() needs the guarded step: construct with max_grad_norm and / or skip_nonfinite")
        s = self._opt_state.cpu().tolist()
        if reset:
            self._opt_state[_lib.NINT_OPT_SKIPPED:_lib.NINT_OPT_MAX_NORM + 1].zero_()
        finite = s[_lib.NINT_OPT_FINITE]
        return {"applied": int(s[_lib.NINT_OPT_APPLIED]), "skipped": int(s[_lib.NINT_OPT_SKIPPED]),
                "clipped": int(s[_lib.NINT_OPT_CLIPPED]), "calls": int(s[_lib.NINT_OPT_CALLS]),
                "mean_norm": s[_lib.NINT_OPT_SUM_NORM] / finite if finite else float("nan"),
                "max_norm": s[_lib.NINT_OPT_MAX_NORM], "last_norm": s[_lib.NINT_OPT_NORM], "last_coef": s[_lib.NINT_OPT_COEF]}

    def state_dict(self):
        if self.guarded:
            # the one host read of the guarded path, at checkpoint time: `step` of every parameter = applied steps
            self._step = int(self._opt_state[_lib.NINT_OPT_APPLIED].item())
            for p, _ in self.trained:
                self.state[p]["step"] = torch.tensor(float(self._step))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)      # torch-format dict (reference utils.py:42)
        steps = []
        for p, off in self.trained:
            st = self.state.get(p, {})
            k = p.numel()
            if "exp_avg" in st:
                self.exp_avg[off:off + k].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                steps.append(int(float(st["step"])))
        self._step = max(steps) if steps else 0
        if self.guarded:
            self._opt_state[_lib.NINT_OPT_APPLIED] = float(self._step)
        self._bind_state()
