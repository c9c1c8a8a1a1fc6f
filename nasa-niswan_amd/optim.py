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
the caller's stream, with no host read (include/nint.h has the arithmetic)."""
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
    reports what happened.  Both off (the default): the plain step, unchanged."""

    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not math.isfinite(max_grad_norm) or max_grad_norm < 0:
                raise ValueError(f"max_grad_norm must be a finite number >= 0 (or None), got {max_grad_norm!r}")
        self.flat = flat
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = max_grad_norm is not None or self.skip_nonfinite
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(flat.params, defaults)
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self._step = 0          # guarded: the count as of the last state_dict() / load_state_dict(); the live one is on the device
        if self.guarded:
            self._opt_state = torch.zeros(_lib.NINT_OPT_STATE, dtype=torch.float64, device=flat.data.device)
            self._norm_scratch = torch.empty(_lib.NINT_GRAD_NORM_BLOCKS, dtype=torch.float64, device=flat.data.device)
        self._bind_state()

    def _bind_state(self):
        for p, off in zip(self.flat.params, self.flat.offsets):
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
            for p in self.flat.params:
                self.state[p]["step"] = torch.tensor(float(self._step))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)      # torch-format dict (reference utils.py:42)
        steps = []
        for p, off in zip(self.flat.params, self.flat.offsets):
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
