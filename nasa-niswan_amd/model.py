"""Drop-in ``ConvLSTMCell`` / ``ConvLSTM`` for the reference's ``model.py`` (lines 196-274).

Same constructor signatures, same module tree and ``state_dict`` keys
(``layers.{i}.conv.weight|bias``, ``conv.weight|bias``: test.ipynb:4698-4699), same return
values -- but ``forward`` runs the MI355X HIP kernels through the C ABI (include/nint.h).
``nn.Conv2d`` objects are kept purely as parameter containers (identical default init under
the same seed, identical checkpoint keys); they are never called.

Extensions are keyword-only with reference-preserving defaults:
    compute_dtype   "f32" (exact-parity mode) or "bf16" (bf16 storage, f32 accumulate)
    out_channels    head width (1 in the reference, L*n_tracers for the level-fused variants)
    return_sequence also return the per-step head outputs (the variant the analysis notebook
                    was run with: model.py:264,272,274 commented code, test.ipynb:273); differentiable:
                    gradients flow through ``seq`` as through ``pred``
"""
from __future__ import annotations

import functools
import weakref
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
from torch._C import _functions

from .engine import LayerCfg, SeqEngine, dtype_code

__all__ = ["ConvLSTMCell", "ConvLSTM"]


def _require_cuda(t: torch.Tensor, who: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"{who}: tensors must live on the MI355X (cuda) -- this package has no CPU path; "
                           "move the module and its inputs with .cuda()")


class _Releaser:
    """Returns a workspace to the engine pool when the autograd graph that owns it dies."""

    def __init__(self, ws):
        self.ws = ws
        self._fin = weakref.finalize(self, SeqEngine.release, ws)

    def release(self):
        self._fin()


def _once_differentiable(fn):
    """torch's ``once_differentiable`` with one difference.  The backward kernels run outside autograd, so under
    ``create_graph=True`` the gradients they return carry no graph; torch's decorator hangs its error node on them only when a
    COTANGENT requires grad, and the cotangent of ``(net(x) * r).sum()`` does not -- a gradient penalty built on dx would
    then contribute nothing and nothing would say so.  Here every returned gradient gets the error node whenever a graph is
    being recorded: double backward is refused, never dropped."""

    @functools.wraps(fn)
    def wrapper(ctx, *args):
        with torch.no_grad():
            outputs = fn(ctx, *args)
        if not torch.is_grad_enabled():
            return outputs
        err = _functions.DelayedError(
            "trying to differentiate twice through ConvLSTM / ConvLSTMCell: double backward is not supported -- the backward "
            "pass runs HIP kernels outside autograd, so a gradient taken with create_graph=True is a constant", len(outputs))
        return err(*[None if v is None else v.detach().requires_grad_(True) for v in outputs])

    return wrapper


def _own_workspace(ctx, who: str):
    """The workspace a graph recorded into is its own only until its backward (or death) returns it to the pool: a forward
    that acquired it since has overwritten the activations.  Refuse instead of running BPTT over another batch's."""
    if ctx.ws.gen != ctx.gen:
        raise RuntimeError(f"{who}: this graph was retained (retain_graph=True) across another forward of the same shape, which "
                           "reused its workspace after the first backward() released it -- the stored activations are gone. "
                           "Run every backward of a retained graph before the next forward of that shape, or run the forward "
                           "again.")
    return ctx.eng, ctx.ws


# ------------------------------------------------------------------------------ autograd glue
class _ConvLSTMFn(torch.autograd.Function):
    """x, head_w, head_b, W_0, b_0, ..., W_{L-1}, b_{L-1} -> pred [, seq]"""

    @staticmethod
    def forward(ctx, module, grad_mode, x, head_w, head_b, *wb):
        eng: SeqEngine = module._engine(x.device)
        B, T, _, H, W = x.shape
        # grad mode is always off inside Function.forward, so the caller samples it
        train = grad_mode and any(ctx.needs_input_grad)
        ws = eng.acquire(B, T, H, W, train, False)
        eng.pack_weights(wb[0::2], wb[1::2])
        eng.forward(ws, x)
        pred = eng.head_forward(ws, head_w, head_b)
        outs = [pred]
        if module.return_sequence:
            outs.append(eng.head_forward_seq(ws, head_w, head_b))       # every step in one launch
        ctx.return_sequence = module.return_sequence
        if train:
            if module.return_sequence:
                ctx.set_materialize_grads(False)                        # an unused output's cotangent stays None: passed as NULL
            ctx.eng, ctx.ws, ctx.rel, ctx.gen = eng, ws, _Releaser(ws), ws.gen
            # references, not copies: the dgrad reads the engine's packed image of these weights (eng.Wd), which every forward
            # rewrites -- torch's version check on the saved tensors is what refuses a backward after an in-place update
            ctx.save_for_backward(head_w, *wb[0::2])
            ctx.x_needs_grad = ctx.needs_input_grad[2]
            ctx.nwb = len(wb)
        else:
            eng.release(ws)
        return tuple(outs) if len(outs) > 1 else pred

    @staticmethod
    @_once_differentiable
    def backward(ctx, dpred, dseq=None):
        eng, ws = _own_workspace(ctx, "ConvLSTM")
        head_w = ctx.saved_tensors[0]           # before the first launch: raises if a weight was modified in place
        L = len(eng.cfgs)
        if ctx.return_sequence:
            if dpred is None and dseq is None:
                ctx.rel.release()
                return (None,) * (5 + ctx.nwb)
            # per-step head gradients (pred's cotangent joins step T-1), then BPTT with one block of them per time step
            dw_head, db_head = eng.head_backward_seq(ws, head_w, dseq, dpred)
            dWs, dbs, dx = eng.backward(ws, ctx.x_needs_grad, zero_state_grads=range(L), seq_grads=True)
        else:
            dw_head, db_head = eng.head_backward(ws, head_w, dpred)
            dWs, dbs, dx = eng.backward(ws, ctx.x_needs_grad, zero_state_grads=range(L))
        ctx.rel.release()
        grads = []
        for l in range(L):
            grads += [dWs[l], dbs[l]]
        return (None, None, dx, dw_head, db_head, *grads)


class _CellFn(torch.autograd.Function):
    """x, h, c, W, b -> h', c'   (model.py:216-231)"""

    @staticmethod
    def forward(ctx, module, grad_mode, x, h, c, W, b):
        eng: SeqEngine = module._engine(x.device)
        B, _, H, Wd = x.shape
        train = grad_mode and any(ctx.needs_input_grad)
        ws = eng.acquire(B, 1, H, Wd, train, True)
        eng.pack_weights([W], [b])
        eng.forward(ws, x.unsqueeze(1), [h], [c])
        h1, c1 = eng.h_last(ws, 0), eng.c_last(ws, 0)
        if train:
            ctx.eng, ctx.ws, ctx.rel, ctx.gen = eng, ws, _Releaser(ws), ws.gen
            ctx.save_for_backward(W)            # (a reference: see _ConvLSTMFn)
            ctx.x_needs_grad = ctx.needs_input_grad[2]
            ctx.has_bias = b is not None
        else:
            eng.release(ws)
        return h1, c1

    @staticmethod
    @_once_differentiable
    def backward(ctx, dh1, dc1):
        eng, ws = _own_workspace(ctx, "ConvLSTMCell")
        ctx.saved_tensors                       # before the first launch: raises if the weight was modified in place
        eng.set_state_grads(ws, 0, dh1, dc1)
        dWs, dbs, dx = eng.backward(ws, ctx.x_needs_grad)
        dh0, dc0 = eng.state_grads(ws, 0)
        ctx.rel.release()
        if dx is not None:
            dx = dx[:, 0]
        return None, None, dx, dh0, dc0, dWs[0], (dbs[0] if ctx.has_bias else None)


class _EngineOwner:
    """Mixin: the per-device engines hold device workspaces and ctypes structures; they are rebuilt on
    demand and must not travel with pickling / copy.deepcopy of the module."""

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engines"] = {}
        return state


# ------------------------------------------------------------------------------ modules
class ConvLSTMCell(_EngineOwner, nn.Module):
    """reference model.py:196-231"""

    def __init__(self, input_channels, hidden_channels, kernel_size, bias=True, *, compute_dtype="f32"):
        super().__init__()
        self.input_channels = input_channels
        self.hidden_channels = hidden_channels
        self.kernel_size = kernel_size
        self.padding = kernel_size // 2
        self.bias = bias
        # parameter container with the reference's name, shape, layout and default init
        # (out-channel order [i,f,g,o], in-channel order [x..., h...]; model.py:207-211,219-221)
        self.conv = nn.Conv2d(in_channels=self.input_channels + self.hidden_channels,
                              out_channels=4 * self.hidden_channels, kernel_size=self.kernel_size,
                              padding=self.padding, bias=self.bias)
        self.sigmoid = nn.Sigmoid()
        self.tanh = nn.Tanh()
        self.compute_dtype = compute_dtype
        self._engines = {}

    def _engine(self, device) -> SeqEngine:
        key = (str(device), dtype_code(self.compute_dtype))
        if key not in self._engines:
            self._engines[key] = SeqEngine([LayerCfg(self.input_channels, self.hidden_channels, self.kernel_size)],
                                           self.compute_dtype, device)
        return self._engines[key]

    def forward(self, x, hidden_state):
        h, c = hidden_state
        _require_cuda(x, "ConvLSTMCell")
        return _CellFn.apply(self, torch.is_grad_enabled(), x, h, c, self.conv.weight, self.conv.bias)


class ConvLSTM(_EngineOwner, nn.Module):
    """reference model.py:234-274"""

    def __init__(self, input_channels, hidden_channels, kernel_size, num_layers, *, out_channels=1,
                 return_sequence=False, compute_dtype="f32"):
        super().__init__()
        assert len(hidden_channels) == num_layers, 'The length of hidden_channels must be equal to num_layers.'
        self.num_layers = num_layers
        self.layers = nn.ModuleList()
        self.layers.append(ConvLSTMCell(input_channels, hidden_channels[0], kernel_size[0], compute_dtype=compute_dtype))
        for i in range(1, num_layers):
            self.layers.append(ConvLSTMCell(hidden_channels[i - 1], hidden_channels[i], kernel_size[i],
                                            compute_dtype=compute_dtype))
        # Bottleneck layer (model.py:251)
        self.conv = nn.Conv2d(hidden_channels[-1], out_channels, kernel_size=1)
        self.return_sequence = return_sequence
        self.compute_dtype = compute_dtype
        self._engines = {}

    def _engine(self, device) -> SeqEngine:
        key = (str(device), dtype_code(self.compute_dtype))
        if key not in self._engines:
            cfgs = [LayerCfg(c.input_channels, c.hidden_channels, c.kernel_size) for c in self.layers]
            self._engines[key] = SeqEngine(cfgs, self.compute_dtype, device)
        return self._engines[key]

    def forward(self, x):
        # x: (batch_size, sequence_length, channels, height, width)  (model.py:254)
        _require_cuda(x, "ConvLSTM")
        wb = []
        for cell in self.layers:
            wb += [cell.conv.weight, cell.conv.bias]
        return _ConvLSTMFn.apply(self, torch.is_grad_enabled(), x, self.conv.weight, self.conv.bias, *wb)
