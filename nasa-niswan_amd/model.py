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
    lon_cyclic      ConvLSTM only: cyclic longitude -- column 0 and column W-1 of the grid are neighbours in every
                    convolution of the stack (rows keep the zero padding); same parameters, same ``state_dict``
                    

Carried state (no reference code: model.py:259-262 always starts from zeros and drops the final state):
``ConvLSTM.forward(x, state=None, *, return_state=False)`` takes ``(h0, c0)`` of every layer and returns ``(h_T, c_T)``, as
tensors (differentiable: chaining two calls is full BPTT across the boundary) or as a ``ConvLSTMState`` that stays on the
device in slab form (detached: truncated BPTT).  DESIGN.md 4.10.
"""
from __future__ import annotations

import functools
import weakref
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
from torch._C import _functions

from .engine import RESIDUAL_STEP0, ConvLSTMState, Feedback, InputNoise, LayerCfg, SeqEngine, dtype_code

__all__ = ["ConvLSTMCell", "ConvLSTM", "ConvLSTMState", "InputNoise"]


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
def _keep_or_release(ctx, eng, ws, train: bool, *weights):
    """The end of every Function.forward.  A graph that will run backward keeps its workspace until then (or until it dies)
    and saves REFERENCES to the weights, not copies: the dgrad reads the engine's packed image of them (eng.Wd), which every
    forward rewrites -- torch's version check on the saved tensors is what refuses a backward after an in-place update.
    Anything else returns the workspace to the pool now."""
    if train:
        ctx.eng, ctx.ws, ctx.rel, ctx.gen = eng, ws, _Releaser(ws), ws.gen
        ctx.save_for_backward(*weights)
    else:
        eng.release(ws)


def _interleave(a, b):
    """[a_0, b_0, a_1, b_1, ...]: the order the Functions take the layers' (W, b) and (h, c) in, and return their gradients in"""
    return [v for pair in zip(a, b) for v in pair]


def train_from_rule(x_needs: bool, layer_needs: Sequence[bool]) -> int:
    """The first layer BPTT has to reach (nint_seq.train_from), from what needs a gradient: 0 if the input does (its gradient
    passes through every layer); else the lowest layer l one of whose tensors -- W_l, b_l, or a tensor state h0_l / c0_l --
    does (``layer_needs[l]``); L if none does (the head alone is trained).  Pure."""
    if x_needs:
        return 0
    return next((l for l, need in enumerate(layer_needs) if need), len(layer_needs))


_NO_FEEDBACK_GRAD = ("ConvLSTM: back-propagation through the fed-back prediction (free_from < T under grad mode with "
                     "an input, parameter or state that requires grad) is not implemented; run the closed loop "
                     "under torch.no_grad(), or train teacher-forced (free_from=None)")


class _CallOpts:
    """the non-tensor arguments of _ConvLSTMFn: the device state that comes in (or None), what goes out, the box the outgoing
    device state is handed back in (a Function's outputs are tensors), and the default route's head-backward rule"""

    def __init__(self, state_in=None, return_state=False, seq_always=False, free_from=None, feedback_grad=False, residual=False,
                 noise=None, fnoise=None):
        self.state_in, self.return_state, self.state_out = state_in, return_state, None
        self.noise = noise              # an InputNoise with its span resolved, or None
        self.fnoise = fnoise            # the noise on the fed-back value: an InputNoise with O sigmas, or None
        self.free_from = free_from      # closed loop from this step on (ConvLSTM(feedback=True)); None: open loop
        self.residual = residual        # the module's head predicts the increment (ConvLSTM(residual=True))
        # ... or a (B, T) feed mask (scheduled sampling); `first`: the first step that feeds anything
        self.first = free_from if free_from is None or isinstance(free_from, int) else Feedback.first_fed(free_from)
        self.feedback_grad = feedback_grad and free_from is not None    # ... and differentiated through what it feeds back (4.19)
        # The default call (no state in, none out) of a return_sequence module ALWAYS takes the per-step head backward
        # (head_backward_seq + BPTT with seq_grads), also when only `pred` has a cotangent; a call with state does so only
        # when `seq` has one.  Two launch plans and two summation orders of dw_head: kept apart, as they have always been.
        self.seq_always = seq_always


class _ConvLSTMFn(torch.autograd.Function):
    """x, head_w, head_b, W_0, b_0, ..., W_{L-1}, b_{L-1} [, h0_0, c0_0, ..., h0_{L-1}, c0_{L-1}]
    -> pred [, seq] [, hT_0, cT_0, ..., hT_{L-1}, cT_{L-1}]

    The one Function of ConvLSTM: the default call is the case with no state in and none out, which launches what it
    always did.  Tensor states are inputs and outputs of the Function: dL/dh0, dL/dc0 come from the BPTT's own d/dh_init,
    d/dc_init, and the cotangents of the returned states enter BPTT as the incoming dh[l] / dc[l].  A ConvLSTMState in or
    out is not seen by autograd."""

    @staticmethod
    def forward(ctx, module, grad_mode, opts, x, head_w, head_b, *rest):
        eng: SeqEngine = module._engine(x.device)
        L = len(eng.cfgs)
        wb, st = rest[:2 * L], rest[2 * L:]
        B, T, _, H, W = x.shape
        # grad mode is always off inside Function.forward, so the caller samples it
        train = grad_mode and any(ctx.needs_input_grad)
        has_init = opts.state_in is not None or len(st) > 0
        # requires_grad_(False) on the lower layers is fine-tuning: BPTT stops above them and they keep no stash
        need = ctx.needs_input_grad
        f = train_from_rule(need[3], [any(need[6 + 2 * l:8 + 2 * l]) or (len(st) > 0 and any(need[6 + 2 * L + 2 * l:8 + 2 * L + 2 * l]))
                                      for l in range(L)]) if train else 0
        # a fed step's input depends on every layer of the step before: the gradient passes through all of them
        rollout = train and opts.feedback_grad and bool(Feedback.steps(opts.first, T))
        if rollout:
            f = 0
        ws = eng.acquire(B, T, H, W, train, has_init, f)
        eng.pack_weights(wb[0::2], wb[1::2])
        if opts.state_in is not None:
            eng.load_state(ws, opts.state_in)
        h0, c0 = (list(st[0::2]), list(st[1::2])) if st else (None, None)
        eng.forward(ws, x, h0, c0, feedback=None if opts.free_from is None else (head_w, head_b, opts.free_from),
                    feedback_grad=rollout, residual=head_w.shape[0] if opts.residual else False, noise=opts.noise,
                    feedback_noise=opts.fnoise)
        outs = [eng.head_forward(ws, head_w, head_b)]
        if module.return_sequence:
            outs.append(eng.head_forward_seq(ws, head_w, head_b))       # every step in one launch
        if opts.return_state == "device":
            opts.state_out = eng.save_state(ws)
        elif opts.return_state:
            for l in range(L):
                outs += [eng.h_last(ws, l), eng.c_last(ws, l)]
        ctx.set_materialize_grads(False)        # a missing cotangent stays None: passed as NULL, or that state keeps its zero_dstate bit
        _keep_or_release(ctx, eng, ws, train, head_w, *wb[0::2])
        ctx.return_sequence, ctx.seq_always = module.return_sequence, opts.seq_always
        ctx.x_needs_grad = ctx.needs_input_grad[3]
        ctx.nwb, ctx.nst = len(wb), len(st)
        ctx.st_needs_grad = any(ctx.needs_input_grad[6 + len(wb):])
        ctx.train_from, ctx.rollout = f, rollout
        return tuple(outs) if len(outs) > 1 else outs[0]

    @staticmethod
    @_once_differentiable
    def backward(ctx, *douts):
        eng, ws = _own_workspace(ctx, "ConvLSTM")
        head_w = ctx.saved_tensors[0]           # before the first launch: raises if a weight was modified in place
        L = len(eng.cfgs)
        nin = 6 + ctx.nwb + ctx.nst
        n0 = 2 if ctx.return_sequence else 1
        dpred = douts[0]
        dseq = douts[1] if ctx.return_sequence else None
        dst = list(douts[n0:]) + [None] * (2 * L - len(douts[n0:]))     # (hT_0, cT_0, ...): all None without tensor states out
        if all(d is None for d in douts):
            ctx.rel.release()
            return (None,) * nin
        # the top layer: the head's dL/dh_{T-1} (per step with a sequence cotangent) plus the cotangent of the returned h_{T-1}
        dh_top = dst[2 * (L - 1)]
        dw_head, db_head, seq_grads, slab = _head_backward(ctx, eng, ws, head_w, dpred, dseq)
        if dw_head is None and slab is None:    # no head gradient at all: the state's cotangent alone (zeros if there is none)
            eng.set_dstate(ws, L - 1, "h", dh_top)
        elif dh_top is not None:
            eng.add_top_dh(ws, dh_top, seq_grads)
        mask, f = 0, ctx.train_from
        for l in range(f, L):                   # (a frozen layer's returned state feeds nothing that wants a gradient)
            dh, dc = dst[2 * l], dst[2 * l + 1]
            if dc is None:
                mask |= 1 << (2 * l)
            else:
                eng.set_dstate(ws, l, "c", dc)
            if l < L - 1:
                if dh is None:
                    mask |= 1 << (2 * l + 1)
                else:
                    eng.set_dstate(ws, l, "h", dh)
        dWs, dbs, dx = eng.backward(ws, ctx.x_needs_grad, seq_grads=seq_grads, zero_mask=mask, train_from=f, rollout=slab)
        if slab is not None:
            dw_head, db_head = eng.rollout_head_backward(ws, head_w, slab)
        elif dx is not None and ws.feedback.res:        # residual head, nothing fed: the skip path into x is the head cotangent
            eng.add_skip_dx(dx, head_w.shape[0], dseq=dseq, dpred=dpred)
        dstate = []
        if ctx.nst:
            for l in range(L):
                dstate += list(eng.state_grads(ws, l)) if ctx.st_needs_grad and l >= f else [None, None]
        ctx.rel.release()
        return (None, None, None, dx, dw_head, db_head, *_interleave(dWs, dbs), *dstate)


def _head_backward(ctx, eng, ws, head_w, dpred, dseq):
    """The head's part of _ConvLSTMFn.backward, ahead of BPTT: (dw_head, db_head, seq_grads, slab).  A roll-out: the head's
    cotangents travel as a slab, which comes back holding what the feedback added -- the head's own gradients are reduced from
    it afterwards.  Else the per-step head backward (the default route's rule: _CallOpts), or the last step's, or nothing."""
    seq_grads = dseq is not None or ctx.seq_always
    if ctx.rollout:
        return None, None, True, eng.rollout_cotangents(ws, head_w, dseq, dpred)
    if seq_grads:
        return (*eng.head_backward_seq(ws, head_w, dseq, dpred), True, None)
    if dpred is not None:
        return (*eng.head_backward(ws, head_w, dpred), False, None)
    return None, None, False, None


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
        _keep_or_release(ctx, eng, ws, train, W)
        ctx.x_needs_grad = ctx.needs_input_grad[2]
        ctx.has_bias = b is not None
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
        dW, db = _interleave(dWs, dbs)
        return None, None, dx, dh0, dc0, dW, (db if ctx.has_bias else None)


class _EngineOwner:
    """Mixin: the per-device engines hold device workspaces and ctypes structures; they are rebuilt on
    demand and must not travel with pickling / copy.deepcopy of the module."""

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engines"] = {}
        return state


# ------------------------------------------------------------------------------ modules
class ConvLSTMCell(_EngineOwner, nn.Module):
    """reference model.py:196-231.  A cell called by itself always zero-pads: cyclic longitude (``ConvLSTM(lon_cyclic=True)``)
    is a property of the whole-sequence passes, and the cells of such a net are parameter containers like any other."""

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
                 return_sequence=False, compute_dtype="f32", lon_cyclic=False, feedback=False, residual=False):
        super().__init__()
        assert len(hidden_channels) == num_layers, 'The length of hidden_channels must be equal to num_layers.'
        # closed loop: the last out_channels input channels are FEEDBACK channels, which forward(free_from=s)
        # fills with the head's own output from step s on.  Not a parameter and not in the state_dict; without free_from the
        # module is, bit for bit, the module without it.
        self.feedback = bool(feedback)
        if self.feedback and not 1 <= out_channels <= input_channels:
            raise ValueError(f"ConvLSTM(feedback=True): the {out_channels} head outputs are fed back into the last input channels, "
                             f"so out_channels <= input_channels ({input_channels}) is required")
        # residual head: the head predicts the tracer's tendency, p_t = x_t[feedback channels] + head(h_t), x_t
        # as the model saw it.  Like `feedback`: not a parameter, not in the state_dict.
        self.residual = bool(residual)
        if self.residual and not self.feedback:
            raise ValueError("ConvLSTM(residual=True) needs feedback=True: the increment is added to the feedback channels, the last "
                             "out_channels input channels")
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
        # cyclic longitude: not a parameter and not in the state_dict -- a trained checkpoint loads into either mode
        self.lon_cyclic = bool(lon_cyclic)
        self._engines = {}

    def _engine(self, device) -> SeqEngine:
        key = (str(device), dtype_code(self.compute_dtype), self.lon_cyclic)
        if key not in self._engines:
            cfgs = [LayerCfg(c.input_channels, c.hidden_channels, c.kernel_size) for c in self.layers]
            self._engines[key] = SeqEngine(cfgs, self.compute_dtype, device, lon_cyclic=self.lon_cyclic)
        return self._engines[key]

    def _pack_weights(self, eng: SeqEngine):
        """the layers' current weights and biases into the engine's packed images (one launch): what the trainer and the
        inference loops, which drive the engine themselves, do before a forward pass"""
        eng.pack_weights([c.conv.weight for c in self.layers], [c.conv.bias for c in self.layers])

    def forward(self, x, state=None, *, return_state=False, free_from=None, feedback_grad=False, free_mask=None, input_noise=None,
                feedback_noise=None):
        """x: (batch_size, sequence_length, channels, height, width)  (model.py:254).

        ``state``: None (zeros, model.py:259-262), a list of ``num_layers`` ``(h, c)`` tensor pairs (B, Ch_l, H, W) -- the
        reference's ``hidden_states`` -- or a ``ConvLSTMState``.  ``return_state``: False = the return values of the
        reference; True = the list of ``(h_T, c_T)`` tensor pairs follows ``pred`` (and ``seq``); "device" = a
        ``ConvLSTMState`` follows instead, left on the device in slab form (no NCHW round trip).

        Tensor states are differentiable both ways: a state that requires grad receives dL/dh0, dL/dc0, and the returned
        tensors carry gradients back into the window, so two chained calls are full BPTT across the boundary.  A
        ``ConvLSTMState`` in or out is DETACHED: chaining calls through it is truncated BPTT.  ``net(x)`` alone takes the
        path it always took.

        ``free_from = s`` (a ``feedback=True`` module only): CLOSED LOOP from step s -- at every step t >= s the last
        ``out_channels`` input channels are replaced, on the device, by the head of the top layer's hidden state after step
        t-1, rounded to the storage type; steps t < s see ``x`` as given (the spin-up).  ``free_from >= T`` feeds nothing
        back; ``free_from = 0`` needs a ``state``.  Forward only: with anything that requires grad under grad mode and
        ``free_from < T`` the call raises -- unless ``feedback_grad=True``.

        ``feedback_grad=True`` (with ``free_from = s >= 1``): ROLL-OUT TRAINING -- the call is differentiable
        through the fed-back prediction, the rounding of the fed value taken straight-through.  The forward pass is the same
        one; the backward pass runs time-major with one extra launch per fed step.  The gradient of ``x`` is zero on the
        fed channels of the fed steps.  ``free_from = 0`` under grad stays refused (the first fed value comes from the
        initial state); with ``free_from >= T`` the flag changes nothing.

        ``free_mask = M`` (in the place of ``free_from``; the two are exclusive): SCHEDULED SAMPLING -- a
        bool / uint8 tensor or array of shape (B, T); image b runs step t on its own last prediction where ``M[b, t]`` is set
        and on ``x`` where it is not.  ``M[b, t] = (t >= s)`` is ``free_from = s`` bit for bit; an all-zero mask is the open
        loop.  What ``free_from`` refuses is refused here by the first column that feeds anything: column 0 set needs a
        ``state`` and is forward only; under grad the call needs ``feedback_grad=True``.  The gradient of ``x`` is zero on the
        fed channels of the fed (b, t) only.  At most 64 images per call.

        A ``residual=True`` module honours all of it with p_t = x_t[feedback channels] + head(h_t): ``pred``,
        ``seq`` and the fed value are that p; the gradient of ``x`` gains the cotangent of p_t on the feedback channels of
        every step that saw ``x`` (zero on the fed ones, as above).  ``free_from = 0`` and a mask with column 0 set are
        refused, state or not: the value fed at step 0 would be the prediction of a step before the window, which has no
        input to be added to.

        ``input_noise = InputNoise(std, channels=None, seed, draw, step0, lane0)``: seeded Gaussian noise is
        added, on the device, to channels ``[c0, c0 + n)`` of the input the model is shown (None: the feedback channels),
        rounded to the storage type.  The noise is a constant: the gradient of ``x`` is what it was, the rounding taken
        straight-through.  Everything above composes with it: a fed step overwrites its fed channels afterwards, an unfed
        step of a ``residual=True`` module takes the NOISY stored value as its base.  None, or an all-zero ``std``: no launch,
        the bits of the call without it.

        ``feedback_noise = InputNoise(std, seed=, draw=, step0=, lane0=)`` (``channels`` must be None: the
        feedback channels): the value every fed step stores becomes round(p + std[o] * z), z the normal of ``input_noise``'s
        rule for (pixel, output o, step0 + t, lane0 + b) -- an ensemble member's perturbation of the free run.  ``std``: one
        float or out_channels floats.  Forward only: refused together with ``feedback_grad=True``, and on a module without
        ``feedback=True``.  None, an all-zero ``std`` or a call that feeds nothing: the launches and bits of the call without it."""
        noise = self._check_noise(x, input_noise)
        fnoise = self._check_feedback_noise(feedback_noise, feedback_grad)
        if free_mask is not None:                       # the refusals of free_from, by the first column with a fed image
            if free_from is not None:
                raise ValueError("free_mask and free_from are exclusive: the mask says for every step what free_from says for all")
            if not self.feedback:
                raise ValueError("free_mask needs a ConvLSTM built with feedback=True")
            if len(x.shape) != 5:
                raise ValueError(f"ConvLSTM: x must be (B, T, C, H, W), got {tuple(x.shape)}")
            mask = Feedback.mask_bt(free_mask, x.shape[0], x.shape[1])
            first = Feedback.first_fed(mask)
            if first == 0 and self.residual:
                raise ValueError(RESIDUAL_STEP0)
            if first == 0 and state is None:
                raise ValueError("free_mask with column 0 set feeds step 0 from the head of the initial state: pass a state")
            if first < x.shape[1] and not (feedback_grad and first >= 1) and self._wants_grad(x, state):
                raise RuntimeError(_NO_FEEDBACK_GRAD)
            if first < x.shape[1] and x.shape[0] > 64:
                raise ValueError(f"free_mask: a feed mask holds at most 64 images per call, got B = {x.shape[0]}")
            free_from = mask if first < x.shape[1] else None         # (nothing fed: the open loop, the call it always was)
            feedback_grad = feedback_grad and free_from is not None
            return self._forward(x, state, return_state, free_from, feedback_grad, noise, fnoise if free_from is not None else None)
        if free_from is not None:                       # every refusal here, before anything is launched (or any device is asked for)
            if not self.feedback:
                raise ValueError("free_from needs a ConvLSTM built with feedback=True")
            if isinstance(free_from, bool) or int(free_from) != free_from or free_from < 0:
                raise ValueError(f"free_from must be a step index >= 0, got {free_from!r}")
            free_from = int(free_from)
            if len(x.shape) != 5:
                raise ValueError(f"ConvLSTM: x must be (B, T, C, H, W), got {tuple(x.shape)}")
            if free_from == 0 and self.residual:
                raise ValueError(RESIDUAL_STEP0)
            if free_from == 0 and state is None:
                raise ValueError("free_from=0 feeds step 0 from the head of the initial state: pass a state")
            if free_from < x.shape[1] and not (feedback_grad and free_from >= 1) and self._wants_grad(x, state):
                raise RuntimeError(_NO_FEEDBACK_GRAD)
        # (a call that feeds nothing has no value to put the noise on: the call without the argument)
        return self._forward(x, state, return_state, free_from, feedback_grad, noise, fnoise if free_from is not None else None)

    def _check_feedback_noise(self, feedback_noise, feedback_grad):
        """the refusals of ``feedback_noise``, before anything is launched; an InputNoise with out_channels sigmas, or None"""
        if feedback_noise is None:
            return None
        if not isinstance(feedback_noise, InputNoise):
            raise ValueError(f"feedback_noise must be an InputNoise or None, got {type(feedback_noise).__name__}")
        if not self.feedback:
            raise ValueError("feedback_noise needs a ConvLSTM built with feedback=True")
        if feedback_noise.channels is not None:
            raise ValueError("feedback_noise: channels must be None -- the noise goes onto the fed-back value, the feedback channels")
        if feedback_grad:
            raise ValueError("feedback_noise is forward only: it is refused together with feedback_grad=True (roll-out training "
                             "through the stochastic feedback is not built)")
        O = self.conv.out_channels
        _, _, sig = feedback_noise.span(O, O)                      # one std for all, or one per output
        if not feedback_noise.active:
            return None
        return InputNoise(sig, None, feedback_noise.seed, feedback_noise.draw, feedback_noise.step0, feedback_noise.lane0)

    def _check_noise(self, x, input_noise):
        """the refusals of ``input_noise``, before anything is launched; the InputNoise the engine takes (span resolved), or None"""
        if input_noise is None:
            return None
        if not isinstance(input_noise, InputNoise):
            raise ValueError(f"input_noise must be an InputNoise or None, got {type(input_noise).__name__}")
        if len(x.shape) != 5:
            raise ValueError(f"ConvLSTM: x must be (B, T, C, H, W), got {tuple(x.shape)}")
        c0, n, _ = input_noise.span(self.layers[0].input_channels, self.conv.out_channels if self.feedback else None)
        if not input_noise.active:
            return None
        return InputNoise(input_noise.std, (c0, n), input_noise.seed, input_noise.draw, input_noise.step0, input_noise.lane0)

    def _wants_grad(self, x, state) -> bool:
        """grad mode is on and an input, a parameter or a tensor state requires grad"""
        return torch.is_grad_enabled() and (
            x.requires_grad or any(p.requires_grad for p in self.parameters())
            or (state is not None and not isinstance(state, ConvLSTMState) and any(t.requires_grad for pair in state for t in pair)))

    def _forward(self, x, state, return_state, free_from, feedback_grad, noise=None, fnoise=None):
        """forward() behind its refusals; ``free_from``: None, a step index or a (B, T) uint8 feed mask; ``noise``: None or an
        InputNoise with its span resolved"""
        _require_cuda(x, "ConvLSTM")
        wb = []
        for cell in self.layers:
            wb += [cell.conv.weight, cell.conv.bias]
        st = []
        if state is None and not return_state:          # the default call: nothing to validate, and its own head-backward rule
            opts = _CallOpts(seq_always=self.return_sequence, free_from=free_from, feedback_grad=bool(feedback_grad),
                             residual=self.residual, noise=noise, fnoise=fnoise)
        else:
            if return_state not in (False, True, "device"):
                raise ValueError(f"return_state must be False, True or 'device', got {return_state!r}")
            if len(x.shape) != 5:
                raise ValueError(f"ConvLSTM: x must be (B, T, C, H, W), got {tuple(x.shape)}")
            eng = self._engine(x.device)
            B, _, _, H, W = x.shape
            if isinstance(state, ConvLSTMState):        # every mismatch is a ValueError here, before anything is launched
                eng.check_state(state, B, H, W)
            elif state is not None:
                hs, cs = eng._state_tensors(state, (B, H, W))
                st = _interleave(hs, cs)
            opts = _CallOpts(state if isinstance(state, ConvLSTMState) else None, return_state, free_from=free_from,
                             feedback_grad=bool(feedback_grad), residual=self.residual, noise=noise, fnoise=fnoise)
        out = _ConvLSTMFn.apply(self, torch.is_grad_enabled(), opts, x, self.conv.weight, self.conv.bias, *wb, *st)
        out = list(out) if isinstance(out, tuple) else [out]
        n0 = 2 if self.return_sequence else 1
        res = out[:n0]
        if return_state == "device":
            res.append(opts.state_out)
        elif return_state:
            res.append([(out[n0 + 2 * l], out[n0 + 2 * l + 1]) for l in range(self.num_layers)])
        return tuple(res) if len(res) > 1 else res[0]
