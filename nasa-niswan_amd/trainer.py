"""One batch of the reference fit loop (train.py:92-114) as a fixed sequence of HIP launches.

    X.cuda(), y.cuda()                      -> inputs already on device
    pred = generator(X)                     -> nint_pack_btchw + the forward pass (SeqEngine._seq_pass) + nint_head_fwd
    pred[:, :, 5:95, 5:149].squeeze()       -> crop folded into the loss kernel (index math)
    MSELoss(y,pred) + L1Loss(y,pred)        -> nint_loss_mse_l1_crop (also emits d loss/d pred); with ``loss_weights`` the
                                               per-cell weighted means of loss.py (the _weighted entries); with ``loss``
                                               (a loss.LossSpec) the MSE / L1 / Huber mix with output and step weights
                                               (the _spec entries)
    zero_grad; loss.backward()              -> nint_head_bwd + the backward pass (grads overwrite the bucket)
    [DDP]                                   -> ONE RCCL all-reduce of the flat gradient bucket
    [stateful]                              -> nint_state_copy before the forward pass (carried state -> slot 0) and after it
                                               (slot T -> carried state): truncated BPTT over consecutive chunks of a record;
                                               with ``skip_nonfinite`` a lane whose saved state is non-finite is zeroed
                                               (torch ops on the state buffers, on the device)
    optimizer.step()                        -> nint_adam_flat (1/world folded in); with ``max_grad_norm`` / ``skip_nonfinite``
                                               nint_adam_flat_guarded: norm, clipping and the skip decided on the device
    loss.item(); r2_score(...cpu())         -> device-side accumulators, read once per epoch
    [bptt_segments = n]                     -> the window runs as n segments of S = T/n steps through ONE S-step training
                                               workspace: a forward sweep that keeps the state at every segment start, then
                                               per segment, last to first, recompute + the backward pass with accumulate = 1 -- the
                                               full-window gradient at 1/n of the resident slabs
    [freeze_layers = f]                     -> fine-tuning: the first f ConvLSTM layers are frozen.  nint_seq.train_from = f: BPTT
                                               stops above layer f-1, a frozen layer keeps no stash and no gradient slabs, the
                                               exchange and the norm run over the trained tail of the bucket, and the optimizer
                                               is AdamW over per-layer groups (nint_adam_flat_groups: ``weight_decay``,
                                               ``layer_lr_scale``).  f = L trains the head alone: no BPTT
    [rollout_from = s]                      -> ROLL-OUT TRAINING: the closed-loop forward from step s,
                                               the same fused head / loss pass with its dpred in the roll-out slab, BPTT through
                                               the fed-back prediction (the roll-out entry), then the head's gradients from
                                               the slab (nint_head_bwd_acc over all T*B images)
    [rollout_from = s, sampling_prob = p]   -> SCHEDULED SAMPLING: per step t >= s and per image a coin of
                                               bias p decides whether the image sees its own last prediction; the same step
                                               under that feed mask (the _sampled entries).  p = 1: the line above, call for call
    [ConvLSTM(residual=True)]               -> RESIDUAL HEAD: every head / loss pass adds the feedback channels of the
                                               step's own input to the head's output (the _res entries); with rollout_from the
                                               closed loop and its backward are the _residual entries.  Every other option
                                               composes: the base of a step is that step's input, so no segment, chunk or
                                               micro-batch boundary is crossed
    [input_noise = sigma]                   -> INPUT NOISE: one nint_input_noise launch behind every filling of an
                                               input slab of step() -- seeded Gaussian noise on the tracer channels, keyed by
                                               (noise_seed, the count of step() calls, rank * B + b, the step's place in the
                                               window), so the sweep and the recompute of a segment see the same input
    [rollout_from = s, ensemble_members = M]-> ENSEMBLE TRAINING: the B lanes are N samples x M members (lane
                                               n*M + m); the closed loop runs with seeded noise on every fed-back value
                                               (nint_seq_fwd_stochastic, training stash on), nint_head_fwd_seq materialises
                                               the members' predictions, nint_ens_loss forms the almost-fair CRPS over the
                                               member lanes and writes every member's d loss / d pred into the roll-out slab,
                                               and the roll-out backward runs as it stands (the noise is a constant)
    [accumulate_steps = k]                  -> k micro-batches add into the bucket (accumulate = 1 from the second on); the
                                               all-reduce and ONE Adam launch with grad_scale = 1/(k world) on the k-th

No autograd graph, no per-kernel Python, no host synchronisation inside the step."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import NINT_LOSS_SPEC_SCRATCH_FLOATS, NINT_LOSS_STATS
from .engine import InputNoise
from .model import ConvLSTM
from .loss import DeviceWeights, EnsembleLoss, LossSpec, crop_loss_launch
from .optim import FlatParams, FusedAdam


def segment_plan(T: int, n: int) -> List[Tuple[int, int]]:
    """The segments of checkpointed BPTT: [(t0, S)] for a window of T steps in n equal segments of S = T / n steps, in time
    order.  ValueError when n < 1 or n does not divide T (one workspace shape serves every segment).  Pure."""
    T, n = int(T), int(n)
    if n < 1:
        raise ValueError(f"bptt_segments must be >= 1, got {n}")
    if T < 1 or T % n:
        raise ValueError(f"bptt_segments = {n} does not divide the window of T = {T} steps (equal segments only)")
    S = T // n
    return [(j * S, S) for j in range(n)]


class FusedTrainer:
    def __init__(self, model: ConvLSTM, lr: float = 1e-3, betas=(0.5, 0.999), eps: float = 1e-8,
                 halo: Tuple[int, int] = (5, 5), process_group=None, distributed: Optional[bool] = None,
                 overlap_allreduce: bool = False, sequence_loss: bool = False, loss_weights=None,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, stateful: bool = False,
                 bptt_segments: Optional[int] = None, accumulate_steps: int = 1, loss: Optional[LossSpec] = None,
                 freeze_layers: int = 0, weight_decay: float = 0.0, layer_lr_scale=None, rollout_from: Optional[int] = None,
                 sampling_prob: Optional[float] = None, sampling_seed: int = 0, input_noise=None, noise_channels=None,
                 noise_seed: int = 0, ensemble_members: Optional[int] = None, feedback_noise=None,
                 ensemble_loss: Optional[EnsembleLoss] = None):
        # Input noise: every step() shows the model its input with N(0, input_noise^2) added to the noise
        # channels (None: the feedback channels), drawn on the device.  `draw` is the count of step() calls (micro-batches
        # included), `lane0` = rank * B with the SAME seed on every rank, `step0` a segment's start in its window.  evaluate()
        # and forward_loss() never add noise.  Checked first: these refusals need no device.
        self._noise_channels, self.noise_seed = noise_channels, noise_seed
        self._noise_model = (model.layers[0].input_channels, model.conv.weight.shape[0] if getattr(model, "feedback", False) else None)
        self._noise, self._draws = None, 0
        self.set_input_noise(input_noise)
        # Roll-out training: from step `rollout_from` on the window runs on its own prediction and the loss's gradient flows
        # back through it.  Checked first: these refusals need no device.
        if rollout_from is not None:
            if isinstance(rollout_from, bool) or int(rollout_from) != rollout_from or rollout_from < 1:
                raise ValueError(f"rollout_from must be a step index >= 1 (the first fed step; step 0 has no prediction to be fed), "
                                 f"got {rollout_from!r}")
            if not getattr(model, "feedback", False):
                raise ValueError("rollout_from needs a ConvLSTM built with feedback=True")
            for name, on in (("bptt_segments > 1", (bptt_segments or 1) > 1), ("stateful", stateful), ("freeze_layers > 0", freeze_layers),
                             ("overlap_allreduce", overlap_allreduce)):
                if on:
                    raise ValueError(f"rollout_from with {name} is not supported: the roll-out backward runs one whole window from "
                                     "the zero state, through every layer, in one call")
            rollout_from = int(rollout_from)
        self.rollout_from = rollout_from
        # Scheduled sampling: with 0 < p < 1 each step draws a (T, B) feed mask, rows below rollout_from forced
        # to 0.  None or 1: every image is fed from rollout_from on (the roll-out step itself); 0: the teacher-forced step.  The
        # draw comes from a CPU generator seeded sampling_seed + rank, made on the first draw (the rank is known once the process
        # group is): reproducible, and different on every rank.
        if sampling_prob is not None and rollout_from is None:
            raise ValueError("sampling_prob needs rollout_from: the coin is thrown for the steps from rollout_from on")
        self.sampling_prob = None
        self.set_sampling_prob(sampling_prob)
        self.sampling_seed = int(sampling_seed)
        self._sampler, self._last_p = None, None
        self.last_mask = None   # (T, B) bool, CPU: what the last step() fed; None before the first step and without sampling
        # Ensemble training: step() takes B = N * M lanes (lane n*M + m: the caller replicates the indices M
        # times) and y of N samples; the members differ by the seeded noise alone -- on the input (``input_noise``, keyed as
        # ever) and on every fed-back value (``feedback_noise``, the same seed and lanes, draw = 0x80000000 | the call count, so
        # the two never share a key) -- and the loss is the almost-fair CRPS over the member lanes (``ensemble_loss``).  All
        # lanes of a sample live on ONE rank: under data parallelism every rank holds whole ensembles and the bucket is reduced
        # as ever; ens_out is not reduced.  Checked here: these refusals need no device.
        self.ensemble_members, self._fb_noise, self._ens_spec = None, None, None
        if ensemble_members is None:
            if feedback_noise is not None or ensemble_loss is not None:
                raise ValueError("feedback_noise / ensemble_loss need ensemble_members: they belong to the ensemble training step")
        else:
            if rollout_from is None:
                raise ValueError("ensemble_members needs rollout_from: the members differ through the closed loop")
            if isinstance(ensemble_members, bool) or int(ensemble_members) != ensemble_members or not 2 <= ensemble_members <= _lib.NINT_ENS_MAX_M:
                raise ValueError(f"ensemble_members must be an integer in [2, {_lib.NINT_ENS_MAX_M}], got {ensemble_members!r}")
            if loss is not None:
                raise ValueError("ensemble_members trains the CRPS (ensemble_loss=EnsembleLoss(...)): a LossSpec (loss=) is refused with it")
            if sampling_prob is not None:
                raise ValueError("ensemble_members with sampling_prob is not supported: scheduled sampling over member lanes is not built")
            if ensemble_loss is not None and not isinstance(ensemble_loss, EnsembleLoss):
                raise TypeError("ensemble_loss must be a loss.EnsembleLoss or None")
            self._ens_spec = ensemble_loss if ensemble_loss is not None else EnsembleLoss()
            if self._ens_spec.step_weights is not None and not sequence_loss:
                raise ValueError("step_weights need FusedTrainer(sequence_loss=True): the last-step loss has one step")
            self.ensemble_members = int(ensemble_members)
            self.set_feedback_noise(feedback_noise)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise _lib.NintError("FusedTrainer needs the model on the MI355X (cuda)")
        # Checkpointed BPTT: step() runs its window as `bptt_segments` equal segments through one training workspace of
        # T / bptt_segments steps (the full-window gradient; None or 1: the whole window resident, today's path)
        if bptt_segments is not None:
            bptt_segments = int(bptt_segments)
            segment_plan(bptt_segments, bptt_segments)           # (n >= 1)
            if bptt_segments > 1 and sequence_loss:
                raise ValueError("bptt_segments with sequence_loss is not supported: the sequence loss's normaliser and per-call "
                                 "statistics are per window, not per segment")
            if bptt_segments > 1 and overlap_allreduce:
                raise ValueError("bptt_segments with overlap_allreduce is not supported: layer 0's slice of the bucket is final "
                                 "only after the first segment's backward, so there is nothing to overlap the exchange with")
        self.bptt_segments = bptt_segments
        # Fine-tuning: the first `freeze_layers` ConvLSTM layers keep their weights (requires_grad False, in no optimizer group);
        # every backward pass of the step starts BPTT's reach at that layer (nint_seq.train_from)
        self.freeze_layers = int(freeze_layers)
        if not 0 <= self.freeze_layers <= model.num_layers:
            raise ValueError(f"freeze_layers must be in [0, {model.num_layers}], got {freeze_layers}")
        if self.freeze_layers > 0 and overlap_allreduce:
            raise ValueError("freeze_layers with overlap_allreduce is not supported: the two-piece exchange runs under layer 0's "
                             "weight gradient, which a frozen layer 0 does not have")
        # Gradient accumulation: the optimizer steps once per `accumulate_steps` calls of step(), on the sum of their buckets
        # scaled by 1 / (accumulate_steps * world): the mean gradient of the group
        self.accumulate_steps = int(accumulate_steps)
        if self.accumulate_steps < 1:
            raise ValueError(f"accumulate_steps must be >= 1, got {accumulate_steps}")
        self._micro = 0         # calls of step() since the last optimizer step
        self._zero = None       # segments: the zero state a stateless window starts from
        self.model = model
        self.device = dev
        self.flat = FlatParams(model)
        # Gradient-norm clipping and dropping of non-finite steps (optim.FusedAdam): the norm is taken of the bucket the optimizer
        # steps on -- under data parallelism the all-reduced sum with grad_scale = 1/world, so every rank takes the same decision
        # from the same bits and nothing more is exchanged
        self.optimizer = FusedAdam(self.flat, lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm,
                                   skip_nonfinite=skip_nonfinite, weight_decay=weight_decay, freeze_layers=self.freeze_layers,
                                   layer_lr_scale=layer_lr_scale)
        self.halo = tuple(halo)
        self.lib = _lib.load()
        # (the size the _spec entries ask for, five doubles per workgroup; the other entries use the first 8194 floats of it)
        self.scratch = torch.zeros(NINT_LOSS_SPEC_SCRATCH_FLOATS, dtype=torch.float32, device=dev)
        # [0..4] pooled: sum d^2, sum |d|, sum y, sum y^2, n; [5..7] per call: sum loss, sum r2_score, calls
        self.stats = torch.zeros(NINT_LOSS_STATS, dtype=torch.float64, device=dev)
        self._dpred = None
        # ensemble training: nint_ens_loss's four sums (SA, SD, SV, cnt), accumulated like `stats`, and its scratch
        self.ens_out = torch.zeros(_lib.NINT_ENS_LOSS_OUT, dtype=torch.float64, device=dev) if self.ensemble_members else None
        self._ens_scratch = None
        self._probe = (None, 0)
        self._marks = None      # diagnostic: a list that step() fills with HIP events (start, after forward, after head/loss, after BPTT, end)
        import torch.distributed as dist
        self.dist = dist
        self.pg = process_group
        if distributed is None:
            distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1
        self.world = dist.get_world_size(process_group) if distributed else 1
        self.distributed = bool(distributed)      # True also for a 1-rank group (exercises the collective path)
        # Data-parallel exchange in two pieces (worth it for the strong-scaling shapes, where the step is ~1.5 ms and
        # the one all-reduce at its end ~5 % of it): the bucket without layer 0's slice is reduced UNDER layer 0's weight gradient
        # (nint_seq.bwd_parts), layer 0's slice after it.  Two all-reduces of disjoint slices: the same sums.
        self.overlap_allreduce = bool(overlap_allreduce)
        # Sequence-to-sequence supervision: y is (B, T, [O,] Hc, Wc), a target at every step of the window, and the loss is
        # MSE + L1 over the per-step head outputs (model.py:264,272,274 commented code) instead of the last one alone
        self.sequence_loss = bool(sequence_loss)
        # Per-cell loss weights (loss.py): an (Hc, Wc) map or (Hc,) row weights -- cos latitude, a mask, their product -- used by
        # step, evaluate and forward_loss in every branch.  Every data-parallel rank must be given the same map.
        self.set_loss_weights(loss_weights)
        # The configurable loss (loss.LossSpec): an MSE / L1 / Huber mix with a weight per output and, with sequence_loss, per
        # step, used by step, evaluate and forward_loss in every branch, on top of the map.  None: the reference's MSE + L1
        # through today's entries.  Not broadcast: every data-parallel rank must be given the same spec.
        self.set_loss(loss)
        # Truncated BPTT over consecutive chunks of a record (dataset.stateful_schedule): step() starts from the state the
        # previous step() ended in, carried on the device in slab form (engine.ConvLSTMState), and gradients stop at the
        # chunk start.  evaluate / forward_loss keep zero-state windows; under data parallelism every rank carries its own.
        self.stateful = bool(stateful)
        self.state = None
        L = model.num_layers
        self._dW = [self.flat.grad_view(2 * l) for l in range(L)]
        self._db = [self.flat.grad_view(2 * l + 1) for l in range(L)]
        self._dw_head = self.flat.grad_view(2 * L)
        self._db_head = self.flat.grad_view(2 * L + 1)
        if self.distributed:
            # identical initial weights on every rank (the reference seeds identically, utils.py:77-88)
            dist.broadcast(self.flat.data, src=0, group=process_group)

    def set_probe(self, buf: Optional[torch.Tensor], mask: int = 0):
        """In-step timing probes (nint_seq.probe, include/nint.h): `buf` = int64/uint64 device tensor of 2*slots words that
        the following step() calls fill with {tag, 100 MHz timestamp} pairs around every launch whose kind is in `mask`;
        None switches them off.  Diagnostic: bench.py prices the kernels INSIDE the step with it."""
        if buf is not None and (self.bptt_segments or 1) > 1:
            raise ValueError("set_probe with bptt_segments is not supported: a probe buffer holds the slots of one forward and "
                             "one backward pass, a segmented step runs several of each")
        self._probe = (buf, int(mask) if buf is not None else 0)

    def set_loss_weights(self, weights):
        """Switch the loss weights (between epochs, say): an (Hc, Wc) array or tensor, an (Hc,) vector of row weights, or None
        for the unweighted loss.  Values are validated here (ValueError for a negative, NaN or inf value or an all-zero
        map), the shape against the target's crop at the next step / evaluate.  Not broadcast between ranks."""
        self._weights = None if weights is None else DeviceWeights(weights)

    def _loss_weights(self, Hc: int, Wc: int):
        """(wgt, wsum) for the engine's head/loss calls, or None"""
        return None if self._weights is None else self._weights.on(self.device, Hc, Wc)

    def set_loss(self, spec: Optional[LossSpec]):
        """Switch the loss (between epochs, say): a loss.LossSpec -- coefficients of the MSE, L1 and Huber terms, the Huber
        threshold, output and step weights -- or None for the reference's MSE + L1 through the entries it has always run.
        The values are validated by LossSpec, the lengths of its weights against the model's outputs and the window at the
        next step / evaluate; step weights need ``sequence_loss``.  epoch_stats() then reports the mean of the configured
        loss.  Under data parallelism the spec is NOT broadcast: every rank must be given the same one."""
        if spec is not None and not isinstance(spec, LossSpec):
            raise TypeError("loss must be a loss.LossSpec or None")
        if spec is not None and spec.step_weights is not None and not self.sequence_loss:
            raise ValueError("step_weights need FusedTrainer(sequence_loss=True): the last-step loss has one step")
        self._spec = spec

    def _loss_spec(self, O: int, T: int):
        """the nint_loss_spec of this call (its weight vector over t*O + o with sequence_loss, over o without), or None"""
        return None if self._spec is None else self._spec.on(self.device, O, T if self.sequence_loss else None)

    def _loss(self, pred, yv, dpred, N, O, H, W, Hc, Wc, wts, spec=None):
        """the stand-alone loss launch of the three-launch paths"""
        crop_loss_launch(pred, yv, dpred, self.scratch, self.stats, N, O, H, W, self.halo[0], self.halo[1], Hc, Wc, wts, spec)

    # ------------------------------------------------------------------ pieces
    def _call_facts(self, X, y):
        """What step() and forward_loss() know of a call before anything is acquired: the loss weights and spec (validated
        against the target's crop, the model's outputs and the window), the shapes, and the target as f32 (asserted to hold
        one value per output, cropped cell [and step])."""
        B, T, _, H, W = X.shape
        O, Hc, Wc = self.model.conv.weight.shape[0], y.shape[-2], y.shape[-1]
        wts = self._loss_weights(Hc, Wc)
        spec = self._loss_spec(O, T)
        yv = y.detach().float().contiguous()
        sq = self.sequence_loss
        assert yv.numel() == B * (T if sq else 1) * O * Hc * Wc, "target must be (B,T,[O,]Hc,Wc)" if sq else "target must be (B,[O,]Hc,Wc)"
        return wts, spec, B, T, H, W, O, Hc, Wc, yv

    def _head_loss_unfused(self, eng, ws, yv, dpred, B, T, O, H, W, Hc, Wc, wts, spec):
        """The three-launch path's first two: the head's output -- of every step with sequence_loss, (B, T*O, H, W), which
        the loss kernel's own index math takes as O' = T*O outputs -- and the stand-alone loss launch on it."""
        m = self.model
        if self.sequence_loss:
            out, O = eng.head_forward_seq(ws, m.conv.weight, m.conv.bias), T * O
        else:
            out = eng.head_forward(ws, m.conv.weight, m.conv.bias)
        self._loss(out, yv, dpred, B, O, H, W, Hc, Wc, wts, spec)
        return out

    def forward_loss(self, X: torch.Tensor, y: torch.Tensor, train: bool = True):
        m = self.model
        eng = m._engine(self.device)
        wts, spec, B, T, H, W, O, Hc, Wc, yv = self._call_facts(X, y)
        ws = eng.acquire(B, T, H, W, train, False)          # (handed to the caller still acquired: no `with eng.window`)
        m._pack_weights(eng)
        eng.forward(ws, X, **self._res_kw())
        dpred = None
        if train:
            shape = (B, T * O if self.sequence_loss else O, H, W)
            if self._dpred is None or self._dpred.shape != shape:
                self._dpred = torch.empty(shape, dtype=torch.float32, device=self.device)
            dpred = self._dpred
        pred = self._head_loss_unfused(eng, ws, yv, dpred, B, T, O, H, W, Hc, Wc, wts, spec)
        return eng, ws, pred, dpred

    def _res_kw(self) -> dict:
        """the ``residual`` argument of every forward pass of a residual-head model, nothing otherwise: the
        calls of any other model are, argument for argument, what they were.  The base of step t is the input of step t itself,
        so segments (bptt_segments) and carried state (stateful) need nothing more: no base crosses a boundary."""
        return dict(residual=self.model.conv.weight.shape[0]) if getattr(self.model, "residual", False) else {}

    def reset_state(self):
        """stateful: the next step() starts every lane from the zero state (a new epoch, a new record)"""
        self.state = None

    @staticmethod
    def _state_for(st, eng, B, H, W):
        """`st` if it is a state of this engine and (B, H, W), else a new zero state"""
        if st is None or st.eng is not eng or (st.B, st.H, st.W) != (B, H, W):
            return eng.new_state(B, H, W)
        return st

    def _carried_state(self, eng, B, H, W, reset):
        """the trainer's state for this step: zeros on first use or when the batch shape changed, lanes in `reset` zeroed"""
        old = None if reset is True else self.state
        st = self.state = self._state_for(old, eng, B, H, W)
        if st is old and reset is not None and reset is not False:
            st.reset(reset)
        return st

    def _drop_nonfinite_lanes(self, st):
        """stateful with skip_nonfinite: a lane whose state just saved holds a NaN or inf in any layer's h or c starts the next
        chunk from the zero state, the other lanes keep their bytes.  Without this the one bad chunk whose
        optimizer step the guard drops would poison the lane, and with it every later step, until reset_state().  Decided on
        the device, no host read; a fill, not a product with a mask (NaN * 0 is NaN)."""
        if not self.optimizer.skip_nonfinite:
            return
        et = torch.bfloat16 if st.dtype == "bf16" else torch.float32
        views = [h.view(et).view(st.B, -1) for h in st.h] + [c.view(st.B, -1) for c in st.c]
        bad = None
        for v in views:
            b = ~torch.isfinite(v).all(dim=1, keepdim=True)
            bad = b if bad is None else bad | b
        for v in views:
            v.masked_fill_(bad, 0)

    def set_input_noise(self, std):
        """the noise level of the steps to come (a curriculum sets it once per epoch): a float or one per noise channel, in the
        units of the stored input; None or 0: no noise, the step it was.  ValueError for a negative or non-finite value, for a
        span outside the input's channels, or -- without ``noise_channels`` -- a model built without feedback=True."""
        if std is None:
            self._noise = None
            return
        nz = InputNoise(std, self._noise_channels, self.noise_seed)
        c0, n, _ = nz.span(*self._noise_model)
        self._noise = InputNoise(nz.std, (c0, n), nz.seed) if nz.active else None

    def _noise_kw(self, draw: int, B: int, step0: int = 0) -> dict:
        """the ``noise`` argument of a forward pass of step(), nothing without noise: the calls are then, argument for argument,
        what they were.  ``draw``: this step()'s number; ``step0``: where the pass's first step lies in the window."""
        if self._noise is None:
            return {}
        rank = self.dist.get_rank(self.pg) if self.distributed else 0
        return dict(noise=InputNoise(self._noise.std, self._noise.channels, self._noise.seed, draw, step0, rank * B))

    def set_feedback_noise(self, std):
        """ensemble training: the noise level on the fed-back value for the steps to come (a curriculum sets it beside
        set_input_noise): a float or one per output, in the units of the stored input.  ValueError without
        ``ensemble_members``, for a negative or non-finite value, and where it leaves both noises zero -- identical members
        make the pair term of the CRPS vanish."""
        if self.ensemble_members is None:
            raise ValueError("set_feedback_noise needs FusedTrainer(ensemble_members=M)")
        nz = None if std is None else InputNoise(std, None, self.noise_seed)
        if nz is not None:
            nz.span(self._noise_model[1] or 0, self._noise_model[1])       # (one value or O values)
        if (nz is None or not nz.active) and self._noise is None:
            raise ValueError("ensemble_members needs noise: input_noise and feedback_noise are both zero, so the members would "
                             "be identical and the CRPS's pair term would vanish")
        self._fb_noise = nz if nz is not None and nz.active else None

    def _fb_noise_kw(self, draw: int, B: int) -> dict:
        """the ``feedback_noise`` argument of the ensemble step's forward pass: the input noise's seed and lanes, and a draw
        with the top bit set, so that no (seed, draw) key is shared with the input noise of any step"""
        if self._fb_noise is None:
            return {}
        rank = self.dist.get_rank(self.pg) if self.distributed else 0
        return dict(feedback_noise=InputNoise(self._fb_noise.std, None, self._fb_noise.seed, 0x80000000 | (draw & 0x7fffffff), 0, rank * B))

    def set_sampling_prob(self, p: Optional[float]):
        """the coin's bias for the steps to come (a curriculum sets it once per epoch); None: no sampling"""
        if p is not None:
            if self.rollout_from is None:
                raise ValueError("sampling_prob needs rollout_from: the coin is thrown for the steps from rollout_from on")
            if isinstance(p, bool) or not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"sampling_prob must be a probability in [0, 1], got {p!r}")
            p = float(p)
        self.sampling_prob = p

    @staticmethod
    def draw_mask(gen: torch.Generator, T: int, B: int, rollout_from: int, p: float) -> torch.Tensor:
        """one step's feed mask, (T, B) bool on the CPU: rand((T, B)) < p, rows t < rollout_from forced to 0.  Pure."""
        m = torch.rand((T, B), generator=gen) < p
        m[:rollout_from] = False
        return m

    @staticmethod
    def sampler(seed: int, rank: int) -> torch.Generator:
        """the CPU generator of a rank's draws"""
        return torch.Generator(device="cpu").manual_seed(int(seed) + int(rank))

    def _draw(self, T: int, B: int):
        """the feed argument of this step's forward pass: None (nothing fed: the teacher-forced step), rollout_from (every image
        fed from there on: the roll-out step) or a (B, T) mask"""
        s = self.rollout_from
        if s is None or not range(min(s, T), T):
            return None
        if self.sampling_prob is None:
            return s
        if self.sampling_prob >= 1.0 or self.sampling_prob <= 0.0:
            # no coin to throw (rand is in [0, 1): < 1 always, < 0 never), and no generator state spent: the roll-out step or the
            # teacher-forced step, call for call.  The mask is still shown.
            if self.last_mask is None or tuple(self.last_mask.shape) != (T, B) or self._last_p != self.sampling_prob:
                self.last_mask = (torch.arange(T) >= (s if self.sampling_prob >= 1.0 else T)).view(T, 1).expand(T, B).clone()
                self._last_p = self.sampling_prob
            return s if self.sampling_prob >= 1.0 else None
        self._last_p = None
        if self._sampler is None:
            rank = self.dist.get_rank(self.pg) if self.distributed else 0
            self._sampler = self.sampler(self.sampling_seed, rank)
        self.last_mask = self.draw_mask(self._sampler, T, B, s, self.sampling_prob)
        if bool(self.last_mask[s:].all()):          # (p = 1: every image fed from s on -- the roll-out step, call for call)
            return s
        return self.last_mask.t().contiguous() if bool(self.last_mask.any()) else None

    def _head_pass(self, eng, ws, yv, B, T, O, H, W, Hc, Wc, wts, acc: bool, spec=None, slab=None):
        """head forward + crop + loss + d loss / d pred + dL/dh + the head's weight gradient on the workspace's last h (every
        h with sequence_loss); `acc`: the head's gradients are added to the bucket (a later micro-batch of a group).
        `slab` (a roll-out window's): the fused pass writes d loss / d pred there (zeros where the loss has no term) and W^T of it
        into the dh_seq blocks the roll-out starts from; the head's weight gradient waits for the slab to come back (_bptt)."""
        m, sq = self.model, self.sequence_loss
        if slab is not None:
            dpred = slab if sq else slab[(T - 1) * B:]
            if not sq:
                slab[:(T - 1) * B].zero_()
        else:
            if self._dpred is None or self._dpred.numel() != B * (T if sq else 1) * O * H * W:
                self._dpred = torch.empty(B * (T if sq else 1), O, H, W, dtype=torch.float32, device=self.device)
            dpred = self._dpred
        hk = dict(dw_out=self._dw_head, db_out=self._db_head, accumulate=acc)
        sk = {} if spec is None else dict(spec=spec)             # (None: today's calls, argument for argument)
        # one pass: loss, d loss / d pred and dL/dh of the last step (the prediction itself is never materialised) or of every
        # step (image order t*B + b, which the head's weight-gradient kernels reduce as T*B images; BPTT adds dL/dh at each t)
        fused = (eng.head_loss_seq_fused if sq else eng.head_loss_fused)(ws, m.conv.weight, m.conv.bias, yv, dpred, self.scratch,
                                                                         self.stats, self.halo, Hc, Wc, wts, **sk)
        if slab is not None:
            if not fused:   # (a head beyond the fused kernels is beyond the feedback kernel too: the forward pass refuses it first)
                raise _lib.NintError("rollout_from: the head is beyond the fused head / loss kernels, which write the roll-out slab")
            eng.rollout_cotangents(ws, m.conv.weight, slab_filled=True, dh_written=sq)
            return
        if not fused:
            self._head_loss_unfused(eng, ws, yv, dpred, B, T, O, H, W, Hc, Wc, wts, spec)
        if sq and fused:
            eng.head_backward(ws, m.conv.weight, dpred, write_dh=False, images=(B, T * B), **hk)
        elif sq:
            eng.head_backward_seq(ws, m.conv.weight, dpred.view(B, T * O, H, W), None, **hk)
        else:
            eng.head_backward(ws, m.conv.weight, dpred, write_dh=not fused, **hk)

    def _bptt(self, eng, ws, acc: bool, last: bool, slab=None):
        """BPTT of a resident window into the bucket -- as a roll-out (`slab`: through the fed-back prediction, then the head's
        gradients from the slab), in two parts around the exchange, or plain.  Returns (pending, n0) for _finish."""
        m, L = self.model, self.model.num_layers
        bk = dict(zero_state_grads=range(L), dW_out=self._dW, db_out=self._db, seq_grads=self.sequence_loss, accumulate=acc,
                  train_from=self.freeze_layers)
        if slab is not None:
            eng.backward(ws, False, rollout=slab, **bk)
            eng.rollout_head_backward(ws, m.conv.weight, slab, self._dw_head, self._db_head, acc)
        elif last and self.distributed and self.overlap_allreduce and L > 1 and self._probe[0] is None:
            # the bucket without layer 0's slice is exchanged under layer 0's weight gradient; _finish exchanges the slice
            n0 = self.flat.offsets[2]              # layers.0.conv.weight + .bias lead the bucket (module parameter order)
            eng.backward(ws, False, parts=1, **bk)
            pending = self.dist.all_reduce(self.flat.grad[n0:], op=self.dist.ReduceOp.SUM, group=self.pg, async_op=True)
            eng.backward(ws, False, parts=2, **bk)
            return pending, n0
        else:
            eng.backward(ws, False, **bk)
        return None, 0

    def step(self, X: torch.Tensor, y: torch.Tensor, reset=None) -> torch.Tensor:
        """One call of the fit loop; returns the loss as a 0-dim DEVICE tensor (no sync).  X: (B,T,C,Hp,Wp) f32 or a
        dataset.SlabBatch.  y: (B,[O,]Hc,Wc), or (B,T,[O,]Hc,Wc) with ``sequence_loss``.
        ``reset`` (stateful trainers only): True, or one boolean per lane -- those lanes start this chunk from the zero state.
        With ``accumulate_steps = k`` the optimizer steps on every k-th call, on the mean gradient of the k calls."""
        if self.ensemble_members is not None:
            return self._ens_step(X, y, reset)
        m = self.model
        eng = m._engine(self.device)
        wts, spec, B, T, H, W, O, Hc, Wc, yv = self._call_facts(X, y)
        if reset is not None and not self.stateful:
            raise ValueError("step(reset=...) needs FusedTrainer(stateful=True)")
        k = self.accumulate_steps
        acc, last = self._micro > 0, self._micro == k - 1       # add to the bucket; exchange and step after this call
        draw, self._draws = self._draws, self._draws + 1        # (input noise: one draw per call, micro-batches included)
        if (self.bptt_segments or 1) > 1:
            plan = segment_plan(T, self.bptt_segments)          # (before anything is acquired)
        else:
            plan = None
        carried = self._carried_state(eng, B, H, W, reset) if self.stateful else None
        mark = self._mark
        if plan is not None:
            mark()
            m._pack_weights(eng)
            self._segments(eng, X, yv, plan, carried, acc, wts, spec, draw)
            return self._finish(last)
        with eng.window(B, T, H, W, True, self.stateful, self.freeze_layers) as ws:
            pb, pm = self._probe
            ws.seq.probe = pb.data_ptr() if pb is not None else None
            ws.seq.probe_mask, ws.seq.probe_slots = pm, (pb.numel() // 2 if pb is not None else 0)
            mark()
            m._pack_weights(eng)
            if carried is not None:
                eng.load_state(ws, carried)          # carried state -> slot 0
            feed = self._draw(T, B)     # (None: nothing is fed -- the step it was)
            eng.forward(ws, X, **(dict(feedback=(m.conv.weight, m.conv.bias, feed), feedback_grad=True) if feed is not None else {}),
                        **self._res_kw(), **self._noise_kw(draw, B))
            if carried is not None:
                eng.save_state(ws, carried)          # slot T -> carried state; BPTT below stops at the chunk start
                self._drop_nonfinite_lanes(carried)
            mark()
            slab = ws.rollout_dpred(eng, O) if ws.feedback.fed else None
            self._head_pass(eng, ws, yv, B, T, O, H, W, Hc, Wc, wts, acc, spec, slab)
            mark()
            pending, n0 = self._bptt(eng, ws, acc, last, slab)
            mark()
        return self._finish(last, pending, n0)

    def _ens_step(self, X, y, reset=None) -> torch.Tensor:
        """step() of an ensemble trainer.  X carries B = N * M lanes, lane n*M + m (the caller replicates the
        indices, as rollout_ensemble does); y is (N, [T,] [O,] Hc, Wc), never replicated.  One step, no host sync: the noisy
        closed-loop training forward, head_forward_seq, nint_ens_loss into the roll-out slab (the last step alone without
        ``sequence_loss``, the other images zeroed), the cotangents of the unfed steps, the roll-out BPTT and the optimizer.
        All lanes of a sample live on one rank."""
        m, M, sq = self.model, self.ensemble_members, self.sequence_loss
        B, T, _, H, W = X.shape
        O, Hc, Wc = m.conv.weight.shape[0], y.shape[-2], y.shape[-1]
        if B % M:
            raise ValueError(f"ensemble step: {B} lanes do not hold whole ensembles of {M} members (lane n*M + m)")
        N = B // M
        if y.shape[0] != N or y.numel() != N * (T if sq else 1) * O * Hc * Wc:
            raise ValueError(f"ensemble step: the target must be ({N}, {'T, ' if sq else ''}[O,] Hc, Wc) for {B} lanes of {M} members -- "
                             f"one per sample, never replicated -- got {tuple(y.shape)}")
        if reset is not None:
            raise ValueError("step(reset=...) needs FusedTrainer(stateful=True)")
        feed = self._draw(T, B)
        if feed is None:
            raise ValueError(f"ensemble step: rollout_from = {self.rollout_from} lies beyond the window of {T} steps: nothing is fed back")
        eng = m._engine(self.device)
        wts = self._loss_weights(Hc, Wc)
        spec = self._ens_spec.on(self.device, O, T if sq else None)
        yv = y.detach().float().contiguous()
        k = self.accumulate_steps
        acc, last = self._micro > 0, self._micro == k - 1
        draw, self._draws = self._draws, self._draws + 1
        need = eng.ens_loss_scratch(N * (T if sq else 1), M, O, H, W)
        if self._ens_scratch is None or self._ens_scratch.numel() < need:
            self._ens_scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        mark = self._mark
        with eng.window(B, T, H, W, True, False, 0) as ws:
            pb, pm = self._probe
            ws.seq.probe = pb.data_ptr() if pb is not None else None
            ws.seq.probe_mask, ws.seq.probe_slots = pm, (pb.numel() // 2 if pb is not None else 0)
            mark()
            m._pack_weights(eng)
            eng.forward(ws, X, feedback=(m.conv.weight, m.conv.bias, feed), feedback_grad=True, **self._res_kw(),
                        **self._noise_kw(draw, B), **self._fb_noise_kw(draw, B))
            mark()
            slab = ws.rollout_dpred(eng, O)
            seq = eng.head_forward_seq(ws, m.conv.weight, m.conv.bias)
            if not sq:
                slab[:(T - 1) * B].zero_()
            eng.ens_loss(ws, seq, yv, slab, M, spec, wts, self._ens_scratch, self.scratch, self.stats, self.ens_out, self.halo,
                         Hc, Wc, every_step=sq)
            eng.rollout_cotangents(ws, m.conv.weight, slab_filled=True, dh_written=False)
            mark()
            pending, n0 = self._bptt(eng, ws, acc, last, slab)
            mark()
        return self._finish(last, pending, n0)

    def ensemble_stats(self, reset: bool = False) -> dict:
        """One device->host read: from nint_ens_loss's sums since the last reset -- ``crps`` (the mean of the trained score),
        ``rmse_mean`` (of the ensemble mean), ``spread`` (sqrt of the mean unbiased member variance) and ``spread_skill``
        (with the sqrt((M + 1) / M) factor of inference.lead_time_table).  Not reduced between ranks."""
        if self.ens_out is None:
            raise ValueError("ensemble_stats needs FusedTrainer(ensemble_members=M)")
        v = torch.cat([self.ens_out, self.stats[:5]]).cpu().tolist()
        if reset:
            self.ens_out.zero_()
        SA, SD, SV, cnt, S2, n = v[0], v[1], v[2], v[3], v[4], v[8]
        M = float(self.ensemble_members)
        if not cnt > 0:
            return dict(crps=float("nan"), rmse_mean=float("nan"), spread=float("nan"), spread_skill=float("nan"))
        kp = (M - 1.0 + self._ens_spec.alpha) / (M * M * (M - 1.0))
        rmse = (S2 / n) ** 0.5 if n > 0 else float("nan")
        spread = (SV / (M * M * (M - 1.0)) / cnt) ** 0.5
        return dict(crps=(SA / M - kp * SD) / cnt, rmse_mean=rmse, spread=spread,
                    spread_skill=((M + 1.0) / M) ** 0.5 * spread / rmse if rmse > 0 else float("nan"))

    def _finish(self, last: bool, pending=None, n0: int = 0) -> torch.Tensor:
        """The end of every call: on the last one of a group the all-reduce of the bucket -- ONE, or with `pending` (the
        asynchronous exchange of the bucket from element `n0` on, started under layer 0's weight gradient) that of the first
        n0 elements -- and the optimizer step."""
        if not last:
            self._micro += 1
            return self.scratch[0]
        self._micro = 0
        if pending is not None:
            self.dist.all_reduce(self.flat.grad[:n0], op=self.dist.ReduceOp.SUM, group=self.pg)
            pending.wait()                         # (stream-level for RCCL: the step stays asynchronous to the host)
        elif self.distributed:
            # (frozen layers lead the bucket -- module parameter order --: the trained tail alone is exchanged; all of it without)
            g = self.flat.grad[self.optimizer.n0:] if self.optimizer.n0 else self.flat.grad
            self.dist.all_reduce(g, op=self.dist.ReduceOp.SUM, group=self.pg)   # RCCL over xGMI
        self.optimizer.step(grad_scale=1.0 / (self.accumulate_steps * self.world))
        self._mark()
        return self.scratch[0]

    def _segments(self, eng, X, yv, plan, carried, acc: bool, wts, spec=None, draw: int = 0):
        """Checkpointed BPTT of one window: the gradients of the whole window into the bucket, with S = T / n
        steps resident instead of T.
          1. forward sweep: segments 0 .. n-2 in an S-step inference workspace (no stash, no dG), each from the state the one
             before left; the state at the start of every segment is kept (B images of h and c per layer each)
          2. segment n-1 in the S-step training workspace, the head / loss pass on its last h, BPTT from zero state gradients
             (the bucket is overwritten, or added to for a later micro-batch)
          3. segments n-2 .. 0: load the segment's start state, recompute its forward with the stash on, BPTT with
             accumulate = 1; its entry gradients dL/dh, dL/dc are what the call before left in ws.dh / ws.dc -- no copy
        Segment 0 starts from the zero state, or from the carried one (stateful: gradients still stop at the chunk start, and
        the carried state becomes the one segment n-1 ended in).  A zero-state segment 0 runs as the whole window's first
        steps do (SeqEngine.zero_start: the h half of K skipped at t = 0), so every segment's forward pass has the whole
        window's bits and so has the loss.  Input noise (``draw``): every pass over a segment carries the segment's start as step0,
        so the sweep and the recompute add the same noise, the whole window's."""
        m, L, mark = self.model, self.model.num_layers, self._mark
        B, T, _, H, W = X.shape
        n, S, f = len(plan), plan[0][1], self.freeze_layers
        seg = (lambda t0: X.segment(t0, S)) if hasattr(X, "segment") else (lambda t0: X[:, t0:t0 + S])
        if carried is None:
            self._zero = self._state_for(self._zero, eng, B, H, W)
        states = [carried if carried is not None else self._zero]
        with eng.window(B, S, H, W, False, True) as wf:
            for t0, _ in plan[:-1]:
                eng.load_state(wf, states[-1])
                eng.zero_start(wf, carried is None and t0 == 0)
                eng.forward(wf, seg(t0), **self._res_kw(), **self._noise_kw(draw, B, t0))
                states.append(eng.save_state(wf))        # slot S -> a new state: the start of the next segment
        with eng.window(B, S, H, W, True, True, f) as ws:
            eng.load_state(ws, states[-1])
            eng.forward(ws, seg(plan[-1][0]), **self._res_kw(), **self._noise_kw(draw, B, plan[-1][0]))
            if carried is not None:
                self.state = eng.save_state(ws)          # (a new object: the chunk's start state above stays what it was)
                self._drop_nonfinite_lanes(self.state)
            mark()
            O = m.conv.weight.shape[0]
            self._head_pass(eng, ws, yv, B, S, O, H, W, yv.shape[-2], yv.shape[-1], wts, acc, spec)
            mark()
            eng.backward(ws, False, zero_state_grads=range(L), dW_out=self._dW, db_out=self._db, accumulate=acc, train_from=f)
            for j in range(n - 2, -1, -1) if f < L else ():      # (the head alone: its gradient is the last segment's)
                eng.load_state(ws, states[j])
                eng.zero_start(ws, carried is None and j == 0)
                eng.forward(ws, seg(plan[j][0]), **self._res_kw(), **self._noise_kw(draw, B, plan[j][0]))
                eng.backward(ws, False, zero_state_grads=(), dW_out=self._dW, db_out=self._db, accumulate=True, train_from=f)
            mark()

    def _mark(self):
        """bench.py --phase-events: one HIP event per phase boundary of a step (nothing is recorded unless asked for)"""
        if self._marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream())
            self._marks.append(ev)

    @torch.no_grad()
    def evaluate(self, X: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Forward + loss only (val_loop, utils.py:52-75); accumulates the R2 statistics.  With ``sequence_loss`` the loss runs
        over every step and the (B, T*O, H, W) sequence is returned."""
        eng, ws, pred, _ = self.forward_loss(X, y, False)
        eng.release(ws)
        return pred

    # ------------------------------------------------------------------ epoch statistics
    def reset_stats(self):
        self.stats.zero_()

    def grad_stats(self, reset: bool = False) -> dict:
        """The guarded optimizer's figures (FusedAdam.grad_stats): applied / skipped / clipped steps, calls, mean / max / last
        gradient norm and the last clip coefficient.  One device read; identical on every rank."""
        return self.optimizer.grad_stats(reset)

    def epoch_stats(self, pooled: bool = False):
        """One device->host read per epoch.  Returns what the reference logs over everything accumulated since
        reset_stats(): (mean of the per-batch losses -- of the configured loss, with ``loss`` / set_loss --, mean of the per-batch sklearn ``r2_score``) -- train.py:113-117;
        for the validation loop at batch size 1 that is the mean of per-sample R2 (utils.py:73-75).  Under DDP
        the sums are all-reduced first, so the means run over every rank's batches.
        ``pooled=True`` appends the pooled R2 over all elements seen (1 - sum d^2 / sum (y - mean y)^2)."""
        s = self.stats.clone()
        if self.world > 1:
            self.dist.all_reduce(s, op=self.dist.ReduceOp.SUM, group=self.pg)
        s2, s1, sy, syy, n, sl, sr2, calls = (float(v) for v in s.cpu())
        if calls == 0:
            return (float("nan"),) * (3 if pooled else 2)
        out = (sl / calls, sr2 / calls)
        if pooled:
            ss_tot = syy - sy * sy / n
            out += (1.0 - s2 / ss_tot if ss_tot > 0 else float("nan"),)
        return out
