"""Host-side engine: owns the device workspaces (allocated through torch's caching allocator,
sized for 288 GB of HBM: every time step's slabs stay resident) and drives the C-ABI HIP
library for one ConvLSTM forward / BPTT.  No arithmetic happens in Python or in torch ops."""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (NINT_BF16, NINT_F32, NintFeedback, NintFeedbackGrad, NintFeedbackMask, NintFeedbackNoise, NintGeom, NintHeadBase, NintLayer, NintLossSpec,
                   NintSeq, check, ptr, stream_ptr)

# 0: the library picks the gate / dgrad pixel-tile height per launch shape; 4 or 8 forces it for every layer of
# engines built afterwards (nint_layer.tile_rows) -- how the tests run both heights on every shape
FORCE_TILE_ROWS = 0
# Thin first-layer inputs (the reference's Conv2d(5+64 -> 256, k=5), model.py:207-211) are fed HORIZONTALLY FOLDED
# when that lowers the number of MFMA K-steps (nint_xfold_pays): 5 x-steps instead of 25.  (Any channel count and grid width
# packs: row tiles up to 160 KiB go through the LDS-tiled pack kernel, wider ones through the per-element one.)  False keeps the plain
# channel-padded layout for engines built afterwards (tests run both).
XFOLD = True
# nint_layer.wide of engines built afterwards (weight-gradient kernel family): 0 = the library's choice, 1 = always the 4-wave
# 64-column kernel, 2 = the 8-wave 128-column kernel wherever it is instantiated (tests run both against each other)
FORCE_WIDE = 0
FORCE_WAVE = None        # merged grids (nint_seq.wave): None = by batch size (SeqEngine._set_wave), 0 = never, 1 = forward wavefront + backward pair, 2 = forward wavefront only (8-row tiles), 4 = 2 + the BPTT pairs (dgrad 0 + dgrad 1, pointwise 0 + the top layer's fused step), 5 = the forward pass of 1 + the BPTT pairs of 4
WAVE_TILES_PER_CU = 1.5   # ... wave = 5 (the layers' own tiles) while 2 * (8-row pixel tiles of the batch) < WAVE_TILES_PER_CU * CUs: B = 1 at 100 x 154; wave = 4 above
FUSE_BWD = 0          # nint_seq.fuse_bwd of new workspaces: 0 = per layer, 1 = never fused, 2 = every layer fused (tests run all three)

RESIDUAL_STEP0 = ("residual head: step 0 cannot be fed -- the fed value is the prediction of the step before, p_{-1} = x_{-1}[feedback "
                  "channels] + head(h_{-1}), and no input precedes the window, even with an initial state; feed from step 1 on "
                  "(free_from >= 1, or a mask whose column 0 is clear)")

DTYPES = {"f32": NINT_F32, "fp32": NINT_F32, "float32": NINT_F32, "bf16": NINT_BF16, "bfloat16": NINT_BF16}


def dtype_code(d) -> int:
    if isinstance(d, int):
        return d
    if isinstance(d, torch.dtype):
        return NINT_BF16 if d == torch.bfloat16 else NINT_F32
    return DTYPES[str(d).lower()]


def _rup(a: int, b: int) -> int:
    return (a + b - 1) // b * b


@dataclass
class LayerCfg:
    Cx: int
    Ch: int
    k: int
    xfold: bool = False      # x source horizontally folded (thin first-layer inputs; set by SeqEngine, nint_layer.xfold)

    def padded(self, kc: int) -> Tuple[int, int, int]:
        return _rup(self.k * self.Cx if self.xfold else self.Cx, kc), _rup(self.Ch, 16), _rup(self.Ch, kc)


class Feedback:
    """What the last forward pass on a workspace fed back: its nint_feedback (O = 0: nothing), the
    tensors its pointers name, the ``feedback_grad`` mark (the window will be trained through what it fed) and the roll-out
    backward's two buffers -- the f32 slab of the per-step head cotangents and the one-step d/dx scratch, None until asked for.
    Scheduled sampling: ``mask``, the pinned host uint8 (T, B) array that ``fm`` (nint_feedback_mask) points
    at, or None; ``fb.from_step`` is then F, the first step with a fed image, so ``fed`` stays the range [F, T).
    Residual head: ``res`` -- the pass ran for a head that predicts the increment, p_t = x_t[feedback channels] +
    head(h_t); every head call on the workspace then adds that base, fed or not (``fb.O`` may be 0: a teacher-forced window)."""

    def __init__(self, T: int, B: int = 1):
        self.T, self.fb, self.keep, self.grad, self.dpred, self.dx_step = T, NintFeedback(), None, False, None, None
        self.B, self.res = B, False
        self.noise = None               # the nint_feedback_noise of the last forward pass, or None
        self.fm, self.mask, self._pin = NintFeedbackMask(), None, None

    @staticmethod
    def steps(from_step: int, T: int) -> range:
        """the steps [F, T) of a T-step window that a closed loop from ``from_step`` feeds, F clamped into [0, T]"""
        return range(min(max(int(from_step), 0), T), T)

    fed = property(lambda self: self.steps(self.fb.from_step if self.fb.O > 0 else self.T, self.T),
                   doc="the steps [F, T) that were fed (empty: the open loop, or a closed loop that starts beyond the window)")

    @staticmethod
    def mask_bt(mask, B: int, T: int) -> torch.Tensor:
        """a feed mask as the host layers take it -- a bool / uint8 tensor or array of shape (B, T), every value 0 or 1 -- as a
        CPU uint8 tensor (B, T); ValueError otherwise.  Pure: no device is asked for."""
        m = torch.as_tensor(mask).detach().cpu()
        if m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != (B, T):
            raise ValueError(f"feed mask: a bool / uint8 tensor or array of shape (B, T) = ({B}, {T}) is needed, got "
                             f"{m.dtype} {tuple(m.shape)}")
        m = m.to(torch.uint8)
        if bool((m > 1).any()):
            raise ValueError("feed mask: every value must be 0 or 1")
        return m

    @staticmethod
    def first_fed(m_bt: torch.Tensor) -> int:
        """F of a (B, T) mask: the first step with a fed image, T if there is none"""
        any_t = m_bt.bool().any(dim=0)
        return int(any_t.to(torch.uint8).argmax()) if bool(any_t.any()) else int(m_bt.shape[1])

    @property
    def fed_mask(self) -> torch.Tensor:
        """(B, T) bool, CPU: image b ran step t on the fed-back prediction (all False: the open loop)"""
        if self.mask is not None and self.fb.O > 0:
            return self.mask.t().bool()
        return (torch.arange(self.T) >= self.fed.start).expand(self.B, self.T).clone()

    def set(self, w=None, b=None, O: int = 0, from_step: int = 0, grad: bool = False, mask=None, res: bool = False):
        """``mask``: a CPU uint8 (B, T) tensor (``mask_bt``) in the place of ``from_step``"""
        self.keep = (w, b)          # the pointers below stay valid as long as the fields name them
        self.res = bool(res)
        self.mask, self.fm.fed = None, None
        if mask is not None:
            # one pinned (T, B) buffer per workspace, time-major (index t*B + b), reused pass after pass: the library reads it on
            # the host while it plans, inside the call, so nothing is in flight from it when the next pass fills it
            if self._pin is None or tuple(self._pin.shape) != (mask.shape[1], mask.shape[0]):
                self._pin = torch.empty(mask.shape[1], mask.shape[0], dtype=torch.uint8, pin_memory=True)
            tb = self._pin
            tb.copy_(mask.t())
            self.mask, self.fm.fed, from_step = tb, tb.data_ptr(), self.first_fed(mask)
        self.fb.w, self.fb.b, self.fb.O, self.fb.from_step, self.grad = ptr(w), ptr(b), O, from_step, grad


@dataclass(frozen=True)
class InputNoise:
    """Seeded Gaussian noise on a span of the input's channels, drawn on the device (include/nint.h: THE RULE).
    ``std``: one float or n floats, in the units of the stored (z-scored) input; ``channels = (c0, n)``, None: the feedback
    channels of the module that takes it (the last out_channels).  The noise of an element is a pure function of (seed, draw,
    lane0 + b, step0 + t, channel offset, pixel): ``draw`` tells one pass from the next, ``step0`` places a segment in its
    window, ``lane0`` a rank's batch in the global one.  A negative or non-finite ``std`` is refused here."""
    std: object
    channels: Optional[Tuple[int, int]] = None
    seed: int = 0
    draw: int = 0
    step0: int = 0
    lane0: int = 0

    def __post_init__(self):
        std = self.std
        try:
            vals = tuple(float(v) for v in std) if hasattr(std, "__iter__") else (float(std),)
        except (TypeError, ValueError):
            raise ValueError(f"InputNoise: std must be a float or a sequence of floats, got {std!r}") from None
        if not vals or any(not (v >= 0.0) or v == float("inf") for v in vals):
            raise ValueError(f"InputNoise: std must be finite and >= 0, got {std!r}")
        object.__setattr__(self, "std", vals if hasattr(std, "__iter__") else vals[0])
        if self.channels is not None:
            ch = tuple(self.channels)
            if len(ch) != 2 or any(isinstance(v, bool) or int(v) != v for v in ch):
                raise ValueError(f"InputNoise: channels must be (c0, n), got {self.channels!r}")
            object.__setattr__(self, "channels", (int(ch[0]), int(ch[1])))
        for name in ("seed", "draw", "step0", "lane0"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < 0:
                raise ValueError(f"InputNoise: {name} must be an integer >= 0, got {v!r}")
            object.__setattr__(self, name, int(v) & 0xffffffff)

    @property
    def active(self) -> bool:
        """False: an all-zero std -- no launch, no allocation, the bits of a pass without noise"""
        return any(v != 0.0 for v in (self.std if isinstance(self.std, tuple) else (self.std,)))

    def span(self, C: int, feedback_O: Optional[int] = None) -> Tuple[int, int, Tuple[float, ...]]:
        """(c0, n, the n sigmas) on an input of C channels; ValueError for a span outside [0, C), a std whose length is not n,
        or channels=None where there are no feedback channels"""
        if self.channels is None:
            if not feedback_O:
                raise ValueError("InputNoise(channels=None) means the feedback channels, and this module was built without "
                                 "feedback=True: give channels=(c0, n)")
            c0, n = C - int(feedback_O), int(feedback_O)
        else:
            c0, n = self.channels
        if n < 1 or c0 < 0 or c0 + n > C:
            raise ValueError(f"InputNoise: channels [{c0}, {c0 + n}) lie outside the input's [0, {C})")
        sig = self.std if isinstance(self.std, tuple) else (self.std,) * n
        if len(sig) != n:
            raise ValueError(f"InputNoise: {len(sig)} std values for {n} channels")
        return c0, n, sig


class Workspace:
    """All slabs of one (B, T, H, W) problem.  Halo slabs are zero-initialised once; kernels only
    ever write their interior, so the zero padding of nn.Conv2d (model.py:207-211) is physical."""

    def __init__(self, eng: "SeqEngine", B: int, T: int, H: int, W: int, train: bool, has_init: bool, train_from: int = 0):
        self.key = SeqEngine.pool_key(B, T, H, W, train, has_init, train_from)
        self.B, self.T, self.H, self.W, self.train = B, T, H, W, train
        # fine-tuning (nint_seq.train_from): layers below it are frozen -- no gate stash (the forward pass then writes none), no
        # dG, no dc and no dh; their slots hold None.  The top layer's dh stays whatever is frozen: the head pass writes it.
        self.train_from = train_from
        self.in_use = False
        self.gen = 0            # bumped by every SeqEngine.acquire: an autograd graph stamps it and refuses a backward after a reuse
        dev, es = eng.device, eng.es
        lib = _lib.load()
        self.g = NintGeom()
        check(lib.nint_geom_make(C.byref(self.g), H, W, eng.P), "nint_geom_make")
        g = self.g
        halo_px, comp_px = g.Hh * g.Wh, H * W
        u8 = dict(dtype=torch.uint8, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        Cxp0 = eng.layers[0].Cxp
        self.xs = torch.zeros(T * B * halo_px * Cxp0 * es, **u8)
        self.h, self.c, self.gates, self.dG, self.dh, self.dc = [], [], [], [], [], []
        for ly in eng.layers:
            Ch16, Chp = ly.Ch16, ly.Chp
            self.h.append(torch.zeros((T + 1) * B * halo_px * Chp * es, **u8))
            self.c.append(torch.zeros((T + 1) * B * comp_px * Chp, **f32))
            if train:
                live = len(self.h) - 1 >= train_from
                self.gates.append(torch.empty(T * B * comp_px * 4 * Ch16 * es, **u8) if live else None)
                self.dG.append(torch.zeros(T * B * halo_px * 4 * Ch16 * es, **u8) if live else None)
                self.dh.append(torch.zeros(B * comp_px * Chp * es, **u8)       # ET: transient gradient, read once per step
                               if live or ly is eng.layers[-1] else None)
                self.dc.append(torch.zeros(B * comp_px * Chp, **f32) if live else None)
        self.dx = None
        self._dh_seq = None
        self.Cxp0 = Cxp0
        self.feedback = Feedback(T, B)     # closed loop, roll-out training: what the last forward pass on this workspace fed back
        self.seq = NintSeq()
        s = self.seq
        s.dtype, s.B, s.T, s.L = eng.dt, B, T, len(eng.cfgs)
        s.need_dx, s.has_init_state, s.n_cu = 0, int(has_init), eng.n_cu
        s.fuse_bwd = FUSE_BWD
        s.lon_cyclic = int(eng.lon_cyclic)
        s.g = g
        s.xs = self.xs.data_ptr()
        for l in range(len(eng.cfgs)):
            s.h[l] = self.h[l].data_ptr()
            s.c[l] = self.c[l].data_ptr()
            if train and l >= train_from:
                s.gates[l] = self.gates[l].data_ptr()
                s.dG[l] = self.dG[l].data_ptr()
                s.dh[l] = self.dh[l].data_ptr()
                s.dc[l] = self.dc[l].data_ptr()
        if train:
            s.wg_partial = eng.wg_partial.data_ptr()
            s.wg_partial_bytes = eng.wg_partial.numel() * 4

    def dh_seq_slab(self, eng) -> torch.Tensor:
        """ET compact [T*B][H][W][Chp of the top layer]: the per-step head gradients (nint_seq.dh_seq).  Allocated when
        sequence gradients are first asked for on this workspace: the many-to-one path never pays for it."""
        if self._dh_seq is None:
            self._dh_seq = torch.empty(self.T * self.B * self.H * self.W * eng.layers[-1].Chp * eng.es, dtype=torch.uint8, device=eng.device)
        return self._dh_seq

    fb = property(lambda self: self.feedback.fb)       # the nint_feedback of the last forward pass

    def rollout_dpred(self, eng, O: int) -> torch.Tensor:
        """f32 (T*B, O, H, W), image t*B + b: the direct cotangent l_t of every step's head output going into the roll-out
        backward, g_t = l_t + (the gradient that came back through the feedback) coming out (nint_feedback_grad.dpred)"""
        if self.feedback.dpred is None or self.feedback.dpred.shape[1] != O:
            self.feedback.dpred = torch.empty(self.T * self.B, O, self.H, self.W, dtype=torch.float32, device=eng.device)
        return self.feedback.dpred

    # byte offsets of slab (t) inside the per-layer stacks
    def h_view(self, eng, l: int, slot: int) -> int:
        return self.h[l].data_ptr() + slot * self.B * self.g.Hh * self.g.Wh * eng.layers[l].Chp * eng.es

    def c_view(self, eng, l: int, slot: int) -> int:
        return self.c[l].data_ptr() + slot * self.B * self.H * self.W * eng.layers[l].Chp * 4


class ConvLSTMState:
    """The recurrent state (h, c) of every layer of one engine, kept on the device IN SLAB FORM: per layer
    an ET halo slab [B][Hh][Wh][Chp] for h and an f32 compact slab [B][H][W][Chp] for c -- the very bytes of slot T of a
    workspace, so carrying it into the next call costs ONE launch (nint_state_copy) and no f32 NCHW round trip.
    Detached by construction: it is not a tensor autograd knows, so a chain of calls through it is TRUNCATED BPTT --
    gradients stop at the chunk boundary.  (Pass the (h, c) tensor pairs instead for gradients across the boundary.)
    A state belongs to the engine that made it (layer widths, storage dtype, halo P, boundary condition) and to one
    (B, H, W).  A cyclic-longitude engine's h images carry wrapped halo columns: they never reach a
    zero-padding engine."""

    def __init__(self, eng: "SeqEngine", B: int, H: int, W: int, zero: bool = True):
        self.eng, self.B, self.H, self.W = eng, int(B), int(H), int(W)
        if self.B < 1 or self.H < 1 or self.W < 1:
            raise ValueError(f"ConvLSTMState: B, H, W must be positive, got {(B, H, W)}")
        self.g = NintGeom()
        check(eng.lib.nint_geom_make(C.byref(self.g), self.H, self.W, eng.P), "nint_geom_make")
        new = torch.zeros if zero else torch.empty       # (a state that one whole-image copy fills at once needs no fill)
        self.h, self.c = [], []
        for ly in eng.layers:
            self.h.append(new(self.B * self.g.Hh * self.g.Wh * ly.Chp * eng.es, dtype=torch.uint8, device=eng.device))
            self.c.append(new(self.B * self.H * self.W * ly.Chp, dtype=torch.float32, device=eng.device))

    @property
    def dtype(self) -> str:
        return "bf16" if self.eng.dt == NINT_BF16 else "f32"

    @property
    def layers(self) -> List[int]:
        return [cfg.Ch for cfg in self.eng.cfgs]

    def _ptrs(self):
        return [t.data_ptr() for t in self.h], [t.data_ptr() for t in self.c]

    def tensors(self) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """The reference's ``hidden_states`` list: [(h, c)] per layer, (B, Ch, H, W) f32 (model.py:259-262,270)."""
        eng, B, g = self.eng, self.B, self.g
        return [(eng._unpack_h(l, h.data_ptr(), B, g), eng._unpack_compact(l, c.data_ptr(), B, g))
                for l, (h, c) in enumerate(zip(self.h, self.c))]

    def select(self, lanes: Sequence[int]) -> "ConvLSTMState":
        """A new state whose sample b is this state's sample lanes[b] -- a permutation, a subset, a repetition -- or the zero
        state where lanes[b] is -1 (that lane starts a new record).  One launch."""
        lanes = [int(v) for v in lanes]
        if not lanes or any(v < -1 or v >= self.B for v in lanes):
            raise ValueError(f"ConvLSTMState.select: lanes must be a non-empty sequence of values in [-1, {self.B}), got {lanes}")
        out = ConvLSTMState(self.eng, len(lanes), self.H, self.W, zero=False)
        self.eng._state_copy(out._ptrs(), self._ptrs(), out.B, self.B, lanes, self.g)
        return out

    def reset(self, mask=None) -> "ConvLSTMState":
        """Zero state for every sample (mask None) or for the samples whose mask entry is true; the others keep theirs.  The
        object is changed in place (its buffers are replaced by the result of one launch)."""
        if mask is None:
            lanes = [-1] * self.B
        else:
            m = [bool(v) for v in (mask.tolist() if hasattr(mask, "tolist") else mask)]
            if len(m) != self.B:
                raise ValueError(f"ConvLSTMState.reset: mask has {len(m)} entries, the state has B = {self.B}")
            lanes = [-1 if v else b for b, v in enumerate(m)]
        if any(v < 0 for v in lanes):
            new = self.select(lanes)
            self.h, self.c = new.h, new.c
        return self

    def clone(self) -> "ConvLSTMState":
        return self.select(range(self.B))


class SeqEngine:
    def __init__(self, cfgs: Sequence[LayerCfg], dtype="f32", device="cuda", lon_cyclic: bool = False):
        """``lon_cyclic`` (nint_seq.lon_cyclic): column 0 and column W-1 are neighbours in every convolution
        of the stack -- every workspace's plan carries the halo wrap launches, and a folded input is packed, preprocessed
        and unfolded by the _cyclic entries.  False: zero padding, the engine as it has always been."""
        if len(cfgs) < 1 or len(cfgs) > _lib.NINT_MAX_LAYERS:
            raise ValueError("1..8 layers supported")
        self.lon_cyclic = bool(lon_cyclic)
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.NintError("the ConvLSTM hot path runs on the MI355X only (device must be cuda); "
                                 "there is no CPU fallback")
        self.dt = dtype_code(dtype)
        self.es = 2 if self.dt == NINT_BF16 else 4
        self.kc = self.lib.nint_kc(self.dt)
        self.cfgs = [LayerCfg(c.Cx, c.Ch, c.k, bool(l == 0 and XFOLD and self.lib.nint_xfold_pays(c.Cx, c.k, self.dt)))
                     for l, c in enumerate(cfgs)]
        self.P = max(c.k // 2 for c in cfgs)
        for c in cfgs:
            if c.k % 2 == 0:
                raise ValueError("odd kernel sizes only (padding k//2, model.py:204)")
        n_cu = C.c_int(0)
        with torch.cuda.device(self.device):
            check(self.lib.nint_device_info(C.byref(n_cu), None, None, None, 0), "nint_device_info")
        self.n_cu = n_cu.value
        u8 = dict(dtype=torch.uint8, device=self.device)
        self.Wf, self.Wd, self.bias_p, self.layers = [], [], [], []
        wg_bytes = 0
        for cfg in self.cfgs:
            nbytes = self.lib.nint_packed_weight_bytes(cfg.Cx, cfg.Ch, cfg.k, self.dt, int(cfg.xfold))
            Cxp, Ch16, Chp = cfg.padded(self.kc)
            self.Wf.append(torch.zeros(nbytes, **u8))
            self.Wd.append(torch.zeros(nbytes, **u8))
            self.bias_p.append(torch.zeros(4 * Ch16, dtype=torch.float32, device=self.device))
            ly = NintLayer()
            ly.Cx, ly.Cxp, ly.Ch, ly.Ch16, ly.Chp, ly.k = cfg.Cx, Cxp, cfg.Ch, Ch16, Chp, cfg.k
            ly.xfold = int(cfg.xfold)
            ly.Wf, ly.Wd, ly.bias_p = self.Wf[-1].data_ptr(), self.Wd[-1].data_ptr(), self.bias_p[-1].data_ptr()
            self.layers.append(ly)
            ly.tile_rows = FORCE_TILE_ROWS
            ly.wide = FORCE_WIDE
            # the layers' split-K slabs sit side by side in one workspace: one launch folds them all
            wg_bytes += (self.lib.nint_wgrad_workspace_bytes(C.byref(ly), self.dt, self.n_cu) + 255) // 256 * 256
        # shapes the weight-gradient kernel has no instantiation for: known NOW, reported at the first training
        # workspace (forward / inference work for every odd k) instead of as a shape error in the first backward()
        self.train_unsupported = self.untrainable_layers(self.cfgs, self.dt, self.n_cu)
        self._wg_bytes = wg_bytes
        self._wg_partial = None
        self._noise_sigma: Dict[tuple, torch.Tensor] = {}      # InputNoise's sigmas on the device, by value
        self.pool: Dict[tuple, List[Workspace]] = {}

    @property
    def wg_partial(self):
        if self._wg_partial is None:
            # exactly the sum of the layers' nint_wgrad_workspace_bytes, each rounded up to 256 bytes: the query is an upper bound
            # for every N and the planner checks it (tests/test_gpu_memory_contract.py runs it at this size)
            self._wg_partial = torch.empty(self._wg_bytes // 4, dtype=torch.float32, device=self.device)
        return self._wg_partial

    # ------------------------------------------------------------------ weights
    def pack_weights(self, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]]):
        """OIHW f32 conv weights of every layer -> MFMA fragment order (fwd + dgrad images) and permuted bias: one launch."""
        L = len(self.cfgs)
        Ws, bs = [], []
        for l, cfg in enumerate(self.cfgs):
            W = weights[l].detach()
            if W.dtype != torch.float32 or not W.is_contiguous():
                W = W.float().contiguous()
            assert tuple(W.shape) == (4 * cfg.Ch, cfg.Cx + cfg.Ch, cfg.k, cfg.k), W.shape
            b = biases[l]
            if b is not None:
                b = b.detach()
                if b.dtype != torch.float32 or not b.is_contiguous():
                    b = b.float().contiguous()
            Ws.append(W); bs.append(b)
        wp = (C.c_void_p * L)(*[W.data_ptr() for W in Ws])
        bp = (C.c_void_p * L)(*[None if b is None else b.data_ptr() for b in bs])
        lys = (NintLayer * L)(*self.layers)
        check(self.lib.nint_pack_weights_layers(wp, bp, lys, L, self.dt, stream_ptr()), "nint_pack_weights_layers")

    @staticmethod
    def untrainable_layers(cfgs: Sequence[LayerCfg], dtype, n_cu: int = 256, train_from: int = 0) -> List[str]:
        """Layers whose weight gradient no kernel instantiation covers (`nint_wgrad_workspace_bytes` == 0):
        kernel sizes other than 1, 3, 5, 7.  Only the layers from ``train_from`` on are asked about: a frozen layer needs no
        weight gradient.  Pure host
        arithmetic -- callable without a GPU."""
        lib = _lib.load()
        dt = dtype_code(dtype)
        kc = lib.nint_kc(dt)
        bad = []
        for l, cfg in enumerate(cfgs):
            if l < train_from:
                continue
            ly = NintLayer()
            ly.Cx, ly.Ch, ly.k, ly.xfold = cfg.Cx, cfg.Ch, cfg.k, int(cfg.xfold)
            ly.Cxp, ly.Ch16, ly.Chp = cfg.padded(kc)
            if lib.nint_wgrad_workspace_bytes(C.byref(ly), dt, n_cu) == 0:
                bad.append(f"layer {l} (Cin={cfg.Cx}, Ch={cfg.Ch}, k={cfg.k})")
        return bad

    # ------------------------------------------------------------------ workspaces
    def acquire(self, B, T, H, W, train: bool, has_init: bool, train_from: int = 0) -> Workspace:
        """``train_from`` (training workspaces): the first layer that is trained; the layers below it get no stash and no
        gradient slabs (Workspace), and a kernel size the weight-gradient kernel lacks is refused only from there on."""
        train_from = int(train_from) if train else 0
        if not 0 <= train_from <= len(self.cfgs):
            raise ValueError(f"train_from must be in [0, {len(self.cfgs)}], got {train_from}")
        bad = self.train_unsupported if train else []
        if bad and train_from:
            bad = self.untrainable_layers(self.cfgs, self.dt, self.n_cu, train_from)
        if bad:
            raise _lib.NintError("training is not supported for " + ", ".join(bad) + ": the weight-gradient "
                                 "kernel is instantiated for kernel sizes 1, 3, 5 and 7 only (the reference accepts any odd k, "
                                 "model.py:204); forward / inference (torch.no_grad()) work for every odd k")
        key = self.pool_key(B, T, H, W, train, has_init, train_from)
        pool = self.pool.setdefault(key, [])
        ws = next((w for w in pool if not w.in_use), None)
        if ws is None:
            ws = Workspace(self, B, T, H, W, train, has_init, train_from)
            for l, ly in enumerate(self.layers):
                ws.seq.layer[l] = ly
            pool.append(ws)
        else:
            ws.seq.probe, ws.seq.probe_mask, ws.seq.probe_slots = None, 0, 0     # (a trainer's timing probes do not outlive its step)
            ws.seq.has_init_state = int(has_init)                                # (nor does a zero_start)
        ws.in_use = True
        ws.gen += 1
        return ws

    @staticmethod
    def pool_key(B, T, H, W, train: bool, has_init: bool, train_from: int = 0) -> tuple:
        """the pool's key of a workspace: (B, T, H, W, train, has_init), with train_from behind it where layers are frozen
        (a run that freezes nothing keeps the keys it has always had)"""
        return (B, T, H, W, train, has_init) + ((train_from,) if train_from else ())

    @staticmethod
    def release(ws: Workspace):
        ws.in_use = False

    @contextlib.contextmanager
    def window(self, B, T, H, W, train: bool, has_init: bool, train_from: int = 0):
        """``with eng.window(...) as ws``: acquire, and the release whatever happens inside -- how a caller that does not
        hand the workspace to an autograd graph runs a window (pack_weights, [load_state,] forward, ... in the body)"""
        ws = self.acquire(B, T, H, W, train, has_init, train_from)
        try:
            yield ws
        finally:
            self.release(ws)

    # ------------------------------------------------------------------ carried state
    def new_state(self, B: int, H: int, W: int) -> ConvLSTMState:
        """the zero state of a (B, H, W) problem (model.py:259-262) in device form"""
        return ConvLSTMState(self, B, H, W)

    def state_from_tensors(self, pairs) -> ConvLSTMState:
        """[(h, c)] per layer, (B, Ch, H, W) tensors on the engine's device -> a (detached) device state"""
        hs, cs = self._state_tensors(pairs, None)
        B, _, H, W = hs[0].shape
        st = ConvLSTMState(self, B, H, W)
        self._write_state(hs, cs, st._ptrs(), B, st.g)
        return st

    # ------------------------------------------------------------------ the NCHW <-> slab boundary
    # The only code that knows how a (B, Ch, H, W) f32 tensor of layer l lies in a slab: h in ET halo images [B][Hh][Wh][Chp],
    # everything else (c, dL/dh, dL/dc) in compact images [B][H][W][Chp], f32 or (`et`) the engine's element type.  Slabs are
    # given by device address, `g` is the problem's NintGeom, `what` the name a failing call is reported under.  The packers
    # view the normalised tensor in the shape the kernel will read: a tensor of another size is refused (RuntimeError) before
    # the launch, never read past its end.
    def _pack_h(self, l: int, t: torch.Tensor, dst: int, B: int, g: NintGeom, what: str = "pack h"):
        ly = self.layers[l]
        src = t.detach().float().contiguous().view(B, 1, ly.Ch, g.H, g.W)
        check(self.lib.nint_pack_btchw(ptr(src), C.c_void_p(dst), B, 1, ly.Ch, ly.Chp, C.byref(g), self.dt, stream_ptr()), what)

    def _pack_compact(self, l: int, t: torch.Tensor, dst: int, B: int, g: NintGeom, et: bool = False, what: str = "pack c",
                      add: bool = False):
        """`add`: the slab receives old + t (nint_pack_compact_add) instead of t"""
        ly = self.layers[l]
        fn = self.lib.nint_pack_compact_add if add else self.lib.nint_pack_compact
        src = t.detach().float().contiguous().view(B, ly.Ch, g.H, g.W)
        check(fn(ptr(src), C.c_void_p(dst), B, ly.Ch, ly.Chp, g.H, g.W, self.dt if et else NINT_F32, stream_ptr()), what)

    def _unpack_h(self, l: int, src: int, B: int, g: NintGeom, image0: int = 0) -> torch.Tensor:
        """images image0 .. image0 + B of the halo slab that starts at `src`"""
        ly = self.layers[l]
        out = torch.empty(B, ly.Ch, g.H, g.W, dtype=torch.float32, device=self.device)
        check(self.lib.nint_unpack_halo(C.c_void_p(src), ptr(out), image0, B, ly.Ch, ly.Chp, C.byref(g), self.dt, stream_ptr()),
              "nint_unpack_halo")
        return out

    def _unpack_compact(self, l: int, src: int, B: int, g: NintGeom, et: bool = False, what: str = "nint_unpack_compact") -> torch.Tensor:
        ly = self.layers[l]
        out = torch.empty(B, ly.Ch, g.H, g.W, dtype=torch.float32, device=self.device)
        check(self.lib.nint_unpack_compact(C.c_void_p(src), ptr(out), B, ly.Ch, ly.Chp, g.H, g.W, self.dt if et else NINT_F32,
                                           stream_ptr()), what)
        return out

    def _write_state(self, hs, cs, dst, B: int, g: NintGeom, tag: str = ""):
        """the (h, c) tensors of every layer -> the (h pointers, c pointers) of a state or of a workspace slot"""
        for l in range(len(self.cfgs)):
            self._pack_h(l, hs[l], dst[0][l], B, g, "pack h" + tag)
            self._pack_compact(l, cs[l], dst[1][l], B, g, what="pack c" + tag)

    def _state_tensors(self, pairs, BHW):
        """validate a list of (h, c) tensor pairs against the engine (and a (B, H, W), when given): ValueError naming what differs"""
        pairs = list(pairs)
        if len(pairs) != len(self.cfgs):
            raise ValueError(f"state: {len(pairs)} (h, c) pairs given, the model has {len(self.cfgs)} layers")
        hs, cs = [], []
        for l, (cfg, hc) in enumerate(zip(self.cfgs, pairs)):
            if not isinstance(hc, (tuple, list)) or len(hc) != 2:
                raise ValueError(f"state: layer {l} must be an (h, c) pair of tensors")
            for name, t in zip("hc", hc):
                if not isinstance(t, torch.Tensor) or t.dim() != 4:
                    raise ValueError(f"state: {name} of layer {l} must be a (B, {cfg.Ch}, H, W) tensor")
                if not t.is_floating_point():
                    raise ValueError(f"state: {name} of layer {l} has dtype {t.dtype}, a floating-point tensor is expected")
                if t.device.type != self.device.type:
                    raise ValueError(f"state: {name} of layer {l} lives on {t.device}, the model on {self.device}")
                ref = pairs[0][0].shape          # (without a (B, H, W): the first tensor's)
                want = (BHW[0], cfg.Ch, BHW[1], BHW[2]) if BHW is not None else (ref[0], cfg.Ch, ref[2], ref[3])
                if tuple(t.shape) != want:
                    raise ValueError(f"state: {name} of layer {l} has shape {tuple(t.shape)}, expected {want} "
                                     "(B, hidden channels of the layer, grid of the input)")
            hs.append(hc[0]); cs.append(hc[1])
        return hs, cs

    def check_state(self, state: ConvLSTMState, B: int, H: int, W: int):
        """a device state against this engine and a (B, H, W) problem, before any launch: ValueError naming what differs"""
        eng = state.eng
        if eng is not self:
            if eng.dt != self.dt:
                raise ValueError(f"state: dtype {state.dtype}, the model computes in {'bf16' if self.dt == NINT_BF16 else 'f32'}")
            if [c.Ch for c in eng.cfgs] != [c.Ch for c in self.cfgs]:
                raise ValueError(f"state: layers {[c.Ch for c in eng.cfgs]}, the model has {[c.Ch for c in self.cfgs]}")
            if eng.P != self.P:
                raise ValueError(f"state: made by an engine with halo P = {eng.P}, this one has P = {self.P}")
            if eng.lon_cyclic != self.lon_cyclic:
                name = lambda cyc: "cyclic longitude" if cyc else "zero padding"
                raise ValueError(f"state: made by an engine with {name(eng.lon_cyclic)}, this one has {name(self.lon_cyclic)} "
                                 "(the h images of the two differ in their halo columns)")
        if state.B != B:
            raise ValueError(f"state: batch size B = {state.B}, the input has B = {B}")
        if (state.H, state.W) != (H, W):
            raise ValueError(f"state: grid {(state.H, state.W)}, the input has {(H, W)}")

    def _state_copy(self, dst, src, B_dst: int, B_src: int, lanes, g):
        """ONE nint_state_copy launch: (h pointers, c pointers) of every layer, destination <- source through `lanes`"""
        L = len(self.cfgs)
        arr = lambda v: (C.c_void_p * L)(*v)
        chp = (C.c_int32 * L)(*[ly.Chp for ly in self.layers])
        ln = None if lanes is None else (C.c_int32 * B_dst)(*[int(v) for v in lanes])
        check(self.lib.nint_state_copy(arr(dst[0]), arr(dst[1]), arr(src[0]), arr(src[1]), chp, L, B_dst, B_src, ln, C.byref(g),
                                       self.dt, stream_ptr()), "nint_state_copy")

    def _slot_ptrs(self, ws: Workspace, slot: int):
        L = range(len(self.cfgs))
        return [ws.h_view(self, l, slot) for l in L], [ws.c_view(self, l, slot) for l in L]

    def load_state(self, ws: Workspace, state: ConvLSTMState):
        """state -> slot 0 of a has_init workspace (the initial state the forward pass starts from): one launch"""
        if not ws.key[5]:
            raise ValueError("load_state needs a workspace acquired with has_init=True (others start from the zero state)")
        self.check_state(state, ws.B, ws.H, ws.W)
        self._state_copy(self._slot_ptrs(ws, 0), state._ptrs(), ws.B, ws.B, None, ws.g)

    def zero_start(self, ws: Workspace, on: bool):
        """A has_init workspace whose slot 0 holds the ZERO state runs its following passes as a zero-state window (``on``) --
        the first step skips the h half of K, BPTT writes no dL/dh_init and the weight gradient skips the zero h source: the
        launches and the bits of a has_init=False workspace, which an explicit all-zero state does not give
        -- or from the state in slot 0 again (off).  The segments of one window share a workspace this way (trainer.py)."""
        if not ws.key[5]:
            raise ValueError("zero_start needs a workspace acquired with has_init=True")
        ws.seq.has_init_state = 0 if on else 1

    def save_state(self, ws: Workspace, state: Optional[ConvLSTMState] = None) -> ConvLSTMState:
        """slot T of a workspace (h_{T-1}, c_{T-1} of every layer after forward) -> `state` (a new one if None): one launch"""
        if state is None:
            state = ConvLSTMState(self, ws.B, ws.H, ws.W, zero=False)
        else:
            self.check_state(state, ws.B, ws.H, ws.W)
        self._state_copy(state._ptrs(), self._slot_ptrs(ws, ws.T), ws.B, ws.B, None, ws.g)
        return state

    # ------------------------------------------------------------------ passes
    def forward(self, ws: Workspace, x: torch.Tensor, h0: Optional[List[torch.Tensor]] = None,
                c0: Optional[List[torch.Tensor]] = None, feedback=None, feedback_grad: bool = False, residual=False,
                noise: Optional[InputNoise] = None, feedback_noise: Optional[InputNoise] = None):
        """x (B,T,C,H,W) f32 on the engine's device, or a dataset.SlabBatch of that shape.  Runs model.py:253-271
        (all layers, all steps).

        ``feedback = (w, b, from_step)``: CLOSED LOOP -- the head ``w`` (O, Ch_top), ``b`` (O)
        or None, of the top layer's hidden state is rounded to the storage type and written into the last O input channels
        before every step ``t >= from_step``; earlier steps see what ``x`` holds.  The input slab is filled from ``x`` first
        (tensor or SlabBatch), then the pass writes into it.  from_step = 0 needs a has_init workspace.
        In the place of ``from_step``: a FEED MASK (scheduled sampling), a bool / uint8 tensor or array of
        shape (B, T) -- image b runs step t on the fed-back prediction where it is set and on ``x`` where it is not; B <= 64.

        ``feedback_grad=True`` (with ``feedback``, on a training workspace): the window will be trained THROUGH the fed-back
        prediction.  It marks the workspace: ``backward(..., rollout=...)`` then runs the roll-out backward.
        The forward pass is the same one.  Without it a backward pass on a fed window is refused, as ever.

        ``residual``: False, or the number O of head outputs of a RESIDUAL HEAD -- the head predicts the
        increment, p_t = x_t[last O channels] + head(h_t) with x_t as the model saw it.  It marks the workspace: every head
        call on it (head_forward[_seq], the fused head / loss passes, the skill pass) then adds that base, and with
        ``feedback`` the fed value is round_ET(p_{t-1}) of that p (the _residual entries).  A fed image at step 0 is refused:
        p_{-1} has no base, even with a state.

        ``feedback_noise`` (with ``feedback``): an InputNoise whose ``std`` is one float or O floats
        -- every fed step stores round_ET(p + std[o] * z), z the input noise's normal of (pixel, o, step0 + t, lane0 + b).  It is
        one more field of the same feedback launches (nint_seq_fwd_stochastic).  None, all zeros or nothing fed: the entries and
        bits of the pass without it.  With ``feedback_grad=True`` the window is trained through the noisy
        feedback: z is a constant, so under the straight-through rule the roll-out backward of the noise-free window is its
        adjoint and runs as it stands."""
        B, T, Cc, H, W = x.shape
        assert (B, T, H, W) == (ws.B, ws.T, ws.H, ws.W) and Cc == self.cfgs[0].Cx
        s = ws.seq
        res_O = 0 if residual is False or residual is None else int(residual)
        if res_O and (not 1 <= res_O <= Cc or self._beyond_fused_head(self.layers[-1].Chp, res_O)):
            raise _lib.NintError(f"residual head: {res_O} outputs on {self.layers[-1].Chp} padded channels over {Cc} input channels is "
                                 "beyond the staged head kernels, which alone add the base (NINT_E_SHAPE), or has no feedback channels")
        ws.feedback.noise = None
        ws.feedback.set(res=bool(res_O))       # (stays as this pass sets it: a backward pass on a fed window is refused unless marked)
        if feedback is not None:
            w, b, from_step = feedback
            _, _, O, w2, b2 = self._head_args(w, b)
            mask = None
            if not isinstance(from_step, int) and getattr(from_step, "ndim", 0) > 0:         # (a 0-dim value is a step index)
                mask = Feedback.mask_bt(from_step, B, T)
                if B > 64:
                    raise _lib.NintError(f"feedback: a feed mask holds at most 64 images per step, got B = {B} (NINT_E_SHAPE)")
                from_step = Feedback.first_fed(mask)
            from_step = int(from_step)
            if w2.numel() != O * self.cfgs[-1].Ch or not 1 <= O <= Cc:      # (O, Ch) or the 1x1 conv's (O, Ch, 1, 1)
                raise ValueError(f"feedback: head weight {tuple(w.shape)} does not map {self.cfgs[-1].Ch} hidden channels onto "
                                 f"at most {Cc} input channels")
            if from_step < 0 or (from_step == 0 and not s.has_init_state):
                raise ValueError("feedback: step 0 can only be fed from a given initial state (from_step = 0 needs a state)")
            if res_O and from_step == 0:
                raise ValueError(RESIDUAL_STEP0)
            if res_O and res_O != O:
                raise ValueError(f"residual head: residual = {res_O} outputs, the fed-back head has {O}")
            if self._beyond_fused_head(self.layers[-1].Chp, O):
                raise _lib.NintError(f"feedback: a head of {O} outputs on {self.layers[-1].Chp} padded channels is beyond the "
                                     "staged head kernels (nint_head_feedback: NINT_E_SHAPE)")
            ws.feedback.set(w2, b2, O, from_step, bool(feedback_grad), mask, bool(res_O))
        if feedback_noise is not None and feedback_noise.active and feedback is not None:      # (nothing fed back: nothing to put it on)
            if feedback_noise.channels is not None:
                raise ValueError("feedback_noise: the noise goes onto the fed-back value of the closed loop -- its channels must be "
                                 "None (the feedback channels)")
            _, _, sig = feedback_noise.span(ws.feedback.fb.O, ws.feedback.fb.O)
            fn = NintFeedbackNoise()
            fn.sigma = self._sigma_tensor(sig).data_ptr()
            fn.seed, fn.draw, fn.step0, fn.lane0 = feedback_noise.seed, feedback_noise.draw, feedback_noise.step0, feedback_noise.lane0
            ws.feedback.noise = fn
        self.pack_input(ws, x)
        if noise is not None and noise.active:
            self.input_noise(ws, noise, ws.feedback.fb.O or res_O or None)
        if h0 is not None:
            self._write_state(h0, c0, self._slot_ptrs(ws, 0), B, ws.g, "0")
        self._set_wave(ws)
        self._seq_pass(ws, False)

    def input_noise(self, ws: Workspace, noise: InputNoise, feedback_O: Optional[int] = None):
        """One launch of nint_input_noise on the whole input slab of ``ws``: after the slab is filled, before
        the pass reads it.  The n sigmas live on the device, one small tensor per distinct value tuple for the engine's life."""
        cfg = self.cfgs[0]
        c0, n, sig = noise.span(cfg.Cx, feedback_O)
        sd = self._sigma_tensor(sig)
        check(self.lib.nint_input_noise(ptr(ws.xs), 0, ws.B, ws.T, cfg.Cx, ws.Cxp0, c0, n, ptr(sd), cfg.k if cfg.xfold else 0,
                                        int(self.lon_cyclic), noise.seed, noise.draw, noise.step0, noise.lane0, C.byref(ws.g),
                                        self.dt, stream_ptr()), "nint_input_noise")

    def _sigma_tensor(self, sig: Tuple[float, ...]) -> torch.Tensor:
        """the sigmas of a noise launch on the device: one small tensor per distinct value tuple for the engine's life"""
        sd = self._noise_sigma.get(sig)
        if sd is None:
            sd = self._noise_sigma[sig] = torch.tensor(sig, dtype=torch.float32, device=self.device)
        return sd

    def _seq_pass(self, ws: Workspace, bwd: bool, rg: Optional[NintFeedbackGrad] = None):
        """Choose and call the C entry of a whole-sequence pass: forward | backward, each open or (the last forward pass ran with
        a head) closed loop -- whose backward entry refuses every fed window --, and the roll-out backward (``rg``); the closed
        forward and the roll-out backward under a feed mask are the _sampled entries.  The one place in the package that names
        the seven."""
        s, fb, fm = ws.seq, ws.feedback.fb, ws.feedback.fm
        masked = ws.feedback.mask is not None and fb.O > 0
        if ws.feedback.noise is not None and fb.O > 0 and not bwd:          # noise on the fed-back value (4.24): one entry, forward only
            name, extra = "nint_seq_fwd_stochastic", (C.byref(fb), C.byref(fm), int(ws.feedback.res), C.byref(ws.feedback.noise))
        elif ws.feedback.res and fb.O > 0 and (rg is not None or not bwd):    # residual head (4.22): the _sampled entries' twins
            name = "nint_seq_bwd_rollout_residual" if rg is not None else "nint_seq_fwd_residual"
            extra = (C.byref(fb), C.byref(fm)) + ((C.byref(rg),) if rg is not None else ())
        elif rg is not None and masked:
            name, extra = "nint_seq_bwd_rollout_sampled", (C.byref(fb), C.byref(fm), C.byref(rg))
        elif rg is not None:
            name, extra = "nint_seq_bwd_rollout", (C.byref(fb), C.byref(rg))
        elif masked and not bwd:
            name, extra = "nint_seq_fwd_sampled", (C.byref(fb), C.byref(fm))
        elif fb.O > 0:
            name, extra = ("nint_seq_bwd_closed" if bwd else "nint_seq_fwd_closed"), (C.byref(fb),)
        else:
            name, extra = ("nint_seq_bwd" if bwd else "nint_seq_fwd"), ()
        what = name + (" (the backward pass of a window in which the prediction was fed back is not defined)" if bwd and extra and rg is None else "")
        # (seven names, the residual head's two and the stochastic forward)
        check(getattr(self.lib, name)(C.byref(s), *extra, stream_ptr()), what)

    def _set_wave(self, ws: Workspace):
        """nint_seq.wave: independent launches as one grid (a forward wavefront step; in BPTT the dgrad launches of layers 0 and 1
        and the bottom pointwise backward with the top layer's fused step).  FORCE_WAVE = None: wave = 5 for the smallest batches
        (B = 1 at 100 x 154: the layers' own tiles), wave = 4 (every forward layer on 8-row tiles) for everything above;
        an int: that mode (include/nint.h)."""
        tiles8 = ws.B * ((ws.W + 15) // 16) * ((ws.H + 7) // 8)
        if FORCE_WAVE is None:
            # round 4, six fresh processes per setting at B = 8 (profiles/r04_c_wave_repeats.txt): the forward wavefront as one
            # grid per step is 2.79-2.83 ms of forward against 2.87-2.94 in every process but one; the backward pair is neutral
            # (4.82-4.93 against 4.84-4.92 ms) with one slow process in six (5.01): that pair was the "bimodal" of round 3.
            # Three fresh processes per mode and batch (profiles/r04_d_wave_small_batches.txt): B = 1: mode 1 647 samples/s
            # against 586 (mode 2); B = 2: 833 against 841; B = 4: 957 against 966; B = 8: see above.
            # ... and from B = 2 the bottom layer's dgrad rides with layer 1's of the next BPTT step (wave = 4: B = 2 / 4 / 8
            # +3.2 / +1.2 / +0.4 % over wave = 2, every fresh-process pair but one of nine positive; B = 1: 601 against 665 of
            # wave = 1: profiles/r04_f_wave4.txt)
            # B = 1: the same BPTT pairs behind the forward wavefront on the layers' own tiles (wave = 5): 661 against 647 (wave = 1)
            # and 622 (wave = 4) samples/s
            # No upper end: B = 12 / 16 / 32 measure +1.0 ... +2.2 % with wave = 4 against the time-major order (forward -5 %,
            # backward neutral: profiles/r04_h_big_batches.txt); rounds 3-4 had stopped the rule at B = 8.
            mode = 5 if 2 * tiles8 < WAVE_TILES_PER_CU * self.n_cu else 4
        else:
            mode = int(FORCE_WAVE)
        ws.seq.wave = mode if len(self.cfgs) > 1 else 0

    def pack_input(self, ws: Workspace, x):
        """Fill the input slab ws.xs (image t*B+b, channels-last ET, folded for thin inputs) from x: a (B,T,C,H,W)
        f32 tensor (nint_pack_btchw[_xfold]) or a dataset.SlabBatch (the preproc kernel writes the slab directly)."""
        B, T, Cc, H, W = x.shape
        if hasattr(x, "fill_slab"):
            x.fill_slab(self, ws)
            return
        x = x.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        st, g = stream_ptr(), C.byref(ws.g)
        if self.cfgs[0].xfold:       # (cyclic longitude: the fold wraps by itself; a plain slab's halo is the forward pass's)
            name = "nint_pack_btchw_xfold_cyclic" if self.lon_cyclic else "nint_pack_btchw_xfold"
            check(getattr(self.lib, name)(ptr(x), ptr(ws.xs), B, T, Cc, self.cfgs[0].k, ws.Cxp0, g, self.dt, st), name)
        else:
            check(self.lib.nint_pack_btchw(ptr(x), ptr(ws.xs), B, T, Cc, ws.Cxp0, g, self.dt, st), "nint_pack_btchw")

    def h_last(self, ws: Workspace, l: int, slot: Optional[int] = None) -> torch.Tensor:
        return self._unpack_h(l, ws.h[l].data_ptr(), ws.B, ws.g, (ws.T if slot is None else slot) * ws.B)

    def c_last(self, ws: Workspace, l: int) -> torch.Tensor:
        return self._unpack_compact(l, ws.c_view(self, l, ws.T), ws.B, ws.g)

    def head_forward(self, ws: Workspace, w: torch.Tensor, b: Optional[torch.Tensor], slot: Optional[int] = None):
        """model.py:274: 1x1 conv on the last layer's hidden state of time step ``slot-1``."""
        Ch, Chp, O, w2, b2 = self._head_args(w, b)
        slot = ws.T if slot is None else slot
        pred = torch.empty(ws.B, O, ws.H, ws.W, dtype=torch.float32, device=self.device)
        if ws.feedback.res:             # residual head: + the feedback channels of the step's input, block slot - 1 of xs
            if slot < 1:
                raise ValueError("residual head: slot 0 is the initial state, which no input step pairs with")
            base = self._head_base(ws, O, (slot - 1) * ws.B)
            check(self.lib.nint_head_fwd_res(ptr(ws.h[-1]), slot * ws.B, ws.B, Ch, Chp, O, ptr(w2), ptr(b2), ptr(pred),
                                             C.byref(ws.g), self.dt, C.byref(base), stream_ptr()), "nint_head_fwd_res")
            return pred
        check(self.lib.nint_head_fwd(ptr(ws.h[-1]), slot * ws.B, ws.B, Ch, Chp, O, ptr(w2), ptr(b2), ptr(pred),
                                     C.byref(ws.g), self.dt, stream_ptr()), "nint_head_fwd")
        return pred

    def _head_base(self, ws: Workspace, O: int, x_n0: int) -> NintHeadBase:
        """nint_head_base of a workspace's input slab: image ``x_n0`` pairs with the head call's first image; the feedback
        channels are the last O of layer 0's input"""
        cfg = self.cfgs[0]
        if not 1 <= O <= cfg.Cx:
            raise ValueError(f"residual head: {O} outputs do not fit the {cfg.Cx} input channels")
        hb = NintHeadBase()
        hb.xs, hb.x_n0, hb.Cx, hb.Cxp, hb.c0, hb.xfold_k = ws.xs.data_ptr(), int(x_n0), cfg.Cx, ws.Cxp0, cfg.Cx - O, cfg.k if cfg.xfold else 0
        return hb

    _DEFAULT_SPEC = None

    @classmethod
    def _default_spec(cls) -> NintLossSpec:
        """the spec (1, 1, 0) without output weights: the bits of the plain and _weighted loss entries (include/nint.h), for
        the residual fused passes, which exist as twins of the _spec entries only"""
        if cls._DEFAULT_SPEC is None:
            c = NintLossSpec()
            c.mse, c.l1, c.huber, c.delta, c.ow, c.now, c.osum = 1.0, 1.0, 0.0, 1.0, None, 0, 0.0
            cls._DEFAULT_SPEC = c
        return cls._DEFAULT_SPEC

    def _head_args(self, w: torch.Tensor, b: Optional[torch.Tensor]):
        cfg = self.cfgs[-1]
        w2 = w.detach().float().contiguous()
        b2 = None if b is None else b.detach().float().contiguous()
        return cfg.Ch, self.layers[-1].Chp, w.shape[0], w2, b2

    @staticmethod
    def _beyond_fused_head(Chp: int, O: int) -> bool:
        """The fused head/loss kernels' limit: more than 128 padded channels, or the weights [O][CHV] plus one output chunk's
        d loss / d pred of 64 pixels (and 8 KiB of static LDS) beyond the 160 KiB of a CU.  The same rule (head_staged_holds in
        csrc/head.hip) keeps nint_head_fwd / nint_head_bwd on their staged kernels, so the fallback of a shape the fused
        kernels hold would give the same bits."""
        chv = 32 if Chp <= 32 else (64 if Chp <= 64 else 128)
        return Chp > 128 or (O * chv + min(O, 64) * 64) * 4 + 8192 > 160 * 1024

    def head_forward_seq(self, ws: Workspace, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
        """The head on the top layer's hidden state of EVERY step in one launch (nint_head_fwd_seq): (B, T*O, H, W), channel
        t*O + o -- torch.cat of the per-step outputs (model.py:264,272,274 commented code)."""
        Ch, Chp, O, w2, b2 = self._head_args(w, b)
        seq = torch.empty(ws.B, ws.T * O, ws.H, ws.W, dtype=torch.float32, device=self.device)
        if ws.feedback.res:             # residual head: step t's output + the feedback channels of block t of xs
            base = self._head_base(ws, O, 0)
            check(self.lib.nint_head_fwd_seq_res(ptr(ws.h[-1]), ws.B, ws.T, Ch, Chp, O, ptr(w2), ptr(b2), ptr(seq), C.byref(ws.g),
                                                 self.dt, C.byref(base), stream_ptr()), "nint_head_fwd_seq_res")
            return seq
        check(self.lib.nint_head_fwd_seq(ptr(ws.h[-1]), ws.B, ws.T, Ch, Chp, O, ptr(w2), ptr(b2), ptr(seq), C.byref(ws.g),
                                         self.dt, stream_ptr()), "nint_head_fwd_seq")
        return seq

    def head_backward_seq(self, ws: Workspace, w: torch.Tensor, dseq: Optional[torch.Tensor], dpred: Optional[torch.Tensor] = None,
                          dw_out=None, db_out=None, write_dh: bool = True, accumulate: bool = False):
        """Head backward over every step (nint_head_bwd_seq): dseq (B, T*O, H, W) and / or dpred (B, O, H, W), the cotangent
        of pred = head(h_{T-1}), which joins step T-1.  Writes the per-step dL/dh into ws.dh_seq_slab() (unless `write_dh` is
        False) for backward(..., seq_grads=True); returns (dw_head, db_head).  ``accumulate``: as in head_backward."""
        Ch, Chp, O, w2, dw, db = self._head_bwd_args(w, dw_out, db_out, accumulate)
        ds = None if dseq is None else dseq.detach().float().contiguous()
        dp = None if dpred is None else dpred.detach().float().contiguous()
        check(self.lib.nint_head_bwd_seq_acc(ptr(ws.h[-1]), ws.B, ws.T, Ch, Chp, O, ptr(w2), ptr(ds), ptr(dp),
                                             ptr(ws.dh_seq_slab(self)) if write_dh else None, ptr(dw), ptr(db), int(accumulate),
                                             C.byref(ws.g), self.dt, ptr(self.wg_partial), self.wg_partial.numel() * 4, stream_ptr()),
              "nint_head_bwd_seq_acc")
        return dw.view(O, Ch, 1, 1), db

    def _loss_entry(self, seq: bool, weights, spec):
        """The fused head + loss entry of (one step | every step) x (plain | weight map | spec): the C function, its name
        for `check`, and the arguments between `y` and `dpred`.  The one place that chooses among the six."""
        stem = "nint_head_loss_seq_fused" if seq else "nint_head_loss_fused"
        wgt, wsum = weights if weights is not None else (None, 0.0)
        if spec is not None:
            name, extra = stem + "_spec", (ptr(wgt), wsum, C.byref(spec))
        elif weights is not None:
            name, extra = stem + "_weighted", (ptr(wgt), wsum)
        else:
            name, extra = stem, ()
        return getattr(self.lib, name), name, extra

    def _head_loss(self, seq: bool, ws, w, b, y, dpred, scratch, stats, halo, Hc, Wc, weights, spec) -> bool:
        """the body of head_loss_fused (the last step's B images, dL/dh into ws.dh[-1]) and head_loss_seq_fused (every
        step's, dL/dh into ws.dh_seq_slab())"""
        Ch, Chp, O, w2, b2 = self._head_args(w, b)
        if self._beyond_fused_head(Chp, O):
            return False
        n0, N, dh = (ws.B, ws.T, ws.dh_seq_slab(self)) if seq else (ws.T * ws.B, ws.B, ws.dh[-1])
        if ws.feedback.res:
            # residual head: the _res twin of the _spec entry (the default spec gives the plain / weighted entries' bits);
            # `scratch` holds NINT_LOSS_SPEC_SCRATCH_FLOATS floats then
            if scratch.numel() < _lib.NINT_LOSS_SPEC_SCRATCH_FLOATS:
                raise ValueError("residual head: the fused head / loss pass needs a scratch of NINT_LOSS_SPEC_SCRATCH_FLOATS floats")
            name = "nint_head_loss_seq_fused_res" if seq else "nint_head_loss_fused_res"
            wgt, wsum = weights if weights is not None else (None, 0.0)
            sp = spec if spec is not None else self._default_spec()
            base = self._head_base(ws, O, 0 if seq else (ws.T - 1) * ws.B)
            check(getattr(self.lib, name)(ptr(ws.h[-1]), n0, N, Ch, Chp, O, ptr(w2), ptr(b2), ptr(y), ptr(wgt), wsum, C.byref(sp),
                                          ptr(dpred), ptr(dh), ptr(scratch), ptr(stats), C.byref(ws.g), halo[0], halo[1], Hc, Wc,
                                          self.dt, C.byref(base), stream_ptr()), name)
            return True
        fn, name, extra = self._loss_entry(seq, weights, spec)
        check(fn(ptr(ws.h[-1]), n0, N, Ch, Chp, O, ptr(w2), ptr(b2), ptr(y), *extra, ptr(dpred), ptr(dh),
                 ptr(scratch), ptr(stats), C.byref(ws.g), halo[0], halo[1], Hc, Wc, self.dt, stream_ptr()), name)
        return True

    def head_loss_seq_fused(self, ws: Workspace, w: torch.Tensor, b: Optional[torch.Tensor], y: torch.Tensor, dpred: torch.Tensor,
                            scratch: torch.Tensor, stats: torch.Tensor, halo, Hc: int, Wc: int, weights=None, spec=None) -> bool:
        """head_loss_fused over every step (nint_head_loss_seq_fused): y (B, T, O, Hc, Wc); dpred (T*B, O, H, W) in image
        order t*B + b; the per-step dL/dh goes into ws.dh_seq_slab().  False beyond the fused kernel's limit.  `weights`,
        `spec` (its weights run over t*O + o): as in head_loss_fused."""
        return self._head_loss(True, ws, w, b, y, dpred, scratch, stats, halo, Hc, Wc, weights, spec)

    def head_loss_fused(self, ws: Workspace, w: torch.Tensor, b: Optional[torch.Tensor], y: torch.Tensor, dpred: torch.Tensor,
                        scratch: torch.Tensor, stats: torch.Tensor, halo, Hc: int, Wc: int, weights=None, spec=None) -> bool:
        """Training fast path (nint_head_loss_fused): head forward, crop, MSE+L1 sums, d loss / d pred and dL/dh_{T-1}
        (into ws.dh[-1]) in one pass; `scratch[0]` = loss, `stats` accumulated.  False when the head is wider than the
        fused kernel holds (more than 128 padded channels, or weights + one pixel group's d loss / d pred beyond the LDS) (the caller then takes the three separate launches).
        `weights` = (wgt, wsum): the f32 (Hc, Wc) device map and its f64 sum (nint_head_loss_fused_weighted); None: unweighted.
        `spec`: a _lib.NintLossSpec (loss.LossSpec.on) -- the configurable loss, nint_head_loss_fused_spec with or without the
        map, `scratch` then of NINT_LOSS_SPEC_SCRATCH_FLOATS floats; None: the calls above."""
        return self._head_loss(False, ws, w, b, y, dpred, scratch, stats, halo, Hc, Wc, weights, spec)

    def head_skill(self, ws: Workspace, w: torch.Tensor, b: Optional[torch.Tensor], y: torch.Tensor, slots, acc,
                   pred_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Evaluation fast path (nint_head_skill_accum): the head on the last step's images, the crop and the f64 skill sums
        in one pass -- `acc` (an inference.SkillAccumulator: pix, scratch, row weights, crop offset) gains the batch's terms
        in the slots `slots` (a host sequence of ws.B ints, -1 = out of the maps; None = all 0); the prediction goes to memory
        only when `pred_out` (B, O, Hc, Wc) f32 is given.  Returns the batch's (B, O, NINT_SKILL_SAMPLE) f64 sample rows.
        A head beyond the fused kernels' limit (_beyond_fused_head) runs as head_forward + nint_skill_accum: the same sums."""
        Ch, Chp, O, w2, b2 = self._head_args(w, b)
        B, Hc, Wc = ws.B, acc.Hc, acc.Wc
        oy, ox = acc.halo if acc.halo is not None else ((ws.H - Hc) // 2, (ws.W - Wc) // 2)
        yv = y.detach().float().contiguous()
        assert O == acc.O and yv.numel() == B * O * Hc * Wc, "target must be (B,[O,]Hc,Wc)"
        assert pred_out is None or (pred_out.dtype == torch.float32 and pred_out.is_contiguous() and pred_out.numel() == yv.numel())
        sl = None if slots is None else (C.c_int32 * B)(*[int(v) for v in slots])
        sample = torch.empty(B, O, _lib.NINT_SKILL_SAMPLE, dtype=torch.float64, device=self.device)
        scratch = acc.scratch_for(B)
        if self._beyond_fused_head(Chp, O) or ws.feedback.res:       # (residual head: nint_head_fwd_res + nint_skill_accum, no fused twin)
            pred = self.head_forward(ws, w, b)
            check(self.lib.nint_skill_accum(ptr(pred), ptr(yv), sl, acc.nslots, ptr(acc.row_w), ptr(acc.pix), ptr(sample),
                                            ptr(scratch), scratch.numel() * 8, B, O, ws.H, ws.W, oy, ox, Hc, Wc, stream_ptr()),
                  "nint_skill_accum")
            if pred_out is not None:
                pred_out.view(B, O, Hc, Wc).copy_(pred[:, :, oy:oy + Hc, ox:ox + Wc])
            return sample
        check(self.lib.nint_head_skill_accum(ptr(ws.h[-1]), ws.T * B, B, Ch, Chp, O, ptr(w2), ptr(b2), ptr(yv), sl, acc.nslots,
                                             ptr(acc.row_w), ptr(acc.pix), ptr(sample), ptr(pred_out), ptr(scratch),
                                             scratch.numel() * 8, C.byref(ws.g), oy, ox, Hc, Wc, self.dt, stream_ptr()),
              "nint_head_skill_accum")
        return sample

    @staticmethod
    def _check_accumulate(accumulate, *outs):
        if accumulate and any(o is None for o in outs):
            raise ValueError("accumulate=True adds to the destinations: pass them (dW_out / db_out, dw_out / db_out)")

    def _head_bwd_args(self, w: torch.Tensor, dw_out, db_out, accumulate: bool):
        """what both head backward entries start with: the accumulate check, the head's geometry and f32 weights, and the
        gradient destinations (the caller's, or new ones)"""
        self._check_accumulate(accumulate, dw_out, db_out)
        Ch, Chp, O, w2, _ = self._head_args(w, None)
        dw = dw_out if dw_out is not None else torch.empty(O, Ch, dtype=torch.float32, device=self.device)
        db = db_out if db_out is not None else torch.empty(O, dtype=torch.float32, device=self.device)
        return Ch, Chp, O, w2, dw, db

    def head_backward(self, ws: Workspace, w: torch.Tensor, dpred: torch.Tensor, dw_out=None, db_out=None, write_dh: bool = True,
                      images: Optional[Tuple[int, int]] = None, accumulate: bool = False):
        """Writes dL/dh_{T-1} of the last layer into ws.dh[-1] (unless `write_dh` is False: the fused head/loss pass
        already did); returns (dw_head, db_head).  `images` = (first image, count) of the h slab that `dpred` (count, O, H, W)
        belongs to: default the last step's B; (B, T*B) reduces every step's (the fused sequence pass, write_dh False).
        ``accumulate`` (nint_head_bwd_acc): dw_out / db_out (required then) receive old + gradient, one f32 add per element,
        instead of being overwritten -- the micro-batches of one optimizer step sum into the bucket."""
        Ch, Chp, O, w2, dw, db = self._head_bwd_args(w, dw_out, db_out, accumulate)
        n0, N = images if images is not None else (ws.T * ws.B, ws.B)
        assert images is None or not write_dh
        dp = dpred.detach().float().contiguous()
        check(self.lib.nint_head_bwd_acc(ptr(ws.h[-1]), n0, N, Ch, Chp, O, ptr(w2), ptr(dp),
                                         ptr(ws.dh[-1]) if write_dh else None,
                                         ptr(dw), ptr(db), int(accumulate), C.byref(ws.g), self.dt, ptr(self.wg_partial),
                                         self.wg_partial.numel() * 4, stream_ptr()), "nint_head_bwd_acc")
        return dw.view(O, Ch, 1, 1), db

    def rollout_cotangents(self, ws: Workspace, w: torch.Tensor, dseq: Optional[torch.Tensor] = None,
                           dpred: Optional[torch.Tensor] = None, slab_filled: bool = False, dh_written: bool = False) -> torch.Tensor:
        """What the roll-out backward starts from (the roll-out entry's contract, include/nint.h), for a workspace whose forward pass
        was marked ``feedback_grad``: the slab ``ws.rollout_dpred`` filled with l_t -- ``dseq`` (B, T*O, H, W) and / or
        ``dpred`` (B, O, H, W), which joins step T-1; zeros where there is neither -- and W^T l_t in the blocks of
        ``ws.dh_seq_slab`` that the chain itself does not write (t < F-1 and t = T-1; nint_head_bwd_acc, dh only).
        ``slab_filled``: the caller has written l_t into the slab (the fused head / loss passes take it as their dpred);
        ``dh_written``: ... and every block of dh_seq holds W^T l_t (head_loss_seq_fused).  Returns the slab."""
        Ch, Chp, O, w2, _ = self._head_args(w, None)
        B, T, F = ws.B, ws.T, ws.feedback.fed.start
        slab = ws.rollout_dpred(self, O)
        if not slab_filled:
            v = slab.view(T, B, O, ws.H, ws.W)
            if dseq is not None:
                v.copy_(dseq.detach().reshape(B, T, O, ws.H, ws.W).transpose(0, 1))
            else:
                v.zero_()
            if dpred is not None:
                v[T - 1] += dpred.detach()
        if dh_written:
            return slab
        dh_seq = ws.dh_seq_slab(self)
        blk = B * ws.H * ws.W * Chp * self.es
        for t0, t1 in ((0, max(F - 1, 0)), (T - 1, T)):         # images [t0*B, t1*B) of the slab -> the same blocks of dh_seq
            if t1 > t0:
                check(self.lib.nint_head_bwd_acc(ptr(ws.h[-1]), (t0 + 1) * B, (t1 - t0) * B, Ch, Chp, O, ptr(w2), slab[t0 * B:].data_ptr(),
                                                 dh_seq.data_ptr() + t0 * blk, None, None, 0, C.byref(ws.g), self.dt, None, 0,
                                                 stream_ptr()), "nint_head_bwd_acc (dh of the unfed steps)")
        return slab

    def ens_loss(self, ws: Workspace, seq: torch.Tensor, y: torch.Tensor, slab: torch.Tensor, M: int, spec, weights, scratch: torch.Tensor,
                 loss_out: torch.Tensor, stats: torch.Tensor, ens_out: torch.Tensor, halo, Hc: int, Wc: int, every_step: bool = False):
        """The almost-fair CRPS over the member lanes of a roll-out window (nint_ens_loss): ``seq`` is
        head_forward_seq's (B, T*O, H, W) with lanes n*M + m, read in place; d loss / d pred of every member goes into the
        roll-out slab ``slab`` (T*B, O, H, W), image t*B + n*M + m, in place.  ``y``: (N, O, Hc, Wc), the last step's targets, or
        with ``every_step`` (N, T, O, Hc, Wc) -- sample (n, t) then takes row t of the output-weight table.  ``spec``
        (loss.EnsembleLoss.on): ``alpha``, and ``ow`` (device f32 (rows, O)) with its host copy ``ow_host`` (numpy f32, the same
        values: cnt is formed from it here), or both None: all ones.  ``weights`` = (wgt, wsum) as in head_loss_fused, or None.  Without ``every_step`` the images of the steps before the last are NOT
        written: the caller zeroes them.  ``scratch``: f64, at least ens_loss_scratch(...) elements.  No host sync."""
        B, T, H, W = ws.B, ws.T, ws.H, ws.W
        O = slab.shape[1]
        if M < 2 or B % M:
            raise ValueError(f"ens_loss: {B} lanes do not hold whole ensembles of {M} members")
        N, img = B // M, O * H * W
        steps = range(T) if every_step else (T - 1,)
        pairs = [(n, t) for n in range(N) for t in steps]               # y's own order: (N, [T,] O, Hc, Wc) is read in place
        ns = len(pairs)
        assert y.dtype == torch.float32 and y.is_contiguous() and y.numel() == ns * O * Hc * Wc
        assert seq.dtype == torch.float32 and seq.is_contiguous() and seq.numel() == B * T * img and slab.numel() == T * B * img
        poff = (C.c_int64 * ns)(*[((n * M) * T + t) * img for n, t in pairs])
        doff = (C.c_int64 * ns)(*[(t * B + n * M) * img for n, t in pairs])
        wgt, wsum = weights if weights is not None else (None, 0.0)
        sp = _lib.NintEnsLossSpec()
        sp.alpha = float(spec.alpha)
        ow, ow_host, rows = spec.ow, spec.ow_host, None
        if ow is not None:
            nrows = ow.shape[0]
            if every_step and nrows != T or not every_step and nrows != 1:
                raise ValueError(f"ens_loss: {nrows} rows of output weights for {'a window of %d steps' % T if every_step else 'the last step'}")
            rows = (C.c_int32 * ns)(*[t if every_step else 0 for _, t in pairs])
            q64 = ow_host.astype("float64")
            qsum = float(sum(float(q64[r].sum()) for r in rows))
            sp.ow, sp.ow_row, sp.nrows = ow.data_ptr(), rows, nrows
        else:
            qsum = float(ns) * float(O)
            sp.ow, sp.ow_row, sp.nrows = None, None, 0
        sp.cnt = qsum * (wsum if weights is not None else float(Hc) * float(Wc))
        nb = self.lib.nint_ens_loss_scratch_bytes(ns, M, O, H, W)
        if scratch.dtype != torch.float64 or scratch.numel() * 8 < nb:
            raise ValueError("ens_loss: the scratch is smaller than nint_ens_loss_scratch_bytes")
        check(self.lib.nint_ens_loss(ptr(seq), poff, T * img, ptr(slab), doff, img, M, ptr(y), ptr(wgt), wsum, C.byref(sp), ptr(loss_out),
                                     ptr(stats), ptr(ens_out), ptr(scratch), nb, ns, O, H, W, halo[0], halo[1], Hc, Wc, stream_ptr()),
              "nint_ens_loss")

    def ens_loss_scratch(self, N: int, M: int, O: int, H: int, W: int) -> int:
        """f64 elements of nint_ens_loss's scratch for N samples (host arithmetic)"""
        return self.lib.nint_ens_loss_scratch_bytes(N, M, O, H, W) // 8

    def backward(self, ws: Workspace, need_dx: bool, zero_state_grads: Sequence[int] = (),
                 dW_out: Optional[Sequence[torch.Tensor]] = None, db_out: Optional[Sequence[torch.Tensor]] = None, parts: int = 0,
                 seq_grads: bool = False, zero_mask: Optional[int] = None, accumulate: bool = False, train_from: int = 0,
                 rollout: Optional[torch.Tensor] = None):
        """BPTT of model.py:253-271.  Precondition: ws.dh[l], ws.dc[l] hold dL/dh_{T-1}, dL/dc_{T-1}
        (layers listed in ``zero_state_grads`` start from zero state gradients instead).  Returns ([dW_l], [db_l], dx or None).
        ``dW_out`` / ``db_out``: f32 contiguous destinations (e.g. views of a flat gradient bucket).
        ``parts`` (nint_seq.bwd_parts): 0 = everything; 1 = the BPTT chain + the gradients of layers >= 1; 2 = layer 0's weight /
        bias gradient only, after a parts = 1 call on the same workspace (the trainer starts the all-reduce of the rest of the
        bucket in between).
        ``seq_grads`` (nint_seq.dh_seq): the top layer's dL/dh_t of every step is in ws.dh_seq_slab() (head_backward_seq /
        head_loss_seq_fused) and joins the recurrence at each t; ws.dh[-1] is then not read on entry.
        ``accumulate`` (nint_seq.accumulate): every dW / db element this call produces is written as old + gradient (one f32
        add by the element's one writer, bitwise reproducible) into ``dW_out`` / ``db_out``, which are required then.  With
        ``zero_state_grads=()`` on a has_init workspace, ws.dh[l] / ws.dc[l] as the previous call left them are the entry
        gradients: a window runs as segments, last to first, through ONE workspace and sums into one bucket (trainer.py).
        ``train_from`` (nint_seq.train_from): layers below it are frozen -- BPTT stops above them, their ``dW_out`` / ``db_out``
        entries are not touched (they may be None) and their slots of the returned lists hold None.  The workspace must have
        been acquired with a ``train_from`` no larger.  Not with ``need_dx`` or ``parts``; ``train_from == L``: no library call.
        ``rollout`` (a workspace whose forward pass was marked ``feedback_grad``): the slab that
        ``rollout_cotangents`` returned.  BPTT then runs through the fed-back prediction (the roll-out entry, ``seq_grads``
        implied); on return the slab holds g_t, which ``head_backward(images=(B, T*B), write_dh=False)`` reduces to the
        head's gradients.  The returned dx is zero on the fed channels of the fed steps (under a feed mask: of the fed images
        of each step) -- the forward pass overwrote them.  On a residual-head workspace the roll-out entry is
        the _residual one, and the returned dx carries + g_t on the feedback channels of every unfed (t, b): d p_t / d x_t = 1
        there.  (A residual window in which nothing was fed has no slab: its caller adds the head cotangents, add_skip_dx.)"""
        assert ws.train
        fed = bool(ws.feedback.fed)
        if rollout is not None and not ws.feedback.grad:
            raise ValueError("backward(rollout=...) needs a forward pass with feedback=..., feedback_grad=True on this workspace")
        if ws.feedback.grad and fed and rollout is None:
            raise ValueError("backward: this window was run with feedback_grad=True: pass rollout=rollout_cotangents(...)")
        rollout = rollout if fed else None               # (nothing was fed back: the window trains as ever)
        L = len(self.cfgs)
        train_from = int(train_from)
        if not 0 <= train_from <= L:
            raise ValueError(f"train_from must be in [0, {L}], got {train_from}")
        if train_from > 0 and need_dx:
            raise _lib.NintError("backward: need_dx with train_from > 0 is not supported (the input's gradient passes through every layer)")
        if train_from > 0 and parts:
            raise _lib.NintError("backward: parts with train_from > 0 is not supported (the two-piece exchange is defined around layer 0's slice)")
        if train_from < ws.train_from:
            raise _lib.NintError(f"backward: train_from = {train_from} on a workspace acquired with train_from = {ws.train_from}: "
                                 f"layers {train_from} .. {ws.train_from - 1} have no stash")
        self._check_accumulate(accumulate, dW_out, db_out)
        # layers in ``zero_state_grads`` start BPTT from zero dL/dh, dL/dc: flagged, not filled (the first BPTT step
        # then neither reads dc nor accumulates into dh).  The top layer's dh always holds the head's gradient.
        mask = 0
        for l in zero_state_grads:
            mask |= 1 << (2 * l)
            if l < L - 1:
                mask |= 1 << (2 * l + 1)
        # ``zero_mask``: nint_seq.zero_dstate itself, where h and c of a layer differ (a returned state with one cotangent missing)
        ws.seq.zero_dstate = mask if zero_mask is None else int(zero_mask)
        dWs, dbs = [], []
        s = ws.seq
        for l, cfg in enumerate(self.cfgs):
            if l < train_from:
                dWs.append(None)
                dbs.append(None)
                s.dW[l] = s.db[l] = None
                continue
            if dW_out is not None:
                dWs.append(dW_out[l])
                dbs.append(db_out[l])
                assert dWs[-1].numel() == 4 * cfg.Ch * (cfg.Cx + cfg.Ch) * cfg.k * cfg.k and dWs[-1].is_contiguous()
            else:
                dWs.append(torch.empty(4 * cfg.Ch, cfg.Cx + cfg.Ch, cfg.k, cfg.k, dtype=torch.float32, device=self.device))
                dbs.append(torch.empty(4 * cfg.Ch, dtype=torch.float32, device=self.device))
            s.dW[l] = dWs[-1].data_ptr()
            s.db[l] = dbs[-1].data_ptr()
        dx = torch.empty(ws.T * ws.B * ws.H * ws.W * ws.Cxp0 * self.es, dtype=torch.uint8, device=self.device) if need_dx else None
        rg = None
        if rollout is not None:
            rg = NintFeedbackGrad()
            rg.dpred = rollout.data_ptr()
            if not need_dx:
                if ws.feedback.dx_step is None:
                    ws.feedback.dx_step = torch.empty(ws.B * ws.H * ws.W * ws.Cxp0 * self.es, dtype=torch.uint8, device=self.device)
                rg.dx_step = ws.feedback.dx_step.data_ptr()
        dh_seq = ws.dh_seq_slab(self) if seq_grads or rg is not None else None
        with self._bwd_fields(s, dx, need_dx, parts, dh_seq, accumulate, train_from):
            if rg is not None or ws.feedback.fb.O > 0 or train_from < L:
                self._seq_pass(ws, True, rg)
        dx_out = None
        if need_dx:                     # compact [T*B][H][W][Cxp0] -> (B,T,C,H,W)
            C0 = self.cfgs[0].Cx
            tb = torch.empty(ws.T * ws.B, C0, ws.H, ws.W, dtype=torch.float32, device=self.device)
            if self.cfgs[0].xfold:     # gradient of the folded input -> gradient of the input
                name = "nint_unfold_dx_cyclic" if self.lon_cyclic else "nint_unfold_dx"
                check(getattr(self.lib, name)(ptr(dx), ptr(tb), ws.T * ws.B, C0, self.cfgs[0].k, ws.Cxp0, ws.H, ws.W, self.dt,
                                              stream_ptr()), name)
            else:
                check(self.lib.nint_unpack_compact(ptr(dx), ptr(tb), ws.T * ws.B, C0, ws.Cxp0, ws.H, ws.W, self.dt, stream_ptr()),
                      "unpack dx")
            dx_out = tb.view(ws.T, ws.B, C0, ws.H, ws.W).transpose(0, 1).contiguous()
            if rg is not None and ws.feedback.res:      # residual head: the skip path into the input, g_t from the slab
                self.add_skip_dx(dx_out, ws.fb.O, slab=rollout)
            if rg is not None:              # the caller's x never reached those channels
                if ws.feedback.mask is not None:
                    m = ws.feedback.fed_mask.to(self.device)        # (T*B bytes, a plain copy: the pinned buffer is the next pass's)
                    dx_out[:, :, C0 - ws.fb.O:].masked_fill_(m.view(ws.B, ws.T, 1, 1, 1), 0)
                else:
                    dx_out[:, ws.feedback.fed.start:, C0 - ws.fb.O:] = 0
        return dWs, dbs, dx_out

    @staticmethod
    def add_skip_dx(dx: torch.Tensor, O: int, slab: Optional[torch.Tensor] = None, dseq: Optional[torch.Tensor] = None,
                    dpred: Optional[torch.Tensor] = None):
        """Residual head: d p_t / d x_t[feedback channels] = 1, so the input gradient ``dx`` (B, T, C, H, W) gains the total
        cotangent of p_t on its last O channels -- from the roll-out slab (T*B, O, H, W), image t*B + b, which came back
        holding g_t, or from the cotangents of a window in which nothing was fed: ``dseq`` (B, T*O, H, W) and / or ``dpred``
        (B, O, H, W), which joins step T-1.  A boundary operation on the result, in place; the caller zeroes the fed (t, b)."""
        B, T, C0, H, W = dx.shape
        fbc = dx[:, :, C0 - O:]
        if slab is not None:
            fbc += slab.view(T, B, O, H, W).transpose(0, 1)
        if dseq is not None:
            fbc += dseq.detach().reshape(B, T, O, H, W)
        if dpred is not None:
            fbc[:, T - 1] += dpred.detach().reshape(B, O, H, W)

    @staticmethod
    @contextlib.contextmanager
    def _bwd_fields(s: NintSeq, dx, need_dx, parts, dh_seq, accumulate, train_from):
        """the nint_seq fields of ONE backward call: set for the body; bwd_parts, dh_seq, accumulate and train_from put back
        whatever happens, dx once the call has returned (need_dx stays: every call sets its own)"""
        if dx is not None:
            s.dx = dx.data_ptr()
        s.need_dx, s.bwd_parts, s.accumulate, s.train_from = int(need_dx), int(parts), int(bool(accumulate)), train_from
        s.dh_seq = None if dh_seq is None else dh_seq.data_ptr()
        try:
            yield
        finally:
            s.bwd_parts, s.dh_seq, s.accumulate, s.train_from = 0, None, 0, 0
        s.dx = None

    def rollout_head_backward(self, ws: Workspace, w: torch.Tensor, slab: torch.Tensor, dw_out=None, db_out=None, accumulate: bool = False):
        """the end of a roll-out: the slab came back from ``backward(rollout=slab)`` holding g_t; (dw_head, db_head) from it"""
        return self.head_backward(ws, w, slab, dw_out, db_out, write_dh=False, images=(ws.B, ws.T * ws.B), accumulate=accumulate)

    def state_grads(self, ws: Workspace, l: int):
        """dL/dh_init, dL/dc_init of layer l after backward (has_init_state workspaces)."""
        return (self._unpack_compact(l, ws.dh[l].data_ptr(), ws.B, ws.g, True, "unpack dh"),
                self._unpack_compact(l, ws.dc[l].data_ptr(), ws.B, ws.g, False, "unpack dc"))

    def set_state_grads(self, ws: Workspace, l: int, dh: Optional[torch.Tensor], dc: Optional[torch.Tensor]):
        self.set_dstate(ws, l, "h", dh)
        self.set_dstate(ws, l, "c", dc)

    def set_dstate(self, ws: Workspace, l: int, which: str, t: Optional[torch.Tensor]):
        """one cotangent of a returned final state, (B, Ch, H, W), into ws.dh[l] (which = "h") or ws.dc[l] ("c"); None: a
        zero fill of that slab"""
        dst = ws.dh[l] if which == "h" else ws.dc[l]
        if t is None:
            dst.zero_()
        else:
            self._pack_compact(l, t, dst.data_ptr(), ws.B, ws.g, which == "h", "pack dstate")

    def add_top_dh(self, ws: Workspace, dh: torch.Tensor, seq_grads: bool):
        """the top layer's returned h_{T-1} has a cotangent of its own: added to the head's dL/dh_{T-1} where BPTT reads it --
        ws.dh[-1], or the last block of ws.dh_seq_slab() with per-step head gradients (nint_pack_compact_add)"""
        if seq_grads:
            dst = ws.dh_seq_slab(self).data_ptr() + (ws.T - 1) * ws.B * ws.H * ws.W * self.layers[-1].Chp * self.es
        else:
            dst = ws.dh[-1].data_ptr()
        self._pack_compact(len(self.cfgs) - 1, dh, dst, ws.B, ws.g, True, "nint_pack_compact_add", add=True)
