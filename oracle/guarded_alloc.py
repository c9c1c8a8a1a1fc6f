"""A guarded, poisoning allocator for tests and tools: where a kernel writes, and what it may read.

The suite's other checks look inside the buffers they hand to the library.  This helper looks around them and before them:

  * every intercepted allocation is the middle of one ``uint8`` arena, ``front + nbytes + back`` bytes, whose two guards hold
    a known byte.  ``verify()`` compares every guard byte afterwards: a store before a buffer's start or behind its end is
    named with its allocation's call site, instead of silently landing in a neighbour tensor of the caching allocator;
  * ``empty`` / ``empty_like`` payloads (and the guards) are filled with 0x00 (``mode="zero"``) or 0xFF (``mode="poison"``:
    NaN in bf16, f32 and f64, -1 in an int32).  A result that is bit-identical in both modes depends on no byte the library
    did not write itself, inside the buffer or behind its end.

Plain torch only; the library is never touched.  ``patched`` swaps the ``torch`` name of the package's modules for a
``GuardedTorch`` proxy, so engines, workspaces, trainers and accumulators built (and first used: much is allocated lazily)
inside the context allocate through it.  Nothing else changes: tensors made by torch ops (``.to``, ``.clone``, ``.contiguous``,
``torch.cat``, ``from_numpy``) are written in full by torch and are only read by the library; they pass through.
"""
from __future__ import annotations

import contextlib
import importlib
import math
import os
import sys
from typing import List, Optional, Sequence

import torch as _torch

PAGE = 4096
MIN_GUARD = 64 * 1024
FILL = {"zero": 0x00, "poison": 0xFF}
PACKAGE = "nasa_niswan_amd"
# every module of the package that allocates device memory does `import torch`
MODULES = ("engine", "model", "loss", "optim", "trainer", "inference", "dataset", "utils")
_HERE = os.path.abspath(__file__)


class GuardError(AssertionError):
    pass


def guard_bytes(row_stride: int = 0) -> int:
    """max(64 KiB, 4 x the largest row stride Wh * Cp * es of the scenario), rounded up to a whole page: a stray tile row
    lands inside the guard, not behind it"""
    need = max(MIN_GUARD, 4 * int(row_stride))
    return (need + PAGE - 1) // PAGE * PAGE


def _call_site() -> str:
    """file:line of the nearest frame outside this file: where the package (or the test) asked for the buffer"""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    path = f.f_code.co_filename
    parts = path.replace("\\", "/").split("/")
    return f"{'/'.join(parts[-2:])}:{f.f_lineno}"


class _Arena:
    __slots__ = ("arena", "front", "nbytes", "back", "fill", "site", "shape", "dtype", "kind")

    def describe(self) -> str:
        return f"{self.kind}{tuple(self.shape)} {self.dtype} allocated at {self.site}"


def bits(t: _torch.Tensor) -> _torch.Tensor:
    """the tensor's bytes as integers, on the host: what two runs are compared by (never `==` on floats: NaN != NaN)"""
    t = t.detach().contiguous()
    return t.reshape(-1).view(_torch.uint8).cpu()


def same_bits(a: _torch.Tensor, b: _torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and _torch.equal(bits(a), bits(b))


class GuardedTorch:
    """Forwards every attribute to ``torch``; ``zeros``, ``empty``, ``full``, ``zeros_like`` and ``empty_like`` whose result
    would live on a CUDA device (any device with ``devices="all"``) come out of guarded arenas instead."""

    def __init__(self, mode: str = "poison", devices: str = "cuda", row_stride: int = 0, guard: Optional[int] = None):
        if mode not in FILL:
            raise ValueError(f"mode must be 'zero' or 'poison', got {mode!r}")
        if devices not in ("cuda", "all"):
            raise ValueError(f"devices must be 'cuda' or 'all', got {devices!r}")
        self.__dict__["mode"] = mode
        self.__dict__["fill"] = FILL[mode]
        self.__dict__["devices"] = devices
        g = guard_bytes(row_stride) if guard is None else int(guard)
        # a condition, not a measurement: the guard is whole pages, at least 64 KiB and at least four of the widest rows
        assert g % PAGE == 0 and g >= MIN_GUARD and g >= 4 * int(row_stride), (g, row_stride)
        self.__dict__["guard"] = g
        self.__dict__["row_stride"] = int(row_stride)
        self.__dict__["arenas"] = []

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("GuardedTorch is read-only")

    # ------------------------------------------------------------------ which calls are taken
    def _wants(self, device) -> bool:
        if device is None:
            device = _torch.get_default_device() if hasattr(_torch, "get_default_device") else "cpu"
        dev = _torch.device(device)
        return self.devices == "all" or dev.type == "cuda"

    @staticmethod
    def _shape(size) -> tuple:
        if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
            size = size[0]
        return tuple(int(v) for v in size)

    @staticmethod
    def _plain(kw: dict, allowed=("dtype", "device", "requires_grad")) -> bool:
        """the keyword arguments the carver reproduces; a call with any other (out=, pin_memory=, memory_format=, ...) is not
        a device buffer of the package and passes through"""
        return all(k in allowed for k in kw)

    # ------------------------------------------------------------------ the carver
    def _carve(self, kind: str, shape: tuple, dtype, device, payload_fill: Optional[int]) -> _torch.Tensor:
        dtype = _torch.get_default_dtype() if dtype is None else dtype
        es = _torch.empty((), dtype=dtype).element_size()
        nbytes = es * math.prod(shape)
        front = back = self.guard
        arena = _torch.empty(front + nbytes + back, dtype=_torch.uint8, device=device)
        arena.fill_(self.fill)
        pay = arena[front:front + nbytes]
        if payload_fill is not None and payload_fill != self.fill and nbytes:
            pay.fill_(payload_fill)
        # the guards are whole pages, so the payload keeps the alignment the allocator gave the arena
        assert front % PAGE == 0 and back % PAGE == 0
        if arena.data_ptr() % 256 == 0:
            assert pay.data_ptr() % 256 == 0 or nbytes == 0, "payload lost the allocator's alignment"
        a = _Arena()
        a.arena, a.front, a.nbytes, a.back, a.fill = arena, front, nbytes, back, self.fill
        a.site, a.shape, a.dtype, a.kind = _call_site(), shape, dtype, kind
        self.arenas.append(a)
        out = pay.view(dtype).view(shape) if nbytes else _torch.empty(shape, dtype=dtype, device=device)
        assert out.is_contiguous() and (nbytes == 0 or out.data_ptr() == arena.data_ptr() + front)
        return out

    def _finish(self, t, kw):
        if kw.get("requires_grad"):
            t.requires_grad_(True)
        return t

    # ------------------------------------------------------------------ the intercepted entry points
    def empty(self, *size, **kw):
        if not (self._plain(kw) and self._wants(kw.get("device"))):
            return _torch.empty(*size, **kw)
        return self._finish(self._carve("empty", self._shape(size), kw.get("dtype"), kw.get("device"), None), kw)

    def zeros(self, *size, **kw):
        if not (self._plain(kw) and self._wants(kw.get("device"))):
            return _torch.zeros(*size, **kw)
        return self._finish(self._carve("zeros", self._shape(size), kw.get("dtype"), kw.get("device"), 0), kw)

    def full(self, size, fill_value, **kw):
        if not (self._plain(kw) and self._wants(kw.get("device"))):
            return _torch.full(size, fill_value, **kw)
        dtype = kw.get("dtype") or _torch.full((), fill_value).dtype
        t = self._carve("full", self._shape((size,)), dtype, kw.get("device"), None)
        t.fill_(fill_value)
        return self._finish(t, kw)

    def _like(self, kind, t, kw, payload_fill):
        device = kw.get("device", t.device)
        if not (self._plain(kw) and self._wants(device)) or t.layout != _torch.strided:
            return getattr(_torch, kind)(t, **kw)
        return self._finish(self._carve(kind, tuple(t.shape), kw.get("dtype", t.dtype), device, payload_fill), kw)

    def empty_like(self, t, **kw):
        return self._like("empty_like", t, kw, None)

    def zeros_like(self, t, **kw):
        return self._like("zeros_like", t, kw, 0)

    # ------------------------------------------------------------------ caller-made tensors
    def guard_copy(self, t: _torch.Tensor) -> _torch.Tensor:
        """`t` (an input, a target, a weight, a state, a weight map) copied into a guarded arena of its own; requires_grad
        is carried over (the copy is a leaf)"""
        out = self._carve("guard_copy", tuple(t.shape), t.dtype, t.device, None)
        out.copy_(t.detach())
        if t.requires_grad:
            out.requires_grad_(True)
        return out

    def guard_module(self, module):
        """every parameter and buffer of a module re-homed into guarded arenas (same values, same Parameter objects)"""
        for p in list(module.parameters()) + list(module.buffers()):
            p.data = self.guard_copy(p.data)
        return module

    # ------------------------------------------------------------------ the check
    def verify(self) -> int:
        """Compare every guard byte of every arena with its fill value; GuardError names each damaged buffer.  Returns the
        number of arenas checked."""
        if not self.arenas:
            return 0
        counts = []
        for a in self.arenas:
            g = a.arena
            counts.append((g[:a.front] != a.fill).sum() + (g[a.front + a.nbytes:] != a.fill).sum())
        by_dev = {}
        for i, c in enumerate(counts):
            by_dev.setdefault(c.device, []).append(i)
        damaged = []
        for dev, idx in by_dev.items():
            tot = _torch.stack([counts[i] for i in idx]).cpu().tolist()       # one read per device
            damaged += [i for i, n in zip(idx, tot) if n]
        if not damaged:
            return len(self.arenas)
        msgs = []
        for i in sorted(damaged):
            a = self.arenas[i]
            for side, lo, hi in (("front", 0, a.front), ("back", a.front + a.nbytes, a.front + a.nbytes + a.back)):
                g = a.arena[lo:hi]
                pos = (g != a.fill).nonzero().reshape(-1)
                if pos.numel() == 0:
                    continue
                first, last, n = int(pos[0]), int(pos[-1]), int(pos.numel())
                if side == "front":       # offsets relative to the payload's first byte: negative
                    rel = (first - a.front, last - a.front)
                    outer = first < PAGE
                else:                     # ... and to the payload's first byte again: nbytes = the first byte behind it
                    rel = (a.nbytes + first, a.nbytes + last)
                    outer = last >= a.back - PAGE
                msg = (f"guard damaged: {a.describe()}, {side} guard, {n} byte(s), payload-relative offsets "
                       f"[{rel[0]}, {rel[1]}] (payload is [0, {a.nbytes}))")
                if outer:
                    msg += (f"; damage in the outermost {PAGE} bytes of the guard: overrun may exceed the guard -- read the "
                            "extent from the code before this case runs again")
                msgs.append(msg)
        raise GuardError("\n".join(msgs))

    def release(self):
        self.arenas.clear()

    def find(self, site_part: str) -> List[_Arena]:
        """the arenas whose call site contains `site_part` (how a self-check picks one workspace slab)"""
        return [a for a in self.arenas if site_part in a.site]


@contextlib.contextmanager
def patched(modules: Sequence[str] = MODULES, mode: str = "poison", devices: str = "cuda", row_stride: int = 0,
            package: str = PACKAGE, proxy: Optional[GuardedTorch] = None):
    """``with patched(mode="poison", row_stride=...) as gt:`` -- the ``torch`` name of the named package modules is the proxy
    inside the context and what it was afterwards, whatever happens.  Build models, engines, trainers and accumulators, and
    use them for the first time, inside: their buffers are allocated lazily and cached.  ``gt.verify()`` before leaving."""
    gt = proxy if proxy is not None else GuardedTorch(mode, devices, row_stride)
    mods = [importlib.import_module(m if "." in m or not package else f"{package}.{m}") if isinstance(m, str) else m
            for m in modules]
    saved = [(m, m.__dict__["torch"]) for m in mods]
    try:
        for m in mods:
            m.torch = gt
        yield gt
    finally:
        for m, t in saved:
            m.torch = t
