"""Weight- and bias-gradient reductions checked exactly on integer data (TEST INFRASTRUCTURE ONLY; nothing in the product imports it).

The conv weight gradient (``csrc/wgrad.hip``) and the head's weight gradient (``nint_head_bwd``) reduce over every pixel of every
image: about 1.5 M terms per element at the bench geometry.  A rigorous error bound for real data is then wider than what one
dropped 4 x 32 pixel tile changes, so this module offers two checks:

* **Exact.**  ``int_values`` draws dG from {-1, 0, 1} and the x / h sources from {-2, ..., 2}.  Every product is then an
  integer, exact in bf16 x bf16 and in the f32 MFMA, and while ``exact_budget`` holds (every |partial sum| <= sum |dG||cat|
  < 2^24) every partial sum is an integer that f32 represents exactly, whatever the summation order.  The kernel's dW and
  db must then equal ``wgrad_ref`` (f64) bit for bit: a dropped tile, a doubled split, a swapped tap, an empty split that
  was never flushed or an h skip of the wrong length all show, whatever the shape size.
* **Bound** (``wgrad_bound``), for the real data the sequence path stores: ``|dW - ref| <= gamma_{n+1} sum |dG||cat|`` with a
  conservative chain length n.  It sees wiring mistakes that move whole sums (the source one time step off, the wrong
  layer's slab, the wrong skip, another layer's fold-table entry); a dropped tile is the exact check's job.

The tests write their slabs with the layout-only writers of ``oracle/stored_audit.py`` (halo, slack and channel padding stay
zero) and read them back with its readers.  Everything here runs on the device its tensors live on: the references are one f64 GEMM per tap on shifted views, chunked
over images (no conv routine: Winograd and FFT algorithms are not exact).

Conventions (``include/nint.h``, ``csrc/seq.hip``): dG (T*B, 4*Ch, H, W) in the reference's out-channel order ``gate*Ch + ch``;
x (T*B, Cx, H, W) the UNFOLDED input values (a folded slab holds the same values, shifted); h ((T+1)*B or T*B images, Ch,
H, W) with slot s = images [s*B, (s+1)*B), slot t = h_{t-1}: time step t reduces slot t, and slot 0 counts as zero for a
sequence from the zero state (``has_init = 0``: the kernel skips the first B images of the h source).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

U32 = 2.0 ** -24
EXACT_LIMIT = 2 ** 24          # every integer of magnitude <= 2^24 is an f32
DG_MAX, SRC_MAX = 1, 2         # the integer ranges of int_values: dG in {-1, 0, 1}, x / h in {-2, ..., 2}


def int_values(shape, vmax: int, gen: torch.Generator, device="cpu") -> torch.Tensor:
    """f32 tensor of integers drawn uniformly from {-vmax, ..., vmax} (exact in bf16 for vmax <= 256)"""
    return (torch.randint(-vmax, vmax + 1, tuple(shape), generator=gen, dtype=torch.int32).float()).to(device)


def exact_budget(N: int, H: int, W: int, dG_max: int = DG_MAX, src_max: int = SRC_MAX) -> int:
    """A bound on max over dW elements of sum |dG||cat| (and on the db column sums, which are smaller) for a reduction over N
    images of H x W pixels with |dG| <= dG_max and |x|, |h| <= src_max.  Refuses (AssertionError) a case where a partial
    sum could leave the integers f32 holds exactly; returns the bound."""
    b = N * H * W * dG_max * src_max
    assert b < EXACT_LIMIT and N * H * W * dG_max < EXACT_LIMIT, \
        f"{N} images of {H}x{W}: sum |dG||cat| may reach {b} >= 2^24, the exact check does not hold"
    return b


def _h_used(h: torch.Tensor, n0: int, n1: int, has_init: bool, B: int) -> torch.Tensor:
    """h_{t-1} of images n0..n1-1 (slot t = images t*B..), zero for the first B images of a zero-state sequence"""
    hv = h[n0:n1]
    if not has_init and n0 < B:
        hv = hv.clone()
        hv[:B - n0] = 0
    return hv


def _tap_sums(dG: torch.Tensor, x: torch.Tensor, h: Optional[torch.Tensor], k: int, has_init: bool, B: int,
              absval: bool = False, dtype=torch.float64, chunk: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """dW[o][c][ky][kx] = sum_{n,y,x} dG[n,o,y,x] * cat[n, c, y+ky-p, x+kx-p] (zero outside the image), db[o] = sum dG[., o];
    on dG's device in `dtype`.  absval: the same sums of |dG| and |cat|."""
    N, O, H, W = dG.shape
    Cx = x.shape[1]
    Ch = 0 if h is None else h.shape[1]
    p = k // 2
    dev = dG.device
    dW = torch.zeros(O, Cx + Ch, k, k, dtype=dtype, device=dev)
    db = torch.zeros(O, dtype=dtype, device=dev)
    if chunk <= 0:   # images per chunk: about 2^28 elements of f64 operands at a time
        chunk = max(1, (1 << 28) // max(1, (O + Cx + Ch) * (H + 2 * p) * (W + 2 * p)))
    for n0 in range(0, N, chunk):
        n1 = min(N, n0 + chunk)
        a = dG[n0:n1].to(dev, dtype)
        parts = [x[n0:n1].to(dev, dtype)]
        if h is not None:
            parts.append(_h_used(h, n0, n1, has_init, B).to(dev, dtype))
        cat = torch.cat(parts, dim=1)
        if absval:
            a, cat = a.abs(), cat.abs()
        db += a.sum(dim=(0, 2, 3))
        am = a.permute(1, 0, 2, 3).reshape(O, -1)
        cp = torch.nn.functional.pad(cat, (p, p, p, p))
        for ky in range(k):
            for kx in range(k):
                bm = cp[:, :, ky:ky + H, kx:kx + W].permute(1, 0, 2, 3).reshape(Cx + Ch, -1)
                dW[:, :, ky, kx] += am @ bm.t()
    return dW, db


def wgrad_ref(dG: torch.Tensor, x: torch.Tensor, h: Optional[torch.Tensor], k: int, xfold: bool = False, has_init: bool = True,
              B: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dW (4Ch, Cx+Ch, k, k), db (4Ch,)) in f64 of one layer's reduction over all N = T*B images of dG.  x holds the unfolded
    values whether or not the kernel reads a folded slab (``xfold`` changes the storage, not the sum); h: slots 0..T-1 are
    used (slot 0 as zero when has_init is false), None = no h source."""
    del xfold
    return _tap_sums(dG, x, h, k, has_init, B)


def chain_length(N: int, H: int, W: int, es: int, n_cu: int = 256) -> int:
    """A conservative length of the f32 accumulation chain of one dW element, without a copy of wg_plan: the MFMA K-steps over
    ALL pixel tiles of the reduction (bf16: 4 x 32-pixel tiles, 32 pixels per 16x16x32 step; f32: 2 x 32, 4 per 16x16x4 step)
    plus 2 n_cu for the split-K fold."""
    PR, K = (4, 32) if es == 2 else (2, 4)
    return math.ceil(H / PR) * math.ceil(W / 32) * N * (PR * 32 // K) + 2 * n_cu


def gamma(n: int) -> float:
    return n * U32 / (1 - n * U32)


def wgrad_bound(dG: torch.Tensor, x: torch.Tensor, h: Optional[torch.Tensor], k: int, es: int, has_init: bool = True, B: int = 1,
                n_cu: int = 256):
    """For real (stored) data: ((ref_dW, bound_dW), (ref_db, bound_db)) in f64, bound = gamma_{n+1} sum |dG||cat| with n =
    chain_length (the +1: one rounding per f32 product).  Catches mistakes that move whole sums (wrong source, time offset,
    skip, fold-table entry), not a single dropped pixel tile: the exact integer check is there for that."""
    N, _, H, W = dG.shape
    g = gamma(chain_length(N, H, W, es, n_cu) + 1)
    ref = _tap_sums(dG, x, h, k, has_init, B)
    mag = _tap_sums(dG, x, h, k, has_init, B, absval=True)
    return (ref[0], g * mag[0]), (ref[1], g * mag[1])


def bound_ratio(out: torch.Tensor, ref_bound) -> float:
    """max |out - ref| / bound over the elements (a zero bound needs an exact zero)"""
    ref, bound = ref_bound
    d = (out.to(ref.device, torch.float64) - ref).abs()
    if bool(((bound == 0) & (d != 0)).any()):
        return math.inf
    return float((d / bound.clamp_min(1e-300)).max())


def head_ref(h_top: torch.Tensor, dpred: torch.Tensor, w: torch.Tensor):
    """The head's backward in f64 (a 1x1 conv, model.py:274): h_top (N, Ch, H, W), dpred (N, O, H, W), w (O, Ch) ->
    dw[o][c] = sum dpred[n,o] h[n,c], db[o] = sum dpred[n,o], dh[n,c] = sum_o w[o][c] dpred[n,o]."""
    N, Ch, H, W = h_top.shape
    O = dpred.shape[1]
    dev = dpred.device
    dw = torch.zeros(O, Ch, dtype=torch.float64, device=dev)
    db = torch.zeros(O, dtype=torch.float64, device=dev)
    dh = torch.empty(N, Ch, H, W, dtype=torch.float64, device=dev)
    w64 = w.to(dev, torch.float64)
    for n in range(N):
        d = dpred[n].to(torch.float64).reshape(O, -1)
        hv = h_top[n].to(dev, torch.float64).reshape(Ch, -1)
        dw += d @ hv.t()
        db += d.sum(dim=1)
        dh[n] = (w64.t() @ d).reshape(Ch, H, W)
    return dw, db, dh
