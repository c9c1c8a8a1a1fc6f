"""Launch-by-launch audit of the sequence path against the values the kernels STORED (TEST INFRASTRUCTURE ONLY).

Every hot-path launch of ``nint_seq_fwd`` / ``nint_seq_bwd`` reads slabs that an earlier launch stored and that stay
resident in the ``engine.Workspace``.  This module recomputes each launch from exactly those stored inputs, in torch f64
on the CPU, and returns per element ``(ref, bound)``: the exact result of the launch's operation and a bound on how far
the kernel's f32 arithmetic plus its storage roundings may take its stored value from it.  A test then asserts
``max(|stored - ref| / bound) <= 1``.  Unlike a rel-L2 over a whole slab this sees one wrong tile, one dropped tap of one
channel chunk or one stale pixel.

Slab readers (layout only, no arithmetic) decode ``include/nint.h``: halo slabs ``[N][Hh][Wh][Cp]`` with the interior at
``[P:P+H, P:P+W]``, compact slabs ``[N][H][W][Cp]``, gate-stash / dG column ``(cblock*4 + gate)*16 + col`` for channel
``cblock*16 + col``, image ``n = t*B + b`` and the horizontally folded x slab (channel ``kx*Cx + c`` of pixel x holds
``x[x + kx - k/2][c]``).

Error model
-----------
``u = 2^-24`` is the f32 unit roundoff, ``u_ET`` that of the storage type (``2^-8`` for bf16; 0 for f32 storage, which
stores the f32 registers as they are).  Bounds are carried as running error bounds (Wilkinson): a value ``E(v, e)``
is the exact real value ``v`` of the quantity and a bound ``e`` on its distance from the kernel's f32 register.  Each
f32 operation of the kernel adds ``u * (|v| + e)`` (one rounding of a result whose magnitude is at most ``|v| + e``);
an operation with inputs ``E(a, ea)``, ``E(b, eb)`` propagates ``|a| eb + |b| ea + ea eb`` (product) or ``ea + eb``
(sum).  Terms, with the source lines they model:

* Convolution sums (``conv_igemm_body`` in ``csrc/conv_igemm.hip``: the gate kernels' bias-initialised accumulators, its
  "K-slice reduction" of partial sums, and the dgrad epilogue): every product of two stored values is exact in f32 (bf16 x bf16,
  or f32 x f32 inside the MFMA), so the only error is the f32 summation, ``gamma_n * sum |w| |a|`` with
  ``gamma_n = n u / (1 - n u)`` and n the number of roundings on the longest accumulation chain: ``R_MFMA`` per MFMA
  instruction (one per bf16 K-step of 32 channels, ``mma_step<NINT_BF16>``; four per f32 K-step of 16 channels,
  ``mma_step<NINT_F32>``, both in ``csrc/nint_common.h``) plus ``N_SLICE_ADDS`` for the bias and the K-slice partial adds.
  Layers the vector-ALU stencil kernel can run (``fma_quad`` in ``csrc/stencil.hip``: one ``fmaf`` per product) use the product
  count instead.  ``R_MFMA = 1``: n is the K-step count (bf16) or the instruction count (f32), not ``K * u``, which would
  hide a dropped K-chunk.  How ``v_mfma_f32_16x16x32_bf16`` rounds inside one instruction is not documented; what is
  measured is the whole sum: with f32 storage the stash holds the g gate's f32 register, so ``atanh`` of it recovers the
  kernel's pre-activation to ~1e-6 and the audit reports the share of the accumulation bound actually used ('zacc',
  ``_z_from_stash``).  That share is at most 0.30 on the MI355X over every f32 case of tests/test_gpu_stored_audit.py,
  so one rounding per instruction needs no extra allowance.  In bf16 the stored values' own rounding dominates every
  ratio; the accumulation term is the same model.
* ``sigmoidf_`` (``csrc/nint_common.h``): ``rcp(1 + __expf(-z))``.  ``__expf`` scales by log2(e) (one rounding of
  the product, one of the constant: relative ``2|z| u`` of the result) and ``v_exp_f32`` is 1 ulp (``2u``, taken as
  ``4u``); the ``1 +`` rounds once and ``v_rcp_f32`` is 1 ulp (``2u``):
  ``eps_sig(z) = sigma * ((1 - sigma)(2|z| + 4) + 3) u``.
* ``tanhf_`` (``csrc/nint_common.h``): ``fma(2, sigmoid(2x), -1)``: ``eps_tanh(x) = 2 eps_sig(2x) + u |tanh x|``
  (about ``2.4e-7`` absolute near 0: the cancellation is absolute, not relative).
* A derivative taken through an activation uses its largest value on ``[|z| - e, |z| + e]`` (``sigma'`` and ``tanh'``
  fall with ``|z|``), so a bound never rests on a single point of a steep curve.
* LSTM epilogue (``lstm_cell_elem`` in ``csrc/nint_common.h``, called by the MFMA epilogue of ``conv_igemm_body`` and by
  ``stencil_lstm_kernel``; ``tiny_lstm_kernel`` holds its written-out twin): ``c = fma(c_prev, f, i*g)``,
  ``h = o * tanh(c)``; ``c_prev`` is the STORED f32 value, so it is exact.
* Pointwise backward (``lstm_bwd_elem`` in ``csrc/nint_common.h``, called by ``lstm_bwd_pointwise_body`` and by the
  fused step's ``EPI_DGRAD_PW`` epilogue of ``conv_igemm_body``): the
  operations in the kernel's order, gates and ``c`` being stored (exact) inputs, ``dh`` and ``dc`` carrying bounds.
* Transient ``dh`` (``include/nint.h``, ``nint_seq.wave`` and ``nint_cell_bwd_fused``): ``dh_t`` is the sum of two
  pieces, the h columns of the layer's own dgrad of time t+1 (or the injected ``dL/dh_{T-1}``) and the x columns of the
  layer above's dgrad of time t.  Rounded to bf16 per piece it is stored in: classic steps store the first piece and
  read-modify-write the sum (``u_ET (|p_h| + |p_h + p_x|)``), wave 4 / 5 store both pieces (``u_ET (|p_h| + |p_x|)``),
  the fused step keeps its own piece in registers (``u_ET |p_x|``) and a ``lo_*`` problem the other one
  (``u_ET |p_h|``).  The audit does not know which schedule ran each step, so it takes the sum of the three terms, which
  is at least each schedule's own; then one f32 add.
* One RNE rounding per stored ET value: half an ulp of the binade of ``|ref| + e`` (``halfulp``).
* ``dc`` is carried from ``T-1`` down with its own running bound through the chain (``dc_{t-1} = dct * f``).
* ``dx`` of a folded input: each folded piece is rounded to ET once, then ``nint_unfold_dx`` sums the ``k`` pieces in
  f32 (``gamma_k``).

Padding invariants (``check_padding``): the halo ring, the row / column slack and the channel padding of ``xs``, ``h[l]``
and ``dG[l]`` are bit-exact zero after a pass (``engine.Workspace``: "kernels only ever write their interior"; dgrad and
wgrad read the ring as the convolution's zero padding).  The padded gate columns ``Ch..Ch16`` of dG are bit-exact zero:
wgrad sums them into weight-gradient rows that are discarded, and dgrad multiplies them by zero weights, so the only
thing a consumer needs there is a finite value; zero is what the pointwise backward produces from a zero-weight channel
(``dh = dc = 0``).  The padded stash columns hold the activations of a zero pre-activation, ``(i, f, g, o) =
(0.5, 0.5, 0, 0.5)`` exactly (``lstm_stash_zero_w`` in ``csrc/nint_common.h``: ``stencil_lstm_kernel`` and
``tiny_lstm_kernel`` write them explicitly; the MFMA kernels compute them), which the pointwise backward needs finite for the zero dG above.  The channel padding of ``c``, ``dh`` and ``dc`` is zero.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

__all__ = ["Geo", "LayerGeo", "geo_of", "stored_dG", "read_xs", "read_h", "read_c", "read_gates", "read_dG", "read_compact",
           "write_halo", "write_compact", "write_gates", "write_dG", "write_xs", "check_padding", "E", "fwd_launch",
           "bwd_chain", "ratio", "halfulp", "read_workspace", "audit", "U32", "R_MFMA", "N_SLICE_ADDS"]

U32 = 2.0 ** -24
R_MFMA = 1          # roundings per MFMA instruction on the accumulation chain (see the module docstring)
N_SLICE_ADDS = 4    # the bias (accumulator start) and up to three K-slice partial adds


# --------------------------------------------------------------------------- geometry
@dataclass
class LayerGeo:
    Cx: int
    Ch: int
    k: int
    xfold: bool
    Cxp: int
    Ch16: int
    Chp: int
    tile_rows: int = 0


@dataclass
class Geo:
    B: int
    T: int
    H: int
    W: int
    P: int
    Hh: int
    Wh: int
    es: int            # bytes per stored element: 2 = bf16, 4 = f32
    layers: List[LayerGeo]

    @property
    def et(self):
        return torch.bfloat16 if self.es == 2 else torch.float32

    @property
    def kc(self):
        return 32 if self.es == 2 else 16

    @property
    def u_et(self):
        return 2.0 ** -8 if self.es == 2 else 0.0

    @staticmethod
    def make(B, T, H, W, layers: Sequence[Tuple[int, int, int, bool]], es: int):
        """(Cx, Ch, k, xfold) per layer -> the padded geometry nint_geom_make / LayerCfg.padded compute."""
        kc = 32 if es == 2 else 16
        rup = lambda a, b: (a + b - 1) // b * b
        P = max(k // 2 for _, _, k, _ in layers)
        ls = [LayerGeo(Cx, Ch, k, bool(xf), rup(k * Cx if xf else Cx, kc), rup(Ch, 16), rup(Ch, kc)) for Cx, Ch, k, xf in layers]
        return Geo(B, T, H, W, P, rup(H, 8) + 2 * P, rup(W, 32) + 2 * P, es, ls)


def geo_of(eng, ws) -> Geo:
    g = ws.g
    ls = []
    for cfg, ly in zip(eng.cfgs, eng.layers):
        Cxp, Ch16, Chp = cfg.padded(eng.kc)
        ls.append(LayerGeo(cfg.Cx, cfg.Ch, cfg.k, bool(cfg.xfold), Cxp, Ch16, Chp, int(ly.tile_rows)))
    return Geo(ws.B, ws.T, ws.H, ws.W, g.P, g.Hh, g.Wh, eng.es, ls)


# --------------------------------------------------------------------------- readers (layout only)
def _slab(geo: Geo, buf: torch.Tensor, N: int, C: int, halo: bool, et=None) -> torch.Tensor:
    et = et or geo.et
    t = buf.detach().cpu().contiguous().view(torch.uint8).view(et)
    return t.view(N, geo.Hh, geo.Wh, C) if halo else t.view(N, geo.H, geo.W, C)


def _interior(geo: Geo, s: torch.Tensor) -> torch.Tensor:
    return s[:, geo.P:geo.P + geo.H, geo.P:geo.P + geo.W, :]


def _gate_cols(Ch16: int, Ch: int) -> torch.Tensor:
    """index into the stash columns of out-channel gate*Ch + ch (reference order [i,f,g,o])"""
    idx = [((ch // 16) * 4 + gate) * 16 + ch % 16 for gate in range(4) for ch in range(Ch)]
    return torch.tensor(idx, dtype=torch.long)


def read_xs(geo: Geo, xs: torch.Tensor) -> torch.Tensor:
    """ws.xs -> (T*B, Cx, H, W) f32 (exact: every stored value is an f32).  A folded slab must hold, in every kx group, the centre group shifted by kx - k/2
    with zeros outside the image (asserted bit for bit)."""
    ly = geo.layers[0]
    s = _interior(geo, _slab(geo, xs, geo.T * geo.B, ly.Cxp, True))
    if not ly.xfold:
        return s[..., :ly.Cx].float().permute(0, 3, 1, 2).contiguous()
    p, C = ly.k // 2, ly.Cx
    centre = s[..., p * C:(p + 1) * C]
    for kx in range(ly.k):
        want = torch.zeros_like(centre)
        d = kx - p
        lo, hi = max(0, -d), min(geo.W, geo.W - d)
        want[:, :, lo:hi] = centre[:, :, lo + d:hi + d]
        got = s[..., kx * C:(kx + 1) * C]
        bad = (got.view(torch.int16 if geo.es == 2 else torch.int32) != want.view(torch.int16 if geo.es == 2 else torch.int32))
        assert not bool(bad.any()), f"folded x slab: group kx={kx} is not the centre group shifted by {d} ({int(bad.sum())} elements)"
    return centre.float().permute(0, 3, 1, 2).contiguous()


def read_h(geo: Geo, l: int, h: torch.Tensor) -> torch.Tensor:
    """ws.h[l] -> ((T+1)*B, Ch, H, W) f32 (exact); slot s = images [s*B, (s+1)*B): slot 0 = initial state, slot t+1 = h_t"""
    ly = geo.layers[l]
    s = _interior(geo, _slab(geo, h, (geo.T + 1) * geo.B, ly.Chp, True))
    return s[..., :ly.Ch].float().permute(0, 3, 1, 2).contiguous()


def read_compact(geo: Geo, buf: torch.Tensor, N: int, C: int, Cp: int, et) -> torch.Tensor:
    s = _slab(geo, buf, N, Cp, False, et)
    return s[..., :C].float().permute(0, 3, 1, 2).contiguous()


def read_c(geo: Geo, l: int, c: torch.Tensor) -> torch.Tensor:
    ly = geo.layers[l]
    return read_compact(geo, c, (geo.T + 1) * geo.B, ly.Ch, ly.Chp, torch.float32)


def read_gates(geo: Geo, l: int, gates: torch.Tensor) -> torch.Tensor:
    """ws.gates[l] (stash [T*B][H][W][4*Ch16]) -> (T*B, 4*Ch, H, W) f32 in the order [i,f,g,o]"""
    ly = geo.layers[l]
    s = _slab(geo, gates, geo.T * geo.B, 4 * ly.Ch16, False)
    return s[..., _gate_cols(ly.Ch16, ly.Ch)].float().permute(0, 3, 1, 2).contiguous()


def read_dG(geo: Geo, l: int, dG: torch.Tensor) -> torch.Tensor:
    """ws.dG[l] (halo slab [T*B][Hh][Wh][4*Ch16]) -> (T*B, 4*Ch, H, W) f32 in the order [i,f,g,o]"""
    ly = geo.layers[l]
    s = _interior(geo, _slab(geo, dG, geo.T * geo.B, 4 * ly.Ch16, True))
    return s[..., _gate_cols(ly.Ch16, ly.Ch)].float().permute(0, 3, 1, 2).contiguous()


def stored_dG(eng, ws, l):
    """ws.dG[l] -> f32 (T*B, 4*Ch, H, W) on the slab's device in the reference's out-channel order [i,f,g,o]: the summands the
    weight-gradient kernel reduced (layout only, no arithmetic; the column map of read_dG)."""
    g, cfg = ws.g, eng.cfgs[l]
    Ch16 = (cfg.Ch + 15) // 16 * 16
    N = ws.T * ws.B
    t = ws.dG[l].view(torch.bfloat16 if eng.es == 2 else torch.float32).view(N, g.Hh, g.Wh, 4 * Ch16)
    t = t[:, g.P:g.P + ws.H, g.P:g.P + ws.W, :][..., _gate_cols(Ch16, cfg.Ch).to(t.device)]
    return t.float().permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------- writers (layout only; synthetic slabs for the CPU tests)
def _to_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(-1).view(torch.uint8).clone()


def write_halo(geo: Geo, v: torch.Tensor, Cp: int) -> torch.Tensor:
    """(N, C, H, W) values -> halo slab bytes (ET, zero ring / slack / channel padding), on v's device"""
    N, C = v.shape[:2]
    s = torch.zeros(N, geo.Hh, geo.Wh, Cp, dtype=geo.et, device=v.device)
    s[:, geo.P:geo.P + geo.H, geo.P:geo.P + geo.W, :C] = v.permute(0, 2, 3, 1).to(geo.et)
    return _to_bytes(s)


def write_xs(geo: Geo, x: torch.Tensor) -> torch.Tensor:
    """(T*B, Cx, H, W) -> ws.xs bytes, folded when layer 0 is"""
    ly = geo.layers[0]
    if not ly.xfold:
        return write_halo(geo, x, ly.Cxp)
    p = ly.k // 2
    groups = []
    for kx in range(ly.k):
        d = kx - p
        g = torch.zeros_like(x)
        lo, hi = max(0, -d), min(geo.W, geo.W - d)
        g[..., lo:hi] = x[..., lo + d:hi + d]
        groups.append(g)
    return write_halo(geo, torch.cat(groups, dim=1), ly.Cxp)


def write_compact(geo: Geo, v: torch.Tensor, Cp: int, et) -> torch.Tensor:
    N, C = v.shape[:2]
    s = torch.zeros(N, geo.H, geo.W, Cp, dtype=et)
    s[..., :C] = v.permute(0, 2, 3, 1).to(et)
    return _to_bytes(s)


def _gate_slab(geo: Geo, l: int, v: torch.Tensor, halo: bool, pad_vals) -> torch.Tensor:
    ly = geo.layers[l]
    N = v.shape[0]
    Gc = 4 * ly.Ch16
    s = torch.zeros(N, geo.H, geo.W, Gc, dtype=geo.et, device=v.device)
    for gate in range(4):
        for ch in range(ly.Ch, ly.Ch16):
            s[..., ((ch // 16) * 4 + gate) * 16 + ch % 16] = pad_vals[gate]
    s[..., _gate_cols(ly.Ch16, ly.Ch).to(v.device)] = v.permute(0, 2, 3, 1).to(geo.et)
    if not halo:
        return _to_bytes(s)
    h = torch.zeros(N, geo.Hh, geo.Wh, Gc, dtype=geo.et, device=v.device)
    h[:, geo.P:geo.P + geo.H, geo.P:geo.P + geo.W] = s
    return _to_bytes(h)


def write_gates(geo: Geo, l: int, v: torch.Tensor) -> torch.Tensor:
    return _gate_slab(geo, l, v, False, (0.5, 0.5, 0.0, 0.5))


def write_dG(geo: Geo, l: int, v: torch.Tensor) -> torch.Tensor:
    return _gate_slab(geo, l, v, True, (0.0, 0.0, 0.0, 0.0))


# --------------------------------------------------------------------------- padding invariants
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def check_padding(geo: Geo, slabs: Dict[str, torch.Tensor]) -> List[str]:
    """Every halo / slack element and every channel-padding column of the given slabs (keys 'xs', 'h{l}', 'dG{l}',
    'gates{l}', 'c{l}', 'dh{l}', 'dc{l}') against the invariant of the module docstring.  Returns the violations."""
    out = []
    P, H, W = geo.P, geo.H, geo.W

    def halo_zero(name, s, cvalid):
        b = _bits(s)
        ring = b.clone()
        ring[:, P:P + H, P:P + W, :] = 0
        n_ring = int((ring != 0).sum())
        n_pad = int((b[:, P:P + H, P:P + W][..., cvalid] != 0).sum()) if cvalid is not None else 0
        if n_ring:
            out.append(f"{name}: {n_ring} nonzero halo / slack elements")
        if n_pad:
            out.append(f"{name}: {n_pad} nonzero channel-padding elements")

    for name, buf in slabs.items():
        if name == "xs":
            ly = geo.layers[0]
            s = _slab(geo, buf, geo.T * geo.B, ly.Cxp, True)
            used = ly.k * ly.Cx if ly.xfold else ly.Cx
            halo_zero(name, s, slice(used, None))
            continue
        kind, l = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
        ly = geo.layers[l]
        padg = torch.tensor([((ch // 16) * 4 + gate) * 16 + ch % 16 for gate in range(4) for ch in range(ly.Ch, ly.Ch16)],
                            dtype=torch.long)
        if kind == "h":
            halo_zero(name, _slab(geo, buf, (geo.T + 1) * geo.B, ly.Chp, True), slice(ly.Ch, None))
        elif kind == "dG":
            halo_zero(name, _slab(geo, buf, geo.T * geo.B, 4 * ly.Ch16, True), padg)
        elif kind == "gates":
            s = _slab(geo, buf, geo.T * geo.B, 4 * ly.Ch16, False).float()
            if len(padg):
                want = torch.tensor([0.5, 0.5, 0.0, 0.5]).repeat_interleave(ly.Ch16 - ly.Ch)
                n = int((s[..., padg] != want).sum())
                if n:
                    out.append(f"{name}: {n} padded stash columns are not the activations of a zero pre-activation")
        elif kind in ("c", "dh", "dc"):
            N = (geo.T + 1) * geo.B if kind == "c" else geo.B
            et = geo.et if kind == "dh" else torch.float32
            s = _slab(geo, buf, N, ly.Chp, False, et)
            n = int((s[..., ly.Ch:] != 0).sum())
            if n:
                out.append(f"{name}: {n} nonzero channel-padding elements")
        else:
            raise KeyError(name)
    return out


# --------------------------------------------------------------------------- running error bounds
def halfulp(m: torch.Tensor, u_et: float) -> torch.Tensor:
    """half an ulp of the storage type at magnitude m (the RNE rounding error of a value of at most that magnitude)"""
    if u_et == 0.0:
        return torch.zeros_like(m)
    e = torch.floor(torch.log2(m.clamp_min(2.0 ** -126)))
    return torch.exp2(e) * u_et


class E:
    """exact value v (f64) and a bound e on its distance from the kernel's f32 register"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    def mag(self):
        return self.v.abs() + self.e

    def _r(self, v, e, rnd):
        return E(v, e + (U32 * (v.abs() + e) if rnd else 0))

    def mul(self, o, rnd=True):
        o = o if isinstance(o, E) else E(o)
        return self._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e, rnd)

    def add(self, o, rnd=True):
        o = o if isinstance(o, E) else E(o)
        return self._r(self.v + o.v, self.e + o.e, rnd)

    def rsub(self, c, rnd=True):             # c - self
        return self._r(c - self.v, self.e.clone(), rnd)


def gamma(n) -> float:
    return n * U32 / (1 - n * U32)


def eps_sig(z):
    s = torch.sigmoid(z)
    return s * ((1 - s) * (2 * z.abs() + 4) + 3) * U32


def eps_tanh(x):
    return 2 * eps_sig(2 * x) + U32 * torch.tanh(x).abs()


def sig_act(z: E) -> E:
    """sigmoidf_ of a pre-activation carrying a bound"""
    zl = (z.v.abs() - z.e).clamp_min(0)
    s = torch.sigmoid(zl)
    dmax = s * (1 - s)
    return E(torch.sigmoid(z.v), dmax * z.e + eps_sig(z.v))


def tanh_act(z: E) -> E:
    zl = (z.v.abs() - z.e).clamp_min(0)
    dmax = 1 - torch.tanh(zl) ** 2
    return E(torch.tanh(z.v), dmax * z.e + eps_tanh(z.v))


def stencil_may_run(ly: LayerGeo) -> bool:
    """nint_stencil_holds (csrc/stencil.hip): Ch <= 8, k = 3, thin input -- such layers may accumulate one fmaf per product"""
    return ly.Ch <= 8 and ly.k == 3 and ((not ly.xfold and ly.Cx <= 16) or (ly.xfold and ly.k * ly.Cx <= 64))


def n_fwd(geo: Geo, l: int, with_h: bool) -> int:
    ly = geo.layers[l]
    per = R_MFMA * (1 if geo.es == 2 else 4)
    ksteps = (ly.k if ly.xfold else ly.k * ly.k) * ly.Cxp // geo.kc + (ly.k * ly.k * ly.Chp // geo.kc if with_h else 0)
    n = per * ksteps + N_SLICE_ADDS
    if stencil_may_run(ly):
        n = max(n, ly.k * ly.k * (ly.Cxp + ly.Chp) + N_SLICE_ADDS)
    return n


def n_dgrad(geo: Geo, l: int) -> int:
    ly = geo.layers[l]
    per = R_MFMA * (1 if geo.es == 2 else 4)
    return per * (4 * ly.Ch16 // geo.kc) * ly.k * ly.k + N_SLICE_ADDS


def _wbf(geo: Geo, Wt: torch.Tensor) -> torch.Tensor:
    """the f32 parameter rounded RNE to the storage type, as nint_pack_weights stores it"""
    return Wt.detach().float().to(geo.et).double()


def ratio(stored: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    return (stored.double() - ref).abs() / bound.clamp_min(1e-300)


# --------------------------------------------------------------------------- forward launch (l, t)
def fwd_launch(geo: Geo, l: int, x: torch.Tensor, h_prev: Optional[torch.Tensor], c_prev: Optional[torch.Tensor],
               Wt: torch.Tensor, bias: Optional[torch.Tensor]) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Gate launch of layer l at one time step from its stored inputs: x (B, Cx, H, W) (the stored x slab unfolded, or the
    stored h of the layer below), h_prev / c_prev the stored state (None: zero state, the h half of K skipped), Wt / bias the
    f32 parameters.  Returns {'gates': (ref, bound) (B, 4Ch, H, W) [i,f,g,o], 'c': ..., 'h': ...} for the stored values."""
    ly = geo.layers[l]
    Wb = _wbf(geo, Wt)
    k, Ch = ly.k, ly.Ch
    B = x.shape[0]
    hp = torch.zeros(B, Ch, geo.H, geo.W, dtype=torch.float64) if h_prev is None else h_prev
    cat = torch.cat([x, hp], dim=1)
    b = torch.zeros(4 * Ch, dtype=torch.float64) if bias is None else bias.detach().double()
    z = F.conv2d(cat, Wb, b, padding=k // 2)
    s_abs = F.conv2d(cat.abs(), Wb.abs(), b.abs(), padding=k // 2)
    zE = E(z, gamma(n_fwd(geo, l, h_prev is not None)) * s_abs)
    zi, zf, zg, zo = (E(z[:, j * Ch:(j + 1) * Ch], zE.e[:, j * Ch:(j + 1) * Ch]) for j in range(4))
    gi, gf, go = sig_act(zi), sig_act(zf), sig_act(zo)
    gg = tanh_act(zg)
    cp = E(torch.zeros_like(gi.v) if c_prev is None else c_prev)
    ig = gi.mul(gg)                                           # gi * gg
    c = cp.mul(gf, rnd=False).add(ig)                         # fmaf(cp, gf, gi*gg): one rounding
    tc = tanh_act(c)
    h = go.mul(tc)
    u = geo.u_et
    gates_v = torch.cat([gi.v, gf.v, gg.v, go.v], dim=1)
    gates_e = torch.cat([gi.e, gf.e, gg.e, go.e], dim=1)
    return {"gates": (gates_v, gates_e + halfulp(gates_v.abs() + gates_e, u)),
            "c": (c.v, c.e),
            "h": (h.v, h.e + halfulp(h.mag(), u)),
            "zg": (zg.v, zg.e)}


# --------------------------------------------------------------------------- backward
def _dgrad(geo: Geo, l: int, dG: torch.Tensor, Wt: torch.Tensor):
    """d cat[x, h] = W^T (*) dG of layer l for one time step: (value, bound of the f32 accumulation), (B, Cx+Ch, H, W)"""
    ly = geo.layers[l]
    Wb = _wbf(geo, Wt)
    shape = (dG.shape[0], ly.Cx + ly.Ch, geo.H, geo.W)
    v = torch.nn.grad.conv2d_input(shape, Wb, dG, padding=ly.k // 2)
    a = torch.nn.grad.conv2d_input(shape, Wb.abs(), dG.abs(), padding=ly.k // 2)
    return v, gamma(n_dgrad(geo, l)) * a


def _dx_unfolded(geo: Geo, dG0: torch.Tensor, Wt: torch.Tensor):
    """d/dx of layer 0 for one time step as engine.backward returns it: per folded piece (one horizontal tap kx) one ET
    rounding, then the f32 sum of the k pieces (nint_unfold_dx); unfolded: one ET rounding"""
    ly = geo.layers[0]
    Wb = _wbf(geo, Wt)[:, :ly.Cx]
    shape = (dG0.shape[0], ly.Cx, geo.H, geo.W)
    n = gamma(n_dgrad(geo, 0))
    u = geo.u_et
    if not ly.xfold:
        v = torch.nn.grad.conv2d_input(shape, Wb, dG0, padding=ly.k // 2)
        e = n * torch.nn.grad.conv2d_input(shape, Wb.abs(), dG0.abs(), padding=ly.k // 2)
        return v, e + halfulp(v.abs() + e, u)
    v = torch.zeros(shape, dtype=torch.float64)
    e = torch.zeros(shape, dtype=torch.float64)
    mags = torch.zeros(shape, dtype=torch.float64)
    for kx in range(ly.k):
        m = torch.zeros_like(Wb)
        m[..., kx] = 1
        pv = torch.nn.grad.conv2d_input(shape, Wb * m, dG0, padding=ly.k // 2)
        pe = n * torch.nn.grad.conv2d_input(shape, (Wb * m).abs(), dG0.abs(), padding=ly.k // 2)
        pe = pe + halfulp(pv.abs() + pe, u)
        v, e, mags = v + pv, e + pe, mags + pv.abs() + pe
    return v, e + gamma(ly.k) * mags


def pointwise(geo: Geo, dh: E, dc: E, gates: torch.Tensor, c_prev: Optional[torch.Tensor], c_new: torch.Tensor):
    """pointwise backward (lstm_bwd_elem, csrc/nint_common.h) in the kernel's operation order; gates (B, 4Ch, H, W) and c are the
    stored (exact) inputs.  Returns (dG (B, 4Ch, H, W) as E before the ET store, dc_prev as E)."""
    Ch = gates.shape[1] // 4
    gi, gf, gg, go = (gates[:, j * Ch:(j + 1) * Ch] for j in range(4))
    cp = torch.zeros_like(c_new) if c_prev is None else c_prev
    tc = E(torch.tanh(c_new), eps_tanh(c_new))                          # tanhf_(cn)
    one_m = tc.mul(tc).rsub(1.0)                                        # 1 - tc*tc
    dct = dc.add(dh.mul(go).mul(one_m))                                 # dcv + dhv*go*(1 - tc*tc)
    d_o = dh.mul(tc)                                                    # dhv * tc
    one_minus = lambda a: E(a).rsub(1.0)                                # 1.f - a of a stored gate: one rounding
    o_i = dct.mul(gg).mul(gi).mul(one_minus(gi))                        # dct * gg * gi * (1 - gi)
    o_f = dct.mul(cp).mul(gf).mul(one_minus(gf))                        # dct * cp * gf * (1 - gf)
    o_g = dct.mul(gi).mul(E(gg).mul(gg).rsub(1.0))                      # dct * gi * (1 - gg*gg)
    o_o = d_o.mul(go).mul(one_minus(go))                                # d_o * go * (1 - go)
    dG = E(torch.cat([o_i.v, o_f.v, o_g.v, o_o.v], dim=1), torch.cat([o_i.e, o_f.e, o_g.e, o_o.e], dim=1))
    return dG, dct.mul(gf)


class _Lazy64:
    """slices of a stored f32 tensor in f64 (the whole slab in f64 would not fit a long sequence in host memory)"""

    def __init__(self, t):
        self.t = t

    def __getitem__(self, i):
        return self.t[i].double()


def bwd_chain(geo: Geo, Ws: Sequence[torch.Tensor], dG: Sequence[torch.Tensor], gates: Sequence[torch.Tensor],
              c: Sequence[torch.Tensor], dh_T: Sequence[Optional[torch.Tensor]], dc_T: Sequence[Optional[torch.Tensor]],
              t_min: int = 0, has_init: bool = False, need_dx: bool = True):
    """The BPTT launches from the stored slabs.  dG[l] (T*B, 4Ch, H, W), gates[l] the same shape, c[l] ((T+1)*B, Ch, H, W):
    stored values (f64).  dh_T / dc_T: the state gradients at T-1 as stored in ws.dh / ws.dc before the backward (None:
    zero).  Audits time steps t_min .. T-1 (the dc chain runs from T-1 down).  Returns a list of
    (name, stored-key, ref, bound): ('dG', (l, t)), ('dx', t), ('dh_init', l), ('dc_init', l)."""
    B, T, L = geo.B, geo.T, len(geo.layers)
    sl = lambda t: slice(t * B, (t + 1) * B)
    out = []
    dgr = {}
    dG = [d if d.dtype == torch.float64 else _Lazy64(d) for d in dG]
    gates = [g if g.dtype == torch.float64 else _Lazy64(g) for g in gates]
    c = [v if v.dtype == torch.float64 else _Lazy64(v) for v in c]

    def dg(l, t):                                # d cat of layer l at time t from the STORED dG
        if (l, t) not in dgr:
            dgr[(l, t)] = _dgrad(geo, l, dG[l][sl(t)], Ws[l])
        return dgr[(l, t)]

    u = geo.u_et
    dc_run = []
    for l in range(L):
        z = torch.zeros(B, geo.layers[l].Ch, geo.H, geo.W, dtype=torch.float64)
        dc_run.append(E(z.clone() if dc_T[l] is None else dc_T[l].double()))
    for t in range(T - 1, t_min - 1, -1):
        for l in range(L - 1, -1, -1):
            Ch = geo.layers[l].Ch
            if t == T - 1:
                ph = E(torch.zeros(B, Ch, geo.H, geo.W, dtype=torch.float64) if dh_T[l] is None else dh_T[l].double())
            else:
                v, e = dg(l, t + 1)
                ph = E(v[:, -Ch:], e[:, -Ch:])
            if l < L - 1:
                v, e = dg(l + 1, t)
                Cx1 = geo.layers[l + 1].Cx
                px = E(v[:, :Cx1], e[:, :Cx1])
            else:
                px = E(torch.zeros_like(ph.v))
            s = ph.add(px, rnd=False)
            rnd = u * (ph.mag() + px.mag() + s.mag())                   # the per-schedule ET roundings (docstring)
            dh = E(s.v, s.e + rnd).add(E(torch.zeros_like(s.v)))       # + the f32 add of the two pieces
            g_sl = gates[l][sl(t)]
            cp = c[l][sl(t)] if (t > 0 or has_init) else None
            dGe, dc_run[l] = pointwise(geo, dh, dc_run[l], g_sl, cp, c[l][sl(t + 1)])
            out.append(("dG", (l, t), dGe.v, dGe.e + halfulp(dGe.mag(), u)))
        if need_dx:
            v, e = _dx_unfolded(geo, dG[0][sl(t)], Ws[0])
            out.append(("dx", t, v, e))
    if t_min == 0 and has_init:
        for l in range(L):
            Ch = geo.layers[l].Ch
            v, e = dg(l, 0)
            ph = E(v[:, -Ch:], e[:, -Ch:])
            out.append(("dh_init", l, ph.v, ph.e + halfulp(ph.mag(), u)))
            out.append(("dc_init", l, dc_run[l].v, dc_run[l].e))
    return out


# --------------------------------------------------------------------------- whole pass
def read_workspace(eng, ws, dx: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """Every slab of a workspace after forward + backward, decoded on the CPU (f32: exact for every stored value) (plus the raw bytes for check_padding).
    dx: engine.backward's (B, T, C, H, W) f32 result (the unfolded input gradient).
    An inference workspace (train=False) has no stash, dG, dh or dc: those entries are None and the audit checks h, c and the
    padding only."""
    geo = geo_of(eng, ws)
    L = len(geo.layers)
    train = bool(ws.train)
    st = {"geo": geo, "x": read_xs(geo, ws.xs),
          "h": [read_h(geo, l, ws.h[l]) for l in range(L)], "c": [read_c(geo, l, ws.c[l]) for l in range(L)],
          "gates": [read_gates(geo, l, ws.gates[l]) for l in range(L)] if train else None,
          "dG": [read_dG(geo, l, ws.dG[l]) for l in range(L)] if train else None,
          "dh_fin": [read_compact(geo, ws.dh[l], geo.B, geo.layers[l].Ch, geo.layers[l].Chp, geo.et) for l in range(L)] if train else None,
          "dc_fin": [read_compact(geo, ws.dc[l], geo.B, geo.layers[l].Ch, geo.layers[l].Chp, torch.float32) for l in range(L)] if train else None,
          "dx": None if dx is None else dx.detach().cpu().float().transpose(0, 1).reshape(geo.T * geo.B, *dx.shape[2:])}
    raw = {"xs": ws.xs.cpu()}
    for l in range(L):
        raw.update({f"h{l}": ws.h[l].cpu(), f"c{l}": ws.c[l].cpu()})
        if train:
            raw.update({f"dG{l}": ws.dG[l].cpu(), f"gates{l}": ws.gates[l].cpu(), f"dh{l}": ws.dh[l].cpu(), f"dc{l}": ws.dc[l].cpu()})
    st["raw"] = raw
    return st


def _z_from_stash(gates: torch.Tensor, zg: torch.Tensor, e_acc: torch.Tensor):
    """The accumulation alone, measured (f32 storage only, where the stash holds the f32 registers): the g-gate pre-activation
    recovered from the stored tanh, z_meas = atanh(g), on the elements with |g| <= 0.75, where atanh is well conditioned.
    |z_meas - z_ref| <= gamma_n sum|w||a| + eps_tanh / (1 - (|g| + eps)^2), so (stored, ref, bound) for ``ratio`` -- the
    printed ratio is the share of the accumulation bound the kernel's summation actually used."""
    Ch = zg.shape[1]
    g = gates[:, 2 * Ch:3 * Ch]
    m = g.abs() <= 0.75
    zm = torch.atanh(g[m])
    eps = torch.maximum(eps_tanh(zg[m]), eps_tanh(zm))
    return zm, zg[m], e_acc[m] + eps / (1 - (g[m].abs() + eps) ** 2)


def audit(geo: Geo, Ws: Sequence[torch.Tensor], bs: Sequence[Optional[torch.Tensor]], st: Dict[str, object],
          dh_T: Sequence[Optional[torch.Tensor]], dc_T: Sequence[Optional[torch.Tensor]], has_init: bool,
          fwd_ts: Optional[Sequence[int]] = None, t_min: int = 0) -> Dict[str, float]:
    """max(|stored - ref| / bound) per tensor kind ('gates', 'c', 'h', 'dG', 'dx', 'dh_init', 'dc_init'; with f32 storage also
    'zacc', the gate pre-activation's accumulation measured through the stash: _z_from_stash) over the forward
    launches of the time steps fwd_ts (None: all) and the backward launches of t_min .. T-1.  dh_T / dc_T: the state
    gradients stored before the backward (None: zero, as zero_state_grads).  st from an inference workspace (st['gates'] and
    st['dG'] None): the forward's c and h only."""
    B, T, L = geo.B, geo.T, len(geo.layers)
    sl = lambda t: slice(t * B, (t + 1) * B)
    worst: Dict[str, float] = {}

    def note(kind, stored, ref, bound):
        r = float(ratio(stored.double(), ref, bound).max())
        worst[kind] = max(worst.get(kind, 0.0), r)

    for t in (range(T) if fwd_ts is None else fwd_ts):
        for l in range(L):
            x_in = (st["x"][sl(t)] if l == 0 else st["h"][l - 1][sl(t + 1)]).double()
            zero = t == 0 and not has_init
            res = fwd_launch(geo, l, x_in, None if zero else st["h"][l][sl(t)].double(), None if zero else st["c"][l][sl(t)].double(),
                             Ws[l], bs[l])
            if st["gates"] is not None:
                note("gates", st["gates"][l][sl(t)], *res["gates"])
            note("c", st["c"][l][sl(t + 1)], *res["c"])
            note("h", st["h"][l][sl(t + 1)], *res["h"])
            if geo.u_et == 0.0 and st["gates"] is not None:
                note("zacc", *_z_from_stash(st["gates"][l][sl(t)].double(), *res["zg"]))
    if st["dG"] is None:                     # an inference workspace: no stash, no BPTT
        return worst
    for name, key, ref, bound in bwd_chain(geo, Ws, st["dG"], st["gates"], st["c"], dh_T, dc_T, t_min=t_min,
                                           has_init=has_init, need_dx=st.get("dx") is not None):
        if name == "dG":
            l, t = key
            note("dG", st["dG"][l][sl(t)], ref, bound)
        elif name == "dx":
            note("dx", st["dx"][sl(key)], ref, bound)
        else:
            note(name, st["dh_fin" if name == "dh_init" else "dc_fin"][key], ref, bound)
    return worst
