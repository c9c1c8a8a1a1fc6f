"""Which kernel body every gate and BPTT launch of a pass runs (TEST INFRASTRUCTURE ONLY; nothing in the product imports it).

A plain-Python restatement of the host arithmetic that picks each launch, in the style of ``wgrad_audit.exact_budget``: no GPU
calls, no library calls.  It restates

* ``cell_fwd`` (csrc/conv_igemm.hip): the VALU stencil kernel, the dense-K kernel (csrc/tiny_gemm.hip) or ``launch_conv``;
* ``launch_conv``: the K-steps, the 4-row rule (``mt4``), the small-batch rule ``2*N*tiles8 < 3*n_cu``, the column-split rule
  (``few4`` / ``few2`` of the gates, ``few(cols)`` of the dgrad launches) and the ntiles divisibility ladder 16/12/8/6/4/3/2/1;
* ``launch_cfg``: the merged leftover strip (8-row tiles, 1..4 leftover rows, two or more column tiles) and the grid size;
* ``nint_internal_conv_dgrad``: ``nt_begin`` and the n-tile count from ``need_dx`` / the fused forms;
* ``nint_internal_multi_plan``: which merged kernel holds a set of planned launches, or none;
* ``nint_seq_fwd`` / ``nint_seq_bwd`` (csrc/seq.hip): the wavefront grids, ``rows8``, ``fused[l]`` (K-steps <= 24 or the
  ``fuse_bwd`` mask), ``lo`` / ``loc``, ``merge`` / ``merge_d`` / ``merge_p``, the held-back bottom dgrad and the pointwise
  pass that rides behind the top layer's fused step.

A body is ``(DT, EPI, WN, WK, NTW, MT)`` -- the template arguments of ``conv_igemm_body`` -- with DT in {'bf16', 'f32'} and
EPI in {'LSTM', 'DGRAD', 'DGRAD_PW'}.  ``INSTANTIATED`` lists every body ``launch_conv`` instantiates (76).

``plan`` returns every launch of a forward (and, for training, backward) pass in enqueue order as ``Launch`` records: the
pass, the operation, the layer and time step, the host kernel that carries it (``conv_igemm`` for a direct launch,
``conv_lstm_multi[8]``, ``conv_bwd_multi[8]``, ``conv_dgrad_multi8``, ``stencil``, ``tiny``, ``pointwise``), the body, whether
the merged strip exists and the grid.  ``n_cu`` is an argument (256 on the MI355X), as are the engine's choices that the
library reads from the workspace (``wave``, ``fuse_bwd``, ``tile_rows``, ``need_dx``); ``default_wave`` restates
``SeqEngine._set_wave``.

The schedule half (``plan_fwd``, ``plan_bwd``, ``bwd_facts``, ``multi_kernel`` and the launch arithmetic they call) is checked against
the library: ``nint_debug_seq_plan`` runs the drivers' own planner on the host, and
``tests/test_launch_plan_cpu.py::test_ledger_equals_the_library_planner`` requires the two to agree record for record.  The two
stay independent statements of the same thing: this module calls nothing in the library.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

N_CU = 256
SPLIT_NUM = 3               # NINT_SPLIT_NUM
MULTI_MAX = 4               # NINT_MULTI_MAX
TINY_MAXSTEPS = 12          # NINT_TINY_MAXSTEPS
WAVE_TILES_PER_CU = 1.5     # engine.WAVE_TILES_PER_CU
EXPLICIT = 0x40000000       # nint_seq.fuse_bwd: explicit per-layer masks

# (WN, WK, NTW) of launch_conv's gate choices and of its dgrad ladder (n-tiles per workgroup = WN * NTW)
LSTM_SHAPES = ((4, 1, 4), (2, 2, 4), (1, 4, 4))
DGRAD_LADDER = ((16, (4, 1, 4)), (12, (4, 1, 3)), (8, (2, 2, 4)), (6, (2, 2, 3)), (4, (1, 4, 4)), (3, (1, 4, 3)),
                (2, (1, 4, 2)), (1, (1, 4, 1)))
INSTANTIATED = frozenset(
    [(dt, "LSTM", wn, wk, ntw, mt) for dt in ("bf16", "f32") for (wn, wk, ntw) in LSTM_SHAPES for mt in (4, 8)]
    + [(dt, epi, wn, wk, ntw, mt) for dt in ("bf16", "f32") for epi in ("DGRAD", "DGRAD_PW")
       for _, (wn, wk, ntw) in DGRAD_LADDER for mt in (4, 8)])

# nint_internal_multi_plan: the (EPI, WN, WK, NTW, MT) the merged kernels hold (the union of the library's case lists, restated)
MULTI_HOLDS = frozenset([("LSTM", 4, 1, 4, 8), ("LSTM", 2, 2, 4, 8), ("LSTM", 1, 4, 4, 8), ("LSTM", 4, 1, 4, 4),
                         ("LSTM", 2, 2, 4, 4), ("LSTM", 1, 4, 4, 4), ("DGRAD", 1, 4, 4, 8), ("DGRAD", 1, 4, 4, 4),
                         ("DGRAD", 1, 4, 2, 4), ("DGRAD", 2, 2, 3, 8), ("DGRAD", 2, 2, 3, 4), ("DGRAD", 1, 4, 3, 4),
                         ("DGRAD_PW", 1, 4, 3, 8), ("DGRAD_PW", 1, 4, 3, 4)])
CARRIERS = ("conv_igemm", "conv_lstm_multi", "conv_lstm_multi8", "conv_bwd_multi", "conv_bwd_multi8", "conv_dgrad_multi8",
            "stencil", "tiny", "pointwise")


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def rup(a: int, b: int) -> int:
    return cdiv(a, b) * b


def kc_of(dt: str) -> int:
    return 32 if dt == "bf16" else 16


@dataclass(frozen=True)
class Layer:
    """nint_layer as SeqEngine fills it (LayerCfg.padded)"""
    Cx: int
    Ch: int
    k: int
    xfold: bool
    Cxp: int
    Ch16: int
    Chp: int


def xfold_pays(Cx: int, k: int, dt: str) -> bool:
    """nint_xfold_pays (csrc/pack_weights.hip)"""
    kc = kc_of(dt)
    return Cx > 0 and k > 1 and k % 2 == 1 and cdiv(k * Cx, kc) < cdiv(Cx, kc) * k


def layers_of(C: int, hidden: Sequence[int], ks: Sequence[int], dt: str, xfold: bool = True) -> List[Layer]:
    """SeqEngine's layers: layer 0 folded where nint_xfold_pays (engine.XFOLD = xfold)"""
    kc, out = kc_of(dt), []
    for l, (Ch, k) in enumerate(zip(hidden, ks)):
        Cx = C if l == 0 else hidden[l - 1]
        f = l == 0 and xfold and xfold_pays(Cx, k, dt)
        out.append(Layer(Cx, Ch, k, f, rup(k * Cx if f else Cx, kc), rup(Ch, 16), rup(Ch, kc)))
    return out


def default_wave(B: int, H: int, W: int, L: int, n_cu: int = N_CU) -> int:
    """SeqEngine._set_wave with FORCE_WAVE = None"""
    if L <= 1:
        return 0
    tiles8 = B * cdiv(W, 16) * cdiv(H, 8)
    return 5 if 2 * tiles8 < WAVE_TILES_PER_CU * n_cu else 4


def stencil_shape(ly: Layer) -> bool:
    """nint_stencil_shape (= nint_internal_stencil_holds)"""
    return ly.k == 3 and ly.Ch <= 8 and (3 * ly.Cx <= 64 if ly.xfold else ly.Cx <= 16)


def tiny_shape(ly: Layer, dt: str) -> bool:
    """nint_tiny_shape"""
    es = 2 if dt == "bf16" else 4
    xg = cdiv((3 * ly.Cx if ly.xfold else ly.Cx) * es, 16)
    hg = cdiv(ly.Ch * es, 16)
    ngx = (3 if ly.xfold else 9) * xg
    return stencil_shape(ly) and cdiv(ngx + 9 * hg, 4) <= TINY_MAXSTEPS


# ------------------------------------------------------------------------------ one conv_igemm launch
def xchg_rounds(epi: str, wk: int, ntw: int, mt: int) -> int:
    return 2 if (wk == 4 and mt == 4 and ntw % 2 == 0) else (4 if (wk == 4 and mt == 8 and ntw == 4) else 1)


@dataclass(frozen=True)
class Conv:
    """A planned conv_igemm launch: its body, merged strip, grid (gx, gy) and dynamic LDS bytes"""
    body: Tuple[str, str, int, int, int, int]
    strip: bool
    gx: int
    gy: int
    lds: int

    @property
    def variant(self):
        return self.body[1:]


def launch_cfg(dt: str, epi: str, shape: Tuple[int, int, int], mt: int, k: int, nchunks: int, N: int, H: int, W: int,
               ngroups: int) -> Conv:
    """launch_cfg: the merged leftover strip, the grid and the LDS budget (an AssertionError where the C++ returns NINT_E_LDS)"""
    wn, wk, ntw = shape
    p = k // 2
    nhp_pad = rup((mt + 2 * p) * (16 + 2 * p), 16)
    tiles_x, tiles_y = cdiv(W, 16), cdiv(H, mt)
    left = H % mt
    merge = mt >= 8 and 1 <= left <= mt // 2 and tiles_x >= 2
    tiles_full_y = H // mt if merge else tiles_y
    tiles_x2 = cdiv(tiles_x, 2) if merge else 0
    nhp_max = max(nhp_pad, rup((mt // 2 + 2 * p) * (32 + 2 * p), 16) if merge else 0)
    chunk_bytes = 4 * nhp_max * 16
    red = wn * wk * (mt - mt // wk) * (ntw // xchg_rounds(epi, wk, ntw, mt)) * 1024 if wk > 1 else 0
    cpf = min(max((72 * 1024) // chunk_bytes, 1), nchunks)
    cpf = cdiv(nchunks, cdiv(nchunks, cpf))
    lds = max(cpf * chunk_bytes, red)
    assert lds <= 160 * 1024, ("NINT_E_LDS", dt, epi, shape, mt, k)
    return Conv((dt, epi, wn, wk, ntw, mt), merge, N * tiles_x * tiles_full_y + N * tiles_x2, ngroups, lds)


def launch_conv(dt: str, epi: str, ksteps: int, ntiles: int, tile_rows: int, k: int, nchunks: int, N: int, H: int, W: int,
                n_cu: int = N_CU) -> Optional[Conv]:
    """launch_conv: tile_rows is ConvArgs.tile_rows (0, 4 or 8); None = nothing launched (ntiles <= 0)"""
    if ntiles <= 0:
        return None
    if tile_rows:
        mt4 = tile_rows == 4
    else:
        mt4 = ksteps <= 32 if epi != "LSTM" else (ksteps <= 48 or ntiles <= 4)
        if 2 * N * cdiv(W, 16) * cdiv(H, 8) < 3 * n_cu:         # few images: 4-row tiles double the workgroups
            mt4 = True
    mt = 4 if mt4 else 8
    ptiles = N * cdiv(W, 16) * cdiv(H, mt)
    cfg = lambda shape, groups: launch_cfg(dt, epi, shape, mt, k, nchunks, N, H, W, groups)
    if epi == "LSTM":
        assert ntiles % 4 == 0, "NINT_E_SHAPE"
        cbs = ntiles // 4
        few4 = not tile_rows and 2 * ptiles * max(cbs // 4, 1) < SPLIT_NUM * n_cu
        few2 = not tile_rows and 2 * ptiles * max(cbs // 2, 1) < SPLIT_NUM * n_cu
        if cbs % 4 == 0 and not few4:
            return cfg((4, 1, 4), cbs // 4)
        if cbs % 2 == 0 and not few2:
            return cfg((2, 2, 4), cbs // 2)
        return cfg((1, 4, 4), cbs)
    for cols, shape in DGRAD_LADDER:
        few = not tile_rows and epi == "DGRAD" and 2 * ptiles * (ntiles // cols) < SPLIT_NUM * n_cu
        if ntiles % cols == 0 and (cols == 1 or not few):
            return cfg(shape, ntiles // cols)
    raise AssertionError("unreachable")


def gate_launch(ly: Layer, dt: str, N: int, H: int, W: int, tile_rows: int, with_h: bool, n_cu: int = N_CU):
    """cell_fwd: ('stencil' | 'tiny', None) or ('conv_igemm', Conv).  tile_rows = nint_layer.tile_rows (0, 1, 2, 4, 8)"""
    if stencil_shape(ly) and tile_rows == 1:                      # (NINT_STENCIL_AUTO is false for both types)
        return "stencil", None
    if (tile_rows == 2 or (tile_rows == 0 and dt == "f32")) and tiny_shape(ly, dt):    # NINT_TINY_AUTO: f32
        return "tiny", None
    kc = kc_of(dt)
    n0, n1 = ly.Cxp // kc, (ly.Chp // kc if with_h else 0)
    ksteps = n0 * ly.k * (1 if ly.xfold else ly.k) + n1 * ly.k * ly.k
    return "conv_igemm", launch_conv(dt, "LSTM", ksteps, 4 * ly.Ch16 // 16, tile_rows if tile_rows > 2 else 0, ly.k, n0 + n1,
                                     N, H, W, n_cu)


def dgrad_launch(ly: Layer, dt: str, N: int, H: int, W: int, tile_rows: int, dx: bool, dh_prev: bool,
                 pw: Optional[dict] = None, n_cu: int = N_CU) -> Tuple[int, Optional[Conv]]:
    """nint_internal_conv_dgrad: (nt_begin, Conv or None).  pw: None (EPI_DGRAD) or {'gates': bool, 'tile_rows': int}
    (EPI_DGRAD_PW: gates = the layer's own pointwise backward on the h columns; False = only the layer below's, on x)"""
    if not dx and not dh_prev and pw is None:
        return 0, None
    kc = kc_of(dt)
    tr = tile_rows if tile_rows > 2 else 0
    if pw is not None and pw.get("tile_rows"):
        tr = pw["tile_rows"]
    nchunk0 = 4 * ly.Ch16 // kc
    nt_x = ly.Cxp // 16
    nt_h = ly.Ch16 // 16 if (pw is not None and pw["gates"]) else ly.Chp // 16
    nt_begin = 0 if dx else nt_x
    ntiles = (nt_x if dx else 0) + (nt_h if (dh_prev or (pw is not None and pw["gates"])) else 0)
    epi = "DGRAD" if pw is None else "DGRAD_PW"
    return nt_begin, launch_conv(dt, epi, nchunk0 * ly.k * ly.k, ntiles, tr, ly.k, nchunk0, N, H, W, n_cu)


def multi_kernel(convs: Sequence[Conv], pw: bool = False) -> Optional[str]:
    """nint_internal_multi_plan: the merged kernel that holds these planned launches (pw: plus a pointwise pass), or None
    (NINT_E_SHAPE: the caller enqueues them one by one).  The library takes the first kernel whose case list holds them all;
    this states the same choice by its consequences, and tests/test_launch_plan_cpu.py compares the two on every list."""
    vs = [c.variant for c in convs]
    if not 1 <= len(vs) <= MULTI_MAX or any(v not in MULTI_HOLDS for v in vs):
        return None
    nfwd = sum(v[0] == "LSTM" for v in vs)
    if nfwd not in (0, len(vs)) or (pw and nfwd):
        return None
    rows8 = any(v[4] == 8 for v in vs)
    dpair = any(v == ("DGRAD", 2, 2, 3, 8) for v in vs)
    if rows8 and any(v in (("DGRAD", 2, 2, 3, 4), ("DGRAD", 1, 4, 3, 4)) for v in vs):
        return None
    if dpair and any(v not in (("DGRAD", 2, 2, 3, 8), ("DGRAD", 1, 4, 4, 8)) for v in vs):
        return None
    if pw and (rows8 or dpair):
        return None
    if dpair:
        return "conv_dgrad_multi8"
    if nfwd:
        return "conv_lstm_multi8" if rows8 else "conv_lstm_multi"
    return "conv_bwd_multi8" if rows8 else "conv_bwd_multi"


# ------------------------------------------------------------------------------ whole passes
@dataclass(frozen=True)
class Launch:
    pass_: str                # 'fwd' | 'bwd'
    op: str                   # 'gate' | 'dgrad' (EPI_DGRAD, or the classic-layer lo form) | 'fused' | 'pointwise'
    layer: int
    t: int                    # the time step of the launch's own data (a fused step of time u: u)
    kernel: str               # one of CARRIERS
    body: Optional[Tuple[str, str, int, int, int, int]] = None
    strip: bool = False
    grid: Optional[Tuple[int, int]] = None
    nt_begin: int = 0


@dataclass(frozen=True)
class BwdFacts:
    fused: Tuple[bool, ...]
    lo: Tuple[bool, ...]
    loc: Tuple[bool, ...]
    off: Tuple[int, ...]
    merge: bool
    merge_d: bool
    merge_p: bool


def bwd_facts(lys: Sequence[Layer], dt: str, wave: int, fuse_bwd: int, wg_room: bool = True) -> BwdFacts:
    """the per-layer facts of nint_seq_bwd.  wg_room: wg_partial_bytes >= the bottom layer's dh slab (merge_d needs it)"""
    L, kc = len(lys), kc_of(dt)
    explicit = (fuse_bwd & EXPLICIT) != 0
    fused, off = [False] * L, [0] * L
    for l in range(L - 1, -1, -1):
        ksteps = (4 * lys[l].Ch16 // kc) * lys[l].k * lys[l].k
        fused[l] = ((fuse_bwd >> l) & 1) != 0 if explicit else (fuse_bwd == 2 or (fuse_bwd == 0 and ksteps <= 24))
        off[l] = (0 if l == L - 1 else off[l + 1]) + int(fused[l])
    lo = [fused[l] and l > 0 and not fused[l - 1] and (((fuse_bwd >> (8 + l)) & 1) != 0 if explicit else True) for l in range(L)]
    loc = [not fused[l] and l > 0 and not fused[l - 1] and explicit and ((fuse_bwd >> (16 + l)) & 1) != 0 for l in range(L)]
    merge = wave in (1, 3) and L >= 3 and fused[L - 1] and not fused[0] and not loc[0]
    merge_d = (wave in (4, 5) and L >= 2 and not fused[0] and not fused[1] and not loc[0] and not loc[1] and wg_room)
    merge_p = merge_d and L >= 3 and fused[L - 1]
    return BwdFacts(tuple(fused), tuple(lo), tuple(loc), tuple(off), merge, merge_d, merge_p)


def _rec(pass_, op, l, t, kernel, conv: Optional[Conv], nt_begin=0) -> Launch:
    if conv is None:
        return Launch(pass_, op, l, t, kernel)
    return Launch(pass_, op, l, t, kernel, conv.body, conv.strip, (conv.gx, conv.gy), nt_begin)


def plan_fwd(lys: Sequence[Layer], dt: str, B: int, T: int, H: int, W: int, wave: int, tile_rows: int = 0,
             has_init: bool = False, n_cu: int = N_CU) -> List[Launch]:
    """nint_seq_fwd (training and inference alike: the stash pointer changes no launch shape)"""
    L, out = len(lys), []
    rows8 = wave in (2, 3, 4) and 1 < L <= MULTI_MAX

    def one(l, t):
        tr = 8 if (rows8 and tile_rows == 0) else tile_rows
        return gate_launch(lys[l], dt, B, H, W, tr, t > 0 or has_init, n_cu)

    if wave and 1 < L <= MULTI_MAX:
        for w in range(T + L - 1):
            lt = [(l, w - l) for l in range(L) if 0 <= w - l < T]
            launched = [one(l, t) for l, t in lt]
            kern = None
            if len(lt) > 1 and all(k == "conv_igemm" for k, _ in launched):
                kern = multi_kernel([c for _, c in launched])
            for (l, t), (k, c) in zip(lt, launched):
                out.append(_rec("fwd", "gate", l, t, kern or k, c))
        return out
    for t in range(T):
        for l in range(L):
            k, c = one(l, t)
            out.append(_rec("fwd", "gate", l, t, k, c))
    return out


def plan_bwd(lys: Sequence[Layer], dt: str, B: int, T: int, H: int, W: int, wave: int, tile_rows: int = 0,
             fuse_bwd: int = 0, need_dx: bool = False, has_init: bool = False, wg_room: bool = True,
             n_cu: int = N_CU) -> List[Launch]:
    """nint_seq_bwd's BPTT chain (the weight-gradient reductions after it are not conv_igemm launches)"""
    L = len(lys)
    f = bwd_facts(lys, dt, wave, fuse_bwd, wg_room)
    out: List[Launch] = []
    pw_done = [-1] * L
    pend = None                 # the held-back bottom dgrad: (u, nt_begin, Conv)
    pend_pw = None              # the held-back bottom pointwise pass: its time step

    def dg(l, dx, dh, pw=None):
        return dgrad_launch(lys[l], dt, B, H, W, tile_rows, dx, dh, pw, n_cu)

    def flush():
        nonlocal pend
        if pend is not None:
            u, nb, c = pend
            out.append(_rec("bwd", "dgrad", 0, u, "conv_igemm", c, nb))
            pend = None

    def flush_pw():
        nonlocal pend_pw
        if pend_pw is not None:
            out.append(Launch("bwd", "pointwise", 0, pend_pw, "pointwise"))
            pend_pw = None

    for so in range(T - 1, -f.off[0] - 1, -1):
        for l in range(L - 1, -1, -1):
            u = so + f.off[l]
            if u < 0 or u > (T if f.fused[l] else T - 1):
                continue
            if pend_pw is not None and not (l == L - 1 and 1 <= u < T):
                flush_pw()

            def pointwise(t):
                nonlocal pend_pw
                if not f.merge_d or l == 0:
                    flush()
                if f.merge_p and l == 0 and so + f.off[L - 1] >= 2:
                    pend_pw = t
                    return
                out.append(Launch("bwd", "pointwise", l, t, "pointwise"))

            dx = l > 0 or need_dx
            dh = not (u == 0 and not has_init)
            if not f.fused[l]:
                if pw_done[l] != u:
                    pointwise(u)
                pw = None
                if f.loc[l]:
                    pw = {"gates": False, "tile_rows": 4}
                    pw_done[l - 1] = u
                if f.merge_d and l == 1 and pend is not None:
                    nb, c = dg(l, dx, dh)
                    kern = multi_kernel([pend[2], c]) if c is not None else None
                    if kern:
                        out.append(_rec("bwd", "dgrad", 0, pend[0], kern, pend[2], pend[1]))
                        out.append(_rec("bwd", "dgrad", l, u, kern, c, nb))
                        pend = None
                        continue
                if not f.merge_d or l <= 1:
                    flush()
                if (f.merge or f.merge_d) and l == 0 and so > -f.off[0]:
                    nb, c = dg(0, dx, dh)
                    pend = (u, nb, c) if c is not None else None
                    continue
                nb, c = dg(l, dx, dh, pw)
                if c is not None:
                    out.append(_rec("bwd", "dgrad", l, u, "conv_igemm", c, nb))
            elif u == T:
                pointwise(T - 1)
            elif u >= 1:
                pw = {"gates": True, "tile_rows": 0}
                if f.lo[l]:
                    pw_done[l - 1] = u
                if f.merge and pend is not None and l == L - 1:
                    if wave == 3:
                        pw["tile_rows"] = 8
                    nb, c = dg(l, dx, False, pw)
                    kern = multi_kernel([pend[2], c]) if c is not None else None
                    if kern:
                        out.append(_rec("bwd", "dgrad", 0, pend[0], kern, pend[2], pend[1]))
                        out.append(_rec("bwd", "fused", l, u, kern, c, nb))
                        pend = None
                        continue
                if not f.merge_d:
                    flush()
                if pend_pw is not None:
                    nb, c = dg(l, dx, False, pw)
                    kern = multi_kernel([c], pw=True) if c is not None else None
                    if kern:
                        out.append(_rec("bwd", "fused", l, u, kern, c, nb))
                        out.append(Launch("bwd", "pointwise", 0, pend_pw, kern))
                        pend_pw = None
                        continue
                    flush_pw()
                nb, c = dg(l, dx, False, pw)
                out.append(_rec("bwd", "fused", l, u, "conv_igemm", c, nb))
            else:
                if not f.merge_d:
                    flush()
                nb, c = dg(l, dx, dh)
                if c is not None:
                    out.append(_rec("bwd", "dgrad", l, 0, "conv_igemm", c, nb))
    flush_pw()
    flush()
    return out


def plan(C: int, hidden: Sequence[int], ks: Sequence[int], B: int, T: int, H: int, W: int, dt: str,
         wave: Optional[int] = None, tile_rows: int = 0, fuse_bwd: int = 0, need_dx: bool = False, train: bool = True,
         has_init: bool = False, xfold: bool = True, wg_room: bool = True, n_cu: int = N_CU) -> List[Launch]:
    """Every gate and BPTT launch of one forward (+ backward when train) pass of the stack C -> hidden with kernel sizes ks,
    as SeqEngine runs it.  wave None: SeqEngine's choice by batch size; tile_rows: engine.FORCE_TILE_ROWS (every layer)."""
    lys = layers_of(C, hidden, ks, dt, xfold)
    L = len(lys)
    if wave is None:
        wave = default_wave(B, H, W, L, n_cu)
    wave = wave if L > 1 else 0
    out = plan_fwd(lys, dt, B, T, H, W, wave, tile_rows, has_init, n_cu)
    if train:
        out += plan_bwd(lys, dt, B, T, H, W, wave, tile_rows, fuse_bwd, need_dx, has_init, wg_room, n_cu)
    return out


def bodies(launches: Sequence[Launch]) -> Dict[Tuple, set]:
    """body -> the set of (kernel, merged strip) pairs that ran it"""
    d: Dict[Tuple, set] = {}
    for x in launches:
        if x.body is not None:
            d.setdefault(x.body, set()).add((x.kernel, x.strip))
    return d


def fmt_body(b) -> str:
    return "<%s,%s,%d,%d,%d,%d>" % b


# ------------------------------------------------------------------------------ the reachable set
SWEEP_DIMS = dict(Cx=range(1, 129), Ch=range(4, 129), k=(1, 3, 5, 7, 9), N=range(1, 33), tile_rows=(0, 4, 8))


def reachable(n_cu: int = N_CU, geoms: Sequence[Tuple[int, int]] = ((100, 154), (37, 50), (16, 16), (9, 40))) -> Dict[Tuple, set]:
    """body -> the merged-strip values it is launched with, over every layer shape the engine accepts (Cx 1..128, Ch 4..128,
    k in {1, 3, 5, 7, 9}, folded where it pays or plain), every launch form a schedule can give it (gate with / without the h
    half; dgrad with x and / or h columns; fused with / without x columns; a classic layer carrying the layer below's
    pointwise pass), N 1..32 on a few pixel grids and tile_rows 0 / 4 / 8 (what FORCE_TILE_ROWS, rows8, wave 3 and the lo
    form pin).  launch_conv reads the K-steps only through ksteps <= 32 / <= 48 and k only through the LDS budget (never
    exceeded: at most ~72 KiB of halo image and 64 KiB of exchange buffer), so the forms are collected as (K-step class,
    ntiles) first and each class is launched with its largest K-step count and kernel size: the sweep takes about a second."""
    forms: Dict[Tuple, Tuple[int, int, int]] = {}

    def add(dt, epi, ksteps, ntiles, nchunks, k):
        key = (dt, epi, 0 if ksteps <= 32 else (1 if ksteps <= 48 else 2), ntiles)
        forms[key] = max(forms.get(key, (0, 0, 0)), (ksteps, k, nchunks))

    for dt in ("bf16", "f32"):
        kc = kc_of(dt)
        for k in SWEEP_DIMS["k"]:
            for Cx in SWEEP_DIMS["Cx"]:
                for fold in (False, True):
                    if fold and not xfold_pays(Cx, k, dt):
                        continue
                    Cxp = rup(k * Cx if fold else Cx, kc)
                    n0, nt_x = Cxp // kc, Cxp // 16
                    ks_x = n0 * k * (1 if fold else k)
                    for Ch16, Chp in sorted({(rup(Ch, 16), rup(Ch, kc)) for Ch in SWEEP_DIMS["Ch"]}):
                        n1, nd = Chp // kc, 4 * Ch16 // kc
                        for wh in (0, 1):                                       # gate: zero state / with h
                            add(dt, "LSTM", ks_x + wh * n1 * k * k, 4 * Ch16 // 16, n0 + wh * n1, k)
                        for nt in (nt_x + Chp // 16, nt_x, Chp // 16):          # dgrad: dx + dh / dx only / dh only
                            add(dt, "DGRAD", nd * k * k, nt, nd, k)
                        for nt in (nt_x + Ch16 // 16, Ch16 // 16, nt_x + Chp // 16):    # fused with / without x; loc
                            add(dt, "DGRAD_PW", nd * k * k, nt, nd, k)
    out: Dict[Tuple, set] = {}
    ptile_geoms = [(N, H, W) for N in SWEEP_DIMS["N"] for H, W in geoms]
    for (dt, epi, _, ntiles), (ksteps, k, nchunks) in forms.items():
        for tr in SWEEP_DIMS["tile_rows"]:
            for N, H, W in ptile_geoms:
                c = launch_conv(dt, epi, ksteps, ntiles, tr, k, nchunks, N, H, W, n_cu)
                out.setdefault(c.body, set()).add(c.strip)
    return out


# bodies launch_conv instantiates that no launch can select, and why
UNREACHABLE = {
    ("bf16", "DGRAD", 1, 4, 1, 8):
        "bf16 dgrad n-tile counts are even (Cxp and Chp are multiples of 32), so a 1-column shape needs the column split of "
        "ntiles = 2; at 8-row tiles the split never happens: without a pinned tile_rows 8 rows mean 2*N*tiles8 >= 3*n_cu, "
        "so 2*ptiles*(ntiles/cols) >= 3*n_cu, and a pinned tile_rows disables the split",
    ("bf16", "DGRAD", 1, 4, 3, 8):
        "an even bf16 n-tile count divisible by 3 is divisible by 6 and takes (2, 2, 3) unless split, and 8-row tiles are "
        "never split (as above)",
}


def case_launches(C, hidden, ks, B, T, H, W, dtype, wave=None, rows=0, fuse=None, has_init=False, need_dx=True, train=True,
                  fwd_ts=None, t_min=0, n_cu=N_CU, **_) -> List[Launch]:
    """The launches of one tests/test_gpu_*_audit.py run_audit case (its keyword arguments) whose stored outputs the audit
    checks: gate launches of the time steps fwd_ts (None: all), BPTT launches of time u > t_min (with t_min = 0: all) --
    a launch of time u writes dG or d/dh of time u - 1."""
    out = plan(C, hidden, ks, B, T, H, W, dtype, wave=wave, tile_rows=rows, fuse_bwd=0 if fuse is None else fuse,
               need_dx=need_dx, train=train, has_init=has_init, n_cu=n_cu)
    return [x for x in out if (x.t in fwd_ts if fwd_ts is not None else True) or x.pass_ == "bwd"
            if x.pass_ == "fwd" or t_min == 0 or x.t > t_min]
