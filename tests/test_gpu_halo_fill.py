"""GPU: the halo-tile fill of the conv kernels (csrc/conv_igemm.hip: lanes 4j..4j+3 load the four 16-byte quarters of pixel j's
64-byte chunk, 16 pixels a piece, and write them to the four g planes of the LDS image) at the smallest shapes where the
lane -> (pixel, quarter, chunk) mapping can go wrong: a 12 x 20 grid (one full 8-row tile row plus the merged 4 x 32 strip, W no
multiple of 16, pad pixels since the halo tile's pixel count is no multiple of 16) and a single 8 x 16 tile, B = 1 and 2, tile
rows pinned to 4 and to 8, on the bench stack's three layers (62 -> 64 k 5: 2 + 2 chunks, two fills of the dgrad image;
64 -> 32 k 3: 3 chunks; 32 -> 16 k 3), a horizontally folded layer (5 -> 64 k 5) and a k = 7 layer.

Data are small integers (|v| <= 4), so every f32 sum is exact whatever the order of its terms:
  * dgrad: nint_conv_dgrad must EQUAL a NumPy transposed convolution element for element (bf16 outputs: the exact integer
    rounded to bf16 once).  Two sources: random integers, and all ones inside the image -- there only the slab's zero ring tells
    pixels apart, so a piece that read the wrong pixel shows up as a wrong count.
  * gate kernel: weights are integers in units of 2^-7 (pre-activations exact, |z| of a few units so that the gates do not
    saturate); h, c and the stash against oracle/convlstm_oracle.py at the tolerances of tests/test_gpu_parity.py (f32: rtol
    1e-4 / atol 1e-5; bf16: rel-L2 2e-2).
  * tile rows 4 against 8, forward and dgrad, at the tolerance test_forward_wavefront_rule_and_fallback uses for the two
    heights (rel-L2 1e-3).
Launched one by one, the 8-row bodies of four column tiles per wave stage the tile through registers and the others fill it by
LDS-DMA (conv_igemm_body's FILL): both forms of the same image are held to the same references here.  The merged grids, where
every body stages, are held to these launches bit for bit by tests/test_gpu_shapes.py."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

#          name: (Cx, Ch, k, folded)
LAYERS = {"l0_62_64_k5": (62, 64, 5, False), "l1_64_32_k3": (64, 32, 3, False), "l2_32_16_k3": (32, 16, 3, False),
          "xfold_5_64_k5": (5, 64, 5, True), "k7_16_16": (16, 16, 7, False)}
GRIDS = [(12, 20, 2), (12, 20, 1), (8, 16, 1), (8, 16, 2)]          # H, W, B


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


def _engine(layer, dtype, rows):
    """a one-layer engine with the tile height pinned"""
    from nasa_niswan_amd import engine
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    Cx, Ch, k, fold = LAYERS[layer]
    old = engine.FORCE_TILE_ROWS, engine.XFOLD
    engine.FORCE_TILE_ROWS, engine.XFOLD = rows, fold
    try:
        eng = SeqEngine([LayerCfg(Cx, Ch, k)], dtype, "cuda")
    finally:
        engine.FORCE_TILE_ROWS, engine.XFOLD = old
    assert bool(eng.cfgs[0].xfold) == fold and eng.layers[0].tile_rows == rows
    return eng


def _ints(rng, shape, lim=4):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _dgrad_case(layer, H, W, B):
    """integer weights and the two dG sources with their exact transposed convolutions, computed once per shape:
    d cat[b, c, y, x] = sum_{o,u,v} W[o, c, u, v] * dG[b, o, y - u + p, x - v + p]        (autograd of model.py:220)"""
    Cx, Ch, k, _ = LAYERS[layer]
    p = k // 2
    rng = np.random.default_rng(zlib.crc32(repr((layer, H, W, B, "dgrad")).encode()))
    Wt = _ints(rng, (4 * Ch, Cx + Ch, k, k))
    out = {"W": Wt}
    for style in ("random", "ones"):
        dG = _ints(rng, (B, 4 * Ch, H, W)) if style == "random" else np.ones((B, 4 * Ch, H, W))
        pad = np.zeros((B, 4 * Ch, H + 2 * p, W + 2 * p))
        pad[:, :, p:p + H, p:p + W] = dG
        d = np.zeros((B, Cx + Ch, H, W))
        for u in range(k):
            for v in range(k):
                win = pad[:, :, 2 * p - u:2 * p - u + H, 2 * p - v:2 * p - v + W]
                d += np.tensordot(Wt[:, :, u, v], win, axes=([0], [1])).transpose(1, 0, 2, 3)
        assert np.abs(d).max() < 2 ** 24              # every partial sum is an exact f32
        out[style] = (dG, d)
    return out


def _run_dgrad(pkg, eng, layer, H, W, B, dG):
    """nint_conv_dgrad of one integer source -> (dx or None, dh) as (B, C, H, W) f32, and the padding columns' largest magnitude"""
    from oracle import stored_audit as SA
    from nasa_niswan_amd._lib import NintGeom
    lib = pkg.load_library()
    Cx, Ch, k, fold = LAYERS[layer]
    geo = SA.Geo.make(B, 1, H, W, [(Cx, Ch, k, fold)], eng.es)
    g = NintGeom()
    assert lib.nint_geom_make(C.byref(g), H, W, eng.P) == 0
    assert (g.Hh, g.Wh, g.P) == (geo.Hh, geo.Wh, geo.P)
    ly, lg = eng.layers[0], geo.layers[0]
    slab = SA.write_dG(geo, 0, torch.from_numpy(dG).float()).cuda()
    et = geo.et
    dx = None if fold else torch.zeros(B * H * W * lg.Cxp, device="cuda", dtype=et)      # (a folded input takes no gradient here)
    dh = torch.zeros(B * H * W * lg.Chp, device="cuda", dtype=et)
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert lib.nint_conv_dgrad(C.byref(ly), C.byref(g), eng.dt, B, vp(slab), vp(dx) if dx is not None else None, vp(dh), None) == 0
    torch.cuda.synchronize()
    padmax = 0.0
    res = []
    for buf, c, cp in ((dx, Cx, lg.Cxp), (dh, Ch, lg.Chp)):
        if buf is None:
            res.append(None)
            continue
        full = buf.cpu().view(B, H, W, cp).float()
        if cp > c:
            padmax = max(padmax, float(full[..., c:].abs().max()))
        res.append(full[..., :c].permute(0, 3, 1, 2).contiguous())
    return res[0], res[1], padmax


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("H,W,B", GRIDS)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_dgrad_equals_numpy_transposed_convolution_on_integers(pkg, layer, H, W, B, dtype):
    Cx, Ch, k, fold = LAYERS[layer]
    case = _dgrad_case(layer, H, W, B)
    et = torch.bfloat16 if dtype == "bf16" else torch.float32
    by_rows = {}
    for rows in (4, 8):
        eng = _engine(layer, dtype, rows)
        eng.pack_weights([torch.from_numpy(case["W"]).float().cuda()], [None])
        for style in ("random", "ones"):
            dG, d = case[style]
            want = torch.from_numpy(d).float().to(et).float()           # exact integers, rounded once where the output is bf16
            dx, dh, padmax = _run_dgrad(pkg, eng, layer, H, W, B, dG)
            bad_h = int((dh != want[:, Cx:]).sum())
            bad_x = 0 if dx is None else int((dx != want[:, :Cx]).sum())
            print(f"  {layer} {H}x{W} B={B} {dtype} rows {rows} {style}: dh {bad_h} / {dh.numel()} differ, "
                  f"dx {bad_x} differ, padding columns max {padmax}")
            assert bad_h == 0 and bad_x == 0 and padmax == 0.0, (rows, style, bad_h, bad_x, padmax)
            by_rows[rows, style] = (dx, dh)
    # tile rows 4 against 8 (the bound the forward wavefront test holds the two heights to)
    for style in ("random", "ones"):
        for a, b in zip(by_rows[4, style], by_rows[8, style]):
            if a is not None:
                assert float((a - b).norm()) <= 1e-3 * float(b.norm())


@functools.lru_cache(maxsize=None)
def _gate_case(layer, H, W, B):
    """integer x, h, c (c in quarters), weights and bias in units of 2^-7, and the oracle's step in f64"""
    from oracle import convlstm_oracle as O
    Cx, Ch, k, _ = LAYERS[layer]
    rng = np.random.default_rng(zlib.crc32(repr((layer, H, W, B, "gate")).encode()))
    Wt = _ints(rng, (4 * Ch, Cx + Ch, k, k)) / 128.0
    bias = _ints(rng, (4 * Ch,), 2) / 128.0
    x, h, c = _ints(rng, (B, Cx, H, W)), _ints(rng, (B, Ch, H, W)), _ints(rng, (B, Ch, H, W)) / 4.0
    t = lambda a: torch.from_numpy(a)
    z = torch.nn.functional.conv2d(torch.cat([t(x), t(h)], 1), t(Wt), t(bias), padding=k // 2)
    assert float(z.abs().max()) * 128 < 2 ** 24 and float(z.abs().median()) < 8       # exact in f32, and not saturated
    h1, c1, gates = O.cell_forward_stash(t(x), t(h), t(c), t(Wt), t(bias))
    return Wt, bias, x, h, c, h1, c1, torch.cat(gates, 1)


def _run_gate(eng, layer, H, W, B, case):
    from oracle import stored_audit as SA
    Wt, bias, x, h, c = case[:5]
    f = lambda a: torch.from_numpy(a).float().cuda()
    eng.pack_weights([f(Wt)], [f(bias)])
    ws = eng.acquire(B, 1, H, W, True, True)
    try:
        eng.forward(ws, f(x)[:, None].contiguous(), [f(h)], [f(c)])
        torch.cuda.synchronize()
        geo = SA.geo_of(eng, ws)
        return (SA.read_h(geo, 0, ws.h[0])[B:], SA.read_c(geo, 0, ws.c[0])[B:], SA.read_gates(geo, 0, ws.gates[0]))
    finally:
        eng.release(ws)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("H,W,B", GRIDS)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_gate_kernel_on_exact_preactivations(pkg, layer, H, W, B, dtype):
    case = _gate_case(layer, H, W, B)
    want = dict(zip(("h", "c", "stash"), case[5:]))
    by_rows = {}
    for rows in (4, 8):
        got = dict(zip(("h", "c", "stash"), _run_gate(_engine(layer, dtype, rows), layer, H, W, B, case)))
        by_rows[rows] = got
        for name in ("h", "c", "stash"):
            a, b = got[name].double(), want[name]
            assert a.shape == b.shape and bool(torch.isfinite(a).all()), (rows, name)
            err, rel = float((a - b).abs().max()), float((a - b).norm() / b.norm())
            print(f"  {layer} {H}x{W} B={B} {dtype} rows {rows} {name}: max abs err {err:.3e}, rel-L2 {rel:.3e}")
            if dtype == "f32":
                np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-4, atol=1e-5, err_msg=f"{name} rows {rows}")
            else:
                assert rel <= 2e-2, (rows, name, rel)
    for name in ("h", "c", "stash"):
        a, b = by_rows[4][name].double(), by_rows[8][name].double()
        assert float((a - b).norm()) <= 1e-3 * float(b.norm()), name
