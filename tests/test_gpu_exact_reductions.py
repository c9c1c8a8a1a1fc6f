"""The weight- and bias-gradient reductions on INTEGER data, checked bit for bit (oracle/wgrad_audit.py).

dG from {-1, 0, 1}, the x / h sources from {-2, ..., 2}: every product is an exact integer (bf16 x bf16 and the f32 MFMA alike)
and every partial sum an integer below 2^24 (WA.exact_budget), so any summation order gives the same f32 value and the
kernel's dW / db must EQUAL the f64 reference -- whatever the size of the reduction.  One dropped 4 x 32 pixel tile, a doubled
split, a swapped tap, an unflushed empty split or an h skip of the wrong length shows as a mismatch, where a tolerance on
1.5 M-term sums cannot see it.  Every destination and the split-K partial buffer start as NaN, so an element nobody wrote
shows too, and a second run must give identical bits (fixed fold order).

(a) nint_conv_wgrad directly, one case per reachable row (k, NTC, JW, KX) of wgrad.hip's instance table in both storage types, the
    folded x source, the 8-wave kernel, on ragged grids, with N = 1, and at the real geometries.
(b) layer 0's weight gradient as the product computes it: SeqEngine.backward(parts = 2) after a parts = 1 call, on slabs
    overwritten with integers -- the h source skipping the zero state (has_init = 0), a given initial state, T = B = 1.
(c) nint_head_bwd (dw, db and dh) through both of its weight-gradient paths.
"""
import ctypes as C
import time

import pytest
import torch

from oracle import convlstm_oracle as O
from oracle import stored_audit as SA
from oracle import wgrad_audit as WA

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    lib = p.load_library()
    t0 = time.time()
    yield lib
    print(f"\n  test_gpu_exact_reductions wall time {time.time() - t0:.1f} s")


def _n_cu(lib):
    n = C.c_int(0)
    lib.nint_device_info(C.byref(n), None, None, None, 0)
    return n.value


def _rup(a, b):
    return (a + b - 1) // b * b


def _diff(tag, out, ref):
    """bit-equality of an f32 result with the f64 reference, with where it differs when it does"""
    r = ref.float()
    if torch.equal(out, r):
        return
    bad = ~(out == r)
    idx = bad.nonzero()[:8].tolist()
    pytest.fail(f"{tag}: {int(bad.sum())} of {out.numel()} elements differ ({int(torch.isnan(out).sum())} NaN, never written); "
                f"first at {idx}: got {[float(out[tuple(i)]) for i in idx]}, want {[float(r[tuple(i)]) for i in idx]}")


# --------------------------------------------------------------------------------------------------- (a) nint_conv_wgrad
def _direct(lib, Cx, Ch, k, N, H, W, dtype, xfold=False, wide=0, seed=0):
    from nasa_niswan_amd import _lib
    from nasa_niswan_amd._lib import NINT_BF16, NINT_F32, NintGeom, NintLayer
    dt = NINT_BF16 if dtype == "bf16" else NINT_F32
    es = 2 if dtype == "bf16" else 4
    # T = N time steps of B = 1 image: nint_conv_wgrad pairs h image n with dG image n (no skip)
    geo = SA.Geo.make(1, N, H, W, [(Cx, Ch, k, xfold)], es)
    lg = geo.layers[0]
    g = NintGeom()
    _lib.check(lib.nint_geom_make(C.byref(g), H, W, geo.P), "nint_geom_make")
    assert (g.Hh, g.Wh, g.P) == (geo.Hh, geo.Wh, geo.P)
    ly = NintLayer()
    ly.Cx, ly.Cxp, ly.Ch, ly.Ch16, ly.Chp, ly.k, ly.xfold, ly.wide = Cx, lg.Cxp, Ch, lg.Ch16, lg.Chp, k, int(xfold), wide
    assert lg.Cxp == _rup(k * Cx if xfold else Cx, geo.kc)
    WA.exact_budget(N, H, W)
    gen = torch.Generator().manual_seed(seed)
    dG = WA.int_values((N, 4 * Ch, H, W), WA.DG_MAX, gen, "cuda")
    x = WA.int_values((N, Cx, H, W), WA.SRC_MAX, gen, "cuda")
    h = WA.int_values((N, Ch, H, W), WA.SRC_MAX, gen, "cuda")
    dG_s, xs, hs = SA.write_dG(geo, 0, dG), SA.write_xs(geo, x), SA.write_halo(geo, h, lg.Chp)
    n_cu = _n_cu(lib)
    nbytes = lib.nint_wgrad_workspace_bytes(C.byref(ly), dt, n_cu)
    assert nbytes > 0
    ref_W, ref_b = WA.wgrad_ref(dG, x, h, k, xfold=xfold, has_init=True, B=1)
    outs = []
    for _ in range(2):
        part = torch.full((nbytes // 4,), NAN, device="cuda")
        dW = torch.full((4 * Ch, Cx + Ch, k, k), NAN, device="cuda")
        db = torch.full((4 * Ch,), NAN, device="cuda")
        _lib.check(lib.nint_conv_wgrad(C.byref(ly), C.byref(g), dt, N, C.c_void_p(dG_s.data_ptr()), C.c_void_p(xs.data_ptr()),
                                       C.c_void_p(hs.data_ptr()), C.c_void_p(dW.data_ptr()), C.c_void_p(db.data_ptr()),
                                       C.c_void_p(part.data_ptr()), part.numel() * 4, n_cu, None), "nint_conv_wgrad")
        torch.cuda.synchronize()
        outs.append((dW, db))
    tag = f"{Cx}->{Ch} k{k} N={N} {H}x{W} {dtype} xfold={int(xfold)} wide={wide}"
    _diff(tag + " dW", outs[0][0], ref_W)
    _diff(tag + " db", outs[0][1], ref_b)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (tag, "not reproducible")
    print(f"  {tag}: dW, db bit-equal to the f64 sum (max |dW| {float(ref_W.abs().max()):.0f})", flush=True)


# (dtype, xfold, wide, Cx, Ch, k), named by the instance -- 4-wave (k, NTC, JW, KX) or 8-wave <k, NCT> -- it is there for:
# tests/test_wgrad_plan_cpu.py asks the planner that each case reaches it and that no reachable instance is left out
KEYS = {
    "bf16 (5,1,7,5) 62->64": ("bf16", False, 1, 62, 64, 5),
    "bf16 (3,2,5,3) 64->64": ("bf16", False, 1, 64, 64, 3),
    "bf16 (1,2,5,1) 64->32": ("bf16", False, 1, 64, 32, 1),
    "bf16 (7,1,7,7) 16->32 two column groups": ("bf16", False, 1, 16, 32, 7),
    "bf16 folded (5,2,5,1) 5->64": ("bf16", True, 1, 5, 64, 5),
    "bf16 folded (3,2,5,1) 5->32": ("bf16", True, 1, 5, 32, 3),
    "bf16 folded (7,2,5,1) 2->16": ("bf16", True, 1, 2, 16, 7),
    "f32 (5,1,7,5) 62->64": ("f32", False, 0, 62, 64, 5),
    "f32 (3,1,5,3) 48->48": ("f32", False, 0, 48, 48, 3),
    "f32 (1,1,5,1) 48->16": ("f32", False, 0, 48, 16, 1),
    "f32 (7,1,7,7) 16->16 two column groups": ("f32", False, 0, 16, 16, 7),
    "f32 (3,2,5,3) 64->64": ("f32", False, 0, 64, 64, 3),
    "f32 (1,2,5,1) 64->32": ("f32", False, 0, 64, 32, 1),
    "f32 folded (5,1,5,1) 3->32": ("f32", True, 0, 3, 32, 5),
    "f32 folded (3,1,5,1) 5->16": ("f32", True, 0, 5, 16, 3),
    "f32 folded (7,1,5,1) 2->16": ("f32", True, 0, 2, 16, 7),
    "f32 folded (5,2,5,1) 6->16": ("f32", True, 0, 6, 16, 5),
    "f32 folded (3,2,5,1) 10->16": ("f32", True, 0, 10, 16, 3),
    "f32 folded (7,2,5,1) 4->16": ("f32", True, 0, 4, 16, 7),
    "bf16 8-wave <3,4> 64->64": ("bf16", False, 2, 64, 64, 3),
    "bf16 8-wave <5,2> 62->64": ("bf16", False, 2, 62, 64, 5),
    "bf16 8-wave <7,1> 62->64": ("bf16", False, 2, 62, 64, 7),
}


@pytest.mark.parametrize("N", [7, 1])
@pytest.mark.parametrize("name", list(KEYS))
def test_every_dispatch_key_on_a_ragged_grid(lib, name, N):
    """37 x 50: neither a multiple of the tile rows (4 / 2) nor of 32 columns.  N = 7 gives 140 (bf16) / 266 (f32) pixel
    tiles; the split counts these launches plan on 256 CUs (16 of 9 tiles in bf16; 30 of 9 in f32, or 24 of 12 where the f32
    x and h sources share a launch and the count is rounded to a multiple of 8) leave the last split short or empty.  N = 1:
    20 / 38 tiles in 2 / 4 splits."""
    dtype, xfold, wide, Cx, Ch, k = KEYS[name]
    _direct(lib, Cx, Ch, k, N, 37, 50, dtype, xfold=xfold, wide=wide, seed=N)


REAL = {
    "bench layer 0 62->64 k5": (62, 64, 5, 96, 100, 154),
    "bench layer 1 64->32 k3": (64, 32, 3, 96, 100, 154),
    "bench layer 2 32->16 k3": (32, 16, 3, 96, 100, 154),
}


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(REAL))
def test_bench_geometry(lib, name, dtype):
    """the library's own kernel choice (wide = 0) at the bench step's reduction: 96 images of 100 x 154"""
    Cx, Ch, k, N, H, W = REAL[name]
    _direct(lib, Cx, Ch, k, N, H, W, dtype, seed=3)


def test_cfg3_layer(lib):
    _direct(lib, 128, 128, 3, 48, 190, 298, "bf16", seed=4)


def test_cfg4_layer0(lib):
    _direct(lib, 126, 64, 5, 96, 100, 154, "bf16", seed=5)


# --------------------------------------------------------------------------------------------------- (b) the product path
STACKS = {"bench": (62, [64, 32, 16], [5, 3, 3]), "cfg1-refpinned": (5, [64, 32, 16], [5, 3, 3])}


def _product_layer0(C0, hidden, ks, B, T, H, W, dtype, has_init, seed=0):
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    L = len(hidden)
    eng = SeqEngine([LayerCfg(C0 if l == 0 else hidden[l - 1], hidden[l], ks[l]) for l in range(L)], dtype, "cuda")
    params = O.synth_params(C0, hidden, ks, L, seed=seed)
    eng.pack_weights([params[f"layers.{l}.conv.weight"].float().cuda() for l in range(L)],
                     [params[f"layers.{l}.conv.bias"].float().cuda() for l in range(L)])
    g = torch.Generator().manual_seed(seed + 1)
    X = torch.randn(B, T, C0, H, W, generator=g).cuda()
    h0 = [0.5 * torch.randn(B, h, H, W, generator=g).cuda() for h in hidden] if has_init else None
    c0 = [torch.randn(B, h, H, W, generator=g).cuda() for h in hidden] if has_init else None
    ws = eng.acquire(B, T, H, W, True, has_init)
    try:
        eng.forward(ws, X, h0, c0)
        for l, h in enumerate(hidden):
            eng.set_state_grads(ws, l, 0.1 * torch.randn(B, h, H, W, generator=g).cuda(), 0.1 * torch.randn(B, h, H, W, generator=g).cuda())
        eng.backward(ws, False, parts=1)
        torch.cuda.synchronize()
        # integer slabs in place of what the chain stored: x, every slot of h[0] (slot 0 nonzero even from the zero state,
        # where the reduction must skip it), dG[0]
        geo = SA.geo_of(eng, ws)
        lg = geo.layers[0]
        WA.exact_budget(T * B, H, W)
        dG = WA.int_values((T * B, 4 * lg.Ch, H, W), WA.DG_MAX, g, "cuda")
        x = WA.int_values((T * B, lg.Cx, H, W), WA.SRC_MAX, g, "cuda")
        h = WA.int_values(((T + 1) * B, lg.Ch, H, W), WA.SRC_MAX, g, "cuda")
        h[:B][h[:B] == 0] = 1
        for dst, src in ((ws.xs, SA.write_xs(geo, x)), (ws.h[0], SA.write_halo(geo, h, lg.Chp)), (ws.dG[0], SA.write_dG(geo, 0, dG))):
            assert dst.numel() == src.numel()
            dst.copy_(src)
        ref_W, ref_b = WA.wgrad_ref(dG, x, h, lg.k, xfold=lg.xfold, has_init=has_init, B=B)
        outs = []
        for _ in range(2):
            eng.wg_partial.fill_(NAN)
            dW = [torch.full((4 * c.Ch, c.Cx + c.Ch, c.k, c.k), NAN, device="cuda") for c in eng.cfgs]
            db = [torch.full((4 * c.Ch,), NAN, device="cuda") for c in eng.cfgs]
            eng.backward(ws, False, parts=2, dW_out=dW, db_out=db)
            torch.cuda.synchronize()
            outs.append((dW[0], db[0]))
    finally:
        eng.release(ws)
    tag = f"layer 0 {C0}->{hidden[0]} k{ks[0]} xfold={int(lg.xfold)} B={B} T={T} {dtype} has_init={int(has_init)}"
    _diff(tag + " dW", outs[0][0], ref_W)
    _diff(tag + " db", outs[0][1], ref_b)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (tag, "not reproducible")
    print(f"  {tag}: dW, db bit-equal to the f64 sum", flush=True)
    return outs[0][0], lg


@pytest.mark.parametrize("has_init", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("stack", list(STACKS))
def test_layer0_through_the_product_path(lib, stack, dtype, has_init):
    C0, hidden, ks = STACKS[stack]
    _product_layer0(C0, hidden, ks, 8, 12, 100, 154, dtype, has_init)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("stack", list(STACKS))
def test_one_image_one_step_from_the_zero_state(lib, stack, dtype):
    """T = B = 1 from the zero state: the h part has no pixel tile at all; its (empty) splits must still write zeros"""
    C0, hidden, ks = STACKS[stack]
    dW, lg = _product_layer0(C0, hidden, ks, 1, 1, 100, 154, dtype, False)
    assert bool((dW[:, lg.Cx:] == 0).all())


# --------------------------------------------------------------------------------------------------- (c) the head
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("Ch,O,H,W", [(16, 20, 100, 154), (16, 200, 100, 154), (128, 20, 190, 298)])
def test_head_backward(lib, Ch, O, H, W, dtype):
    """dw, db through the scratch (tiled / register-tiled) path and the one-workgroup-per-output path, dh with them; the h
    slab's first two images are not the head's (n0 = 2)"""
    from nasa_niswan_amd import _lib
    from nasa_niswan_amd._lib import NINT_BF16, NINT_F32, NintGeom
    dt = NINT_BF16 if dtype == "bf16" else NINT_F32
    es = 2 if dtype == "bf16" else 4
    N, n0 = 8, 2
    geo = SA.Geo.make(1, N + n0, H, W, [(Ch, Ch, 5, False)], es)
    g = NintGeom()
    _lib.check(lib.nint_geom_make(C.byref(g), H, W, geo.P), "nint_geom_make")
    Chp = geo.layers[0].Chp
    WA.exact_budget(N, H, W)
    gen = torch.Generator().manual_seed(Ch + O)
    h = WA.int_values((N + n0, Ch, H, W), WA.SRC_MAX, gen, "cuda")
    dpred = WA.int_values((N, O, H, W), WA.DG_MAX, gen, "cuda")
    wmax = 1 if O > 128 else 2                         # |dh| <= O * wmax <= 256: exact in bf16
    assert O * wmax <= 256
    w = WA.int_values((O, Ch), wmax, gen, "cuda")
    hs = SA.write_halo(geo, h, Chp)
    ref_w, ref_b, ref_dh = WA.head_ref(h[n0:], dpred, w)
    nout = O * (Ch + 1)
    for scratch_on in (True, False):
        outs = []
        for _ in range(2):
            scratch = torch.full((256 * nout + 16,), NAN, device="cuda") if scratch_on else None
            dw = torch.full((O, Ch), NAN, device="cuda")
            db = torch.full((O,), NAN, device="cuda")
            dh = torch.full((N * H * W * Chp * es,), 255, dtype=torch.uint8, device="cuda")      # NaN in both types
            _lib.check(lib.nint_head_bwd(C.c_void_p(hs.data_ptr()), n0, N, Ch, Chp, O, C.c_void_p(w.data_ptr()),
                                         C.c_void_p(dpred.data_ptr()), C.c_void_p(dh.data_ptr()), C.c_void_p(dw.data_ptr()),
                                         C.c_void_p(db.data_ptr()), C.byref(g), dt,
                                         C.c_void_p(scratch.data_ptr()) if scratch_on else None,
                                         0 if scratch is None else scratch.numel() * 4, None), "nint_head_bwd")
            torch.cuda.synchronize()
            dh_v = dh.view(geo.et).view(N, H, W, Chp)[..., :Ch].float().permute(0, 3, 1, 2)
            outs.append((dw, db, dh_v))
        tag = f"head Ch={Ch} O={O} {H}x{W} {dtype} scratch={int(scratch_on)}"
        _diff(tag + " dw", outs[0][0], ref_w)
        _diff(tag + " db", outs[0][1], ref_b)
        _diff(tag + " dh", outs[0][2], ref_dh)
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), (tag, "not reproducible")
        print(f"  {tag}: dw, db, dh bit-equal to the f64 sums", flush=True)
