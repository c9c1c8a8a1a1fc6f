"""The bf16 backward bodies that move the gate stash and dG as 16-byte vectors (the fused BPTT step's epilogue trades halves
between lane rows 2r / 2r+1 with v_permlane16_swap: conv_igemm.hip, EPI_DGRAD_PW), at the smallest shapes where they can go
wrong: one channel block and fewer items than a block has threads, channel blocks that reach past Ch, W no multiple of 16
(masked lanes beside live ones in a swap pair's wave), merged strip tiles, and the bench stack's bodies under every launch
schedule.  The criterion is run_audit's (tests/test_gpu_stored_audit.py): max err / bound <= 1 per tensor kind against the f64
recomputation from the stored inputs, and clean padding.  The stand-alone pointwise kernel is called directly between
sentinel-filled guards, and on the read-back inputs of an engine run (byte for byte the engine's dG and dc)."""
import ctypes as C

import pytest
import torch

from oracle import guarded_alloc as GA
from oracle import stored_audit as SA
from test_gpu_stored_audit import run_audit

pytestmark = pytest.mark.gpu

RAGGED = dict(C=7, hidden=[24, 16, 8], ks=[5, 3, 3], B=3, T=3)
STACK = dict(C=7, hidden=[64, 32, 16], ks=[5, 3, 3], B=2, T=3, H=20, W=35)
WAVES = [0, 4, 5]
FUSES = [None, 0x40000404, 0x40000202, 0x40020404]
ROWS = [0, 4, 8]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


def test_one_channel_block_fewer_items_than_threads(pkg):
    """hidden [8]: Ch16 = 16, two 8-channel halves per pixel, 35 pixels"""
    run_audit(C=3, hidden=[8], ks=[3], B=1, T=3, H=5, W=7, dtype="bf16", tag="wide 3->[8] 5x7")


@pytest.mark.parametrize("H,W", [(12, 17), (9, 50)])
def test_partial_channel_blocks_and_masked_lanes(pkg, H, W):
    """channel blocks past Ch, W no multiple of 16, 12 = 8 + 4 rows (merged strip tiles) and 9 = 8 + 1"""
    run_audit(**RAGGED, H=H, W=W, dtype="bf16", tag=f"wide ragged {H}x{W}")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("fuse", FUSES)
@pytest.mark.parametrize("wave", WAVES)
def test_bench_bodies_under_every_schedule(pkg, wave, fuse, rows):
    """the stand-alone pointwise kernel, the rider, the fused step with and without its lo_* side, read-modify-write and
    overwrite out0, and both dgrad epilogues"""
    run_audit(**STACK, dtype="bf16", wave=wave, fuse=fuse, rows=rows, tag="wide 7->[64,32,16] 20x35")


def test_bench_bodies_with_initial_state(pkg):
    """d/dh_init in two pieces"""
    w, _, _ = run_audit(**STACK, dtype="bf16", wave=4, has_init=True, tag="wide 7->[64,32,16] 20x35 h0/c0")
    assert {"dh_init", "dc_init"} <= set(w)


def _engine(pkg, Cx, Ch, k, B, T, H, W):
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    eng = SeqEngine([LayerCfg(Cx, Ch, k)], "bf16", "cuda")
    ws = eng.acquire(B, T, H, W, True, False)
    return eng, ws


def test_pointwise_writes_only_the_interior(pkg):
    """nint_cell_bwd_pointwise on 3 x 5 x 7 x Ch16 = 16 between guards: the dG halo ring, the slack, dc's padding channels
    and every guard byte keep their sentinel"""
    lib = pkg.load_library()
    B, H, W = 3, 5, 7
    eng, ws = _engine(pkg, 3, 16, 3, B, 1, H, W)
    try:
        ly, g = eng.layers[0], ws.g
        Ch16, Chp, P, Hh, Wh = int(ly.Ch16), int(ly.Chp), int(g.P), int(g.Hh), int(g.Wh)
        assert Ch16 == 16 and Chp >= Ch16
        Gc = 4 * Ch16
        gen = torch.Generator().manual_seed(5)
        gt = GA.GuardedTorch("poison", row_stride=Wh * Gc * 2)
        rnd = lambda *s: torch.rand(*s, generator=gen)
        gates = gt.guard_copy(rnd(B, H, W, Gc).to(torch.bfloat16).cuda())
        c_prev = gt.guard_copy(torch.randn(B, H, W, Chp, generator=gen).cuda())
        c_new = gt.guard_copy(torch.randn(B, H, W, Chp, generator=gen).cuda())
        dh = gt.guard_copy((0.1 * torch.randn(B, H, W, Chp, generator=gen)).to(torch.bfloat16).cuda())
        dc0 = 0.1 * torch.randn(B, H, W, Chp, generator=gen)
        dc0[..., Ch16:] = 12345.0                                             # sentinel in the padding channels
        dc = gt.guard_copy(dc0.cuda())
        dG = gt.guard_copy(torch.full((B, Hh, Wh, Gc), 77.0, dtype=torch.bfloat16).cuda())
        vp = lambda t: C.c_void_p(t.data_ptr())
        assert lib.nint_cell_bwd_pointwise(C.byref(ly), C.byref(g), eng.dt, B, vp(gates), vp(c_prev), vp(c_new), vp(dh), vp(dc),
                                           vp(dG), None) == 0
        torch.cuda.synchronize()
        assert gt.verify() == 6
        out = dG.cpu().view(torch.int16)
        ring = torch.ones(B, Hh, Wh, Gc, dtype=torch.bool)
        ring[:, P:P + H, P:P + W] = False
        sentinel = torch.tensor(77.0, dtype=torch.bfloat16).view(torch.int16)
        assert bool((out[ring] == sentinel).all()), "a byte of dG outside the interior changed"
        inner = dG.cpu()[:, P:P + H, P:P + W].float()
        assert bool(torch.isfinite(inner).all()) and bool((inner != 77.0).any(dim=-1).all()), "an interior pixel of dG was not written"
        dco = dc.cpu()
        assert bool((dco[..., Ch16:] == 12345.0).all()), "dc's padding channels changed"
        assert bool((dco[..., :Ch16] != dc0[..., :Ch16]).any(dim=-1).all())
    finally:
        eng.release(ws)


def test_standalone_kernel_equals_the_engine_run(pkg):
    """wave = 0, one layer, T = 1: the step's pointwise backward is the stand-alone kernel.  nint_cell_bwd_pointwise on the
    read-back inputs gives the engine's dG slab and dc byte for byte."""
    lib = pkg.load_library()
    Cx, Ch, k, B, T, H, W = 5, 16, 3, 2, 1, 20, 35
    _, eng, st = run_audit(C=Cx, hidden=[Ch], ks=[k], B=B, T=T, H=H, W=W, dtype="bf16", wave=0, tag="wide 5->[16] 20x35 T=1")
    geo, raw = st["geo"], st["raw"]
    ws = eng.acquire(B, T, H, W, True, False)
    try:
        ly, g = eng.layers[0], ws.g
        Chp = geo.layers[0].Chp
        gates = raw["gates0"].cuda()
        c = raw["c0"].cuda()                                                  # slot 0 = c_{-1} (zero), slot 1 = c_0
        dh = SA.write_compact(geo, st["dh_T"][0], Chp, geo.et).cuda()
        dc = SA.write_compact(geo, st["dc_T"][0], Chp, torch.float32).cuda()
        dG = torch.zeros_like(raw["dG0"]).cuda()
        vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        assert lib.nint_cell_bwd_pointwise(C.byref(ly), C.byref(g), eng.dt, B, vp(gates), vp(c), vp(c, B * H * W * Chp * 4), vp(dh),
                                           vp(dc), vp(dG), None) == 0
        torch.cuda.synchronize()
        assert GA.same_bits(dG.cpu().view(torch.uint8).reshape(-1), raw["dG0"].view(torch.uint8).reshape(-1))
        assert GA.same_bits(dc.cpu().view(torch.uint8).reshape(-1), raw["dc0"].view(torch.uint8).reshape(-1))
    finally:
        eng.release(ws)
