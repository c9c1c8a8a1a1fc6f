"""Every gate and BPTT launch of SeqEngine.forward + backward checked elementwise against an f64 recomputation from the
values it read out of the workspace (oracle/stored_audit.py: reference and error bound per element), and the padding of
every slab checked after the pass.  A local mistake -- one tile, one dropped tap of one channel chunk, one stale pixel, a
stray write into the halo -- shows here as err / bound > 1 where the end-to-end rel-L2 gates of the other files cannot see
it.  Each case prints its worst err / bound per tensor kind.

Every layer's weight and bias gradient (the dW / db engine.backward returns) is checked against oracle/wgrad_audit.py's
gamma_{n+1} sum |dG||cat| bound, built from the stored dG[l], the stored x source (xs, or h[l-1] slots 1..T) and h[l] slots
0..T-1 (slot 0 skipped from the zero state): the wiring of layers >= 1 (a source one time step off, the wrong layer's slab,
a wrong skip, another layer's fold-table entry) shows here; the summation itself is checked bit for bit on integer data in
tests/test_gpu_exact_reductions.py."""
import time

import pytest
import torch

from oracle import convlstm_oracle as O
from oracle import stored_audit as SA
from oracle import wgrad_audit as WA

pytestmark = pytest.mark.gpu

KINDS = ("gates", "c", "h", "dG", "dx", "dh_init", "dc_init", "zacc", "dW", "db")


class _Done(Exception):
    """an inference run has no backward: read back after the forward"""


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    t0 = time.time()        # (this file's tests only: the clock starts at its first test, not at collection)
    yield p
    print(f"\n  test_gpu_stored_audit wall time {time.time() - t0:.1f} s")


def run_audit(C, hidden, ks, B, T, H, W, dtype, wave=None, rows=0, fuse=None, has_init=False, zero=False, seed=0,
              fwd_ts=None, t_min=0, params=None, X=None, tag="", need_dx=True, train=True):
    """forward + backward through a Workspace with injected state gradients at T-1 (or zero_state_grads), then the audit.
    need_dx: engine.backward's argument (the trainer passes False).  train=False: an inference workspace (no stash, no BPTT;
    the audit checks h, c and the padding).  Returns (worst err / bound per kind, engine, read-back slabs)."""
    from nasa_niswan_amd import engine
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    L = len(hidden)
    engine.FORCE_TILE_ROWS = rows
    try:
        eng = SeqEngine([LayerCfg(C if l == 0 else hidden[l - 1], hidden[l], ks[l]) for l in range(L)], dtype, "cuda")
    finally:
        engine.FORCE_TILE_ROWS = 0
    params = params or O.synth_params(C, hidden, ks, L, seed=seed)
    Ws = [params[f"layers.{l}.conv.weight"].float() for l in range(L)]
    bs = [params[f"layers.{l}.conv.bias"].float() for l in range(L)]
    eng.pack_weights([w.cuda() for w in Ws], [b.cuda() for b in bs])
    g = torch.Generator().manual_seed(seed + 17)
    X = torch.randn(B, T, C, H, W, generator=g) if X is None else X
    h0 = [0.5 * torch.randn(B, h, H, W, generator=g) for h in hidden] if has_init else None
    c0 = [torch.randn(B, h, H, W, generator=g) for h in hidden] if has_init else None
    ws = eng.acquire(B, T, H, W, train, has_init)
    dWs = dbs = None
    engine.FORCE_WAVE = wave
    try:
        if fuse is not None:
            ws.seq.fuse_bwd = fuse
        eng.forward(ws, X.cuda(), None if h0 is None else [v.cuda() for v in h0], None if c0 is None else [v.cuda() for v in c0])
        geo = SA.geo_of(eng, ws)
        wave_ran = int(ws.seq.wave)
        dh_T = dc_T = None
        for l, h in enumerate(hidden if train else ()):
            eng.set_state_grads(ws, l, (0.1 * torch.randn(B, h, H, W, generator=g)).cuda(), (0.1 * torch.randn(B, h, H, W, generator=g)).cuda())
        torch.cuda.synchronize()
        if not train:
            st = SA.read_workspace(eng, ws)
            raise _Done
        # the stored state gradients the backward starts from (copies of the slabs as set_state_grads left them)
        dh_T = [SA.read_compact(geo, ws.dh[l], B, h, geo.layers[l].Chp, geo.et) for l, h in enumerate(hidden)]
        dc_T = [SA.read_compact(geo, ws.dc[l], B, h, geo.layers[l].Chp, torch.float32) for l, h in enumerate(hidden)]
        if zero:              # zero_state_grads: dc of every layer and dh of every layer but the top one start from zero
            dh_T = [None] * (L - 1) + [dh_T[-1]]
            dc_T = [None] * L
        dWs, dbs, dx = eng.backward(ws, need_dx=need_dx, zero_state_grads=range(L) if zero else ())
        torch.cuda.synchronize()
        st = SA.read_workspace(eng, ws, dx)
    except _Done:
        pass
    finally:
        engine.FORCE_WAVE = None
        ws.seq.fuse_bwd = engine.FUSE_BWD
        eng.release(ws)
    bad = SA.check_padding(geo, st["raw"])
    assert bad == [], (tag, bad)
    worst = SA.audit(geo, Ws, bs, st, dh_T, dc_T, has_init, fwd_ts=fwd_ts, t_min=t_min)
    for l in range(L if train else 0):      # the weight / bias gradient of every layer from the slabs it reduced, reference in f64 on the GPU
        x_src = st["x"] if l == 0 else st["h"][l - 1][B:]
        rW, rb = WA.wgrad_bound(st["dG"][l].cuda(), x_src.cuda(), st["h"][l].cuda(), ks[l], geo.es, has_init=has_init,
                                B=B, n_cu=eng.n_cu)
        worst["dW"] = max(worst.get("dW", 0.0), WA.bound_ratio(dWs[l], rW))
        worst["db"] = max(worst.get("db", 0.0), WA.bound_ratio(dbs[l], rb))
    print(f"  {tag} {dtype} wave={wave_ran} rows={rows} fuse={fuse if fuse is None else hex(fuse)}"
          f"{'' if train else ' inference'}{'' if need_dx or not train else ' need_dx=False'}: max err/bound  "
          + "  ".join(f"{k} {worst[k]:.3f}" if k not in ("dW", "db") else f"{k} {worst[k]:.1e}" for k in KINDS if k in worst), flush=True)
    assert max(worst.values()) <= 1.0, (tag, dtype, wave, rows, fuse, worst)
    if train:
        assert {"gates", "c", "h", "dG", "dW", "db"} | ({"dx"} if need_dx else set()) <= set(worst)
        assert need_dx or "dx" not in worst
    else:
        assert {"c", "h"} <= set(worst) and "gates" not in worst and "dG" not in worst
    st["dW"], st["db"], st["dh_T"], st["dc_T"], st["Ws"], st["bs"] = dWs, dbs, dh_T, dc_T, Ws, bs
    st["wave"] = wave_ran
    return worst, eng, st


# The cases of this file as module-level tables: tests/test_launch_plan_cpu.py reads them (without a GPU) to show which kernel
# bodies the audit reaches (oracle/launch_plan.py).
BENCH = dict(C=62, hidden=[64, 32, 16], ks=[5, 3, 3], B=2, T=3, H=100, W=154)
BENCH_WAVES = [("bf16", 0), ("bf16", 4), ("bf16", 5), ("bf16", None), ("f32", 4)]
RAGGED = dict(C=7, hidden=[24, 16, 8], ks=[5, 3, 3], B=3, T=3, H=37, W=50)
RAGGED_ROWS = [0, 4, 8, 1, 2]
FUSE_MASKS = [0x40000404, 0x40000202, 0x40020404]
INIT2 = dict(C=9, hidden=[32, 16], ks=[5, 3], B=2, T=3, H=29, W=45, has_init=True)
INIT_WAVES = [0, 4, 5]
CFG3 = dict(C=62, hidden=[128, 128, 128], ks=[3, 3, 3], B=1, T=2, H=30, W=70)
CANONICAL = dict(C=5, hidden=[64, 32, 16], ks=[5, 3, 3], B=1, T=48, H=100, W=154, fwd_ts=[0, 1, 24, 46, 47], t_min=45)
DTYPES = ["bf16", "f32"]


def ledger_cases():
    """run_audit's keyword arguments for every case of this file"""
    out = [dict(BENCH, dtype=d, wave=w) for d, w in BENCH_WAVES]
    out += [dict(RAGGED, dtype=d, rows=r) for d in DTYPES for r in RAGGED_ROWS]
    out += [dict(RAGGED, dtype=d, fuse=f) for d in DTYPES for f in FUSE_MASKS]
    out += [dict(RAGGED, dtype=d, zero=True) for d in DTYPES]
    out += [dict(INIT2, dtype=d, wave=w) for d in DTYPES for w in INIT_WAVES]
    out += [dict(CFG3, dtype=d) for d in DTYPES]
    out += [dict(CANONICAL, dtype=d) for d in DTYPES]
    return out


@pytest.mark.parametrize("dtype,wave", BENCH_WAVES)
def test_bench_geometry(pkg, dtype, wave):
    _, eng, st = run_audit(**BENCH, dtype=dtype, wave=wave, tag="bench 62->[64,32,16] 100x154 B=2 T=3")
    # the dW bound's margin against a source one time step off: layer 1's x source read from h[0] slots 0..T-1 instead of 1..T
    B = 2
    rW, _ = WA.wgrad_bound(st["dG"][1].cuda(), st["h"][0][:-B].cuda(), st["h"][1].cuda(), 3, st["geo"].es, has_init=False, B=B,
                           n_cu=eng.n_cu)
    r = WA.bound_ratio(st["dW"][1], rW)
    print(f"  layer 1 dW against the reference of an x source one step early: err/bound {r:.1f}")
    assert r > 1.0, r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", RAGGED_ROWS)
def test_ragged_stack_every_tile_height(pkg, dtype, rows):
    """1 / 2: the stencil / dense-K gate kernels of the tiny top layer (8 hidden channels, k = 3; other layers take 0)"""
    run_audit(**RAGGED, dtype=dtype, rows=rows, tag="ragged 7->[24,16,8] 37x50 B=3 T=3")


@pytest.mark.parametrize("fuse", FUSE_MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_schedules_with_lower_pointwise(pkg, fuse, dtype):
    """explicit fuse_bwd masks (tests/test_gpu_fused_bwd.py): a fused layer running the pointwise backward of the classic
    layer below on its x columns (lo_*), and a classic layer doing the same for the one below it"""
    run_audit(**RAGGED, dtype=dtype, fuse=fuse, tag="ragged fused")


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_state_grads(pkg, dtype):
    run_audit(**RAGGED, dtype=dtype, zero=True, tag="ragged zero_state_grads")


@pytest.mark.parametrize("wave", INIT_WAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_given_initial_state(pkg, dtype, wave):
    """has_init_state: d/dh_init and d/dc_init of both layers (the bottom one's d/dh in two pieces under wave 4 / 5)"""
    w, _, _ = run_audit(**INIT2, dtype=dtype, wave=wave, tag="2 layers with h0/c0")
    assert {"dh_init", "dc_init"} <= set(w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cfg3_like(pkg, dtype):
    run_audit(**CFG3, dtype=dtype, tag="cfg3-like 62->3x128 k3 30x70 B=1 T=2")


@pytest.fixture(scope="module")
def canonical():
    """The reference notebook's model ConvLSTM(5, [64, 32, 16], [5, 3, 3], 3) (test.ipynb:4585, model.py:282-295) on
    (1, 48, 5, 100, 154), PyTorch default init; the f32 CPU oracle's top-layer h at t = 47."""
    params = O.init_params(5, [64, 32, 16], [5, 3, 3], 3, seed=0)
    X = torch.randn(1, 48, 5, 100, 154, generator=torch.Generator().manual_seed(48))
    _, hs, _ = O.convlstm_forward(X, params, return_states=True)
    return params, X, hs[-1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_canonical_T48(pkg, canonical, dtype):
    """forward launches at t in {0, 1, 24, 46, 47}, backward launches of the last three steps, and the end-to-end top-layer
    h at t = 47 against the oracle (the drift over 48 steps, under the standing 2e-2)"""
    params, X, h_ref = canonical
    _, eng, st = run_audit(**CANONICAL, dtype=dtype, params=params, X=X, tag="canonical T=48 (1,48,5,100,154)")
    h47 = st["h"][2][48:49].double()
    e = float((h47 - h_ref.double()).norm() / h_ref.double().norm())
    print(f"  canonical T=48 {dtype}: top-layer h at t=47 rel-L2 against the oracle {e:.3e}")
    assert e <= (2e-2 if dtype == "bf16" else 1e-3), e
