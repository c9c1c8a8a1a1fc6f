"""The launches the bench is made of, and every conv_igemm body the library can select, through the stored-value audit of
tests/test_gpu_stored_audit.py (oracle/stored_audit.py: every element against an f64 recomputation from the slabs the launch
read, within a bound derived from the kernel's arithmetic).

oracle/launch_plan.py restates the host arithmetic that picks each launch; tests/test_launch_plan_cpu.py reads CASES below
(and the cases of tests/test_gpu_stored_audit.py) without a GPU and shows that together they run every body the ledger's sweep
can reach.  The cases:

* the bench geometry 62 -> [64, 32, 16], k [5, 3, 3], 100 x 154 as FusedTrainer.step runs it (need_dx=False,
  zero_state_grads): B = 8 under the default wave (4) and wave 0 (conv_dgrad_multi8_kernel, the 8-row dgrad bodies with the
  merged leftover strip, the 8-row forward grid), B = 2 and B = 1;
* k = 1 and k = 7 training stacks (a folded thin k = 7 input, 16 unfolded channels at k = 7, k = 1 under k = 3);
* inference workspaces (no gate stash, no BPTT): k = 9 and k = 7 stacks, the bench stack at B = 8, the stencil and dense-K
  gate kernels of a tiny top layer;
* small ragged stacks with pinned tile heights and fuse_bwd = 1 / 2 that reach the remaining n-tile rungs of the dgrad
  ladder (a pinned tile_rows disables the column split, so the rung is the n-tile count's divisibility alone).

At B = 8 the audit is also shown to see ONE bad element, once per storage type: one read-back dG[0] value inside a
merged-strip tile of the last image and one h value of layer 1 at the last time step are changed in the host copy (nothing
is written to the GPU), and the re-audit must exceed 1."""
import time

import pytest
import torch

from oracle import launch_plan as LP
from oracle import stored_audit as SA
from test_gpu_stored_audit import run_audit

pytestmark = pytest.mark.gpu

BENCH = dict(C=62, hidden=[64, 32, 16], ks=[5, 3, 3], T=3, H=100, W=154)
TRAINER = dict(need_dx=False, zero=True)          # FusedTrainer.step: backward(ws, False, zero_state_grads=all layers)
SMALL = dict(B=2, T=3, H=20, W=40)                # 20 % 8 = 4 leftover rows, 3 column tiles: every 8-row launch has the strip
WIDE4 = dict(C=128, hidden=[128, 64, 32, 16], ks=[3, 3, 3, 3])    # dgrad n-tiles 16 / 12 / 6 / 4 (f32: 3), fused 16 / 12 / 6 / 3
TALL3 = dict(C=64, hidden=[128, 48, 16], ks=[3, 3, 3])
TINY = dict(C=7, hidden=[16, 8, 8], ks=[5, 3, 3], B=3, T=3, H=37, W=50)    # layers 1-2 stencil-shaped, layer 2 dense-K in f32 too

CASES = {}
for _d in ("bf16", "f32"):
    CASES.update({
        f"bench B=8 trainer {_d}": dict(BENCH, B=8, dtype=_d, **TRAINER),
        # (the f64 audit of B = 8 costs ~10 s per time step on the CPU: the wave-0 and inference forms audit the gate launches
        # of the later steps only, whose bodies include the h half of K)
        f"bench B=8 trainer wave 0 {_d}": dict(BENCH, B=8, dtype=_d, wave=0, fwd_ts=[1, 2], **TRAINER),
        f"bench B=2 trainer {_d}": dict(BENCH, B=2, dtype=_d, **TRAINER),
        f"bench B=1 trainer {_d}": dict(BENCH, B=1, dtype=_d, **TRAINER),
        f"k7 folded 3->[16,8] {_d}": dict(C=3, hidden=[16, 8], ks=[7, 3], dtype=_d, **SMALL),
        f"k7 unfolded 16->[16,16] {_d}": dict(C=16, hidden=[16, 16], ks=[3, 7], dtype=_d, **SMALL),
        f"k1 8->[32,16] {_d}": dict(C=8, hidden=[32, 16], ks=[1, 3], dtype=_d, **SMALL),
        f"inference k9 5->[16,8] {_d}": dict(C=5, hidden=[16, 8], ks=[9, 3], dtype=_d, train=False, **SMALL),
        f"inference k7 16->[32,16] {_d}": dict(C=16, hidden=[32, 16], ks=[7, 7], dtype=_d, train=False, **SMALL),
        f"inference bench B=8 {_d}": dict(BENCH, B=8, dtype=_d, train=False, fwd_ts=[2]),
        f"inference stencil {_d}": dict(TINY, dtype=_d, rows=1, train=False),
        f"inference dense-K {_d}": dict(TINY, dtype=_d, rows=2, train=False),
        f"tiny top wave 5 {_d}": dict(TINY, dtype=_d, wave=5),
        f"wide4 rows8 fused {_d}": dict(WIDE4, dtype=_d, rows=8, fuse=2, **SMALL),
        f"wide4 rows8 classic {_d}": dict(WIDE4, dtype=_d, rows=8, fuse=1, **SMALL),
        f"wide4 rows4 fused {_d}": dict(WIDE4, dtype=_d, rows=4, fuse=2, **SMALL),
        f"wide4 rows4 classic {_d}": dict(WIDE4, dtype=_d, rows=4, fuse=1, **SMALL),
        f"tall3 rows8 fused trainer {_d}": dict(TALL3, dtype=_d, rows=8, fuse=2, need_dx=False, **SMALL),
        f"tall3 fused trainer {_d}": dict(TALL3, dtype=_d, fuse=2, need_dx=False, **SMALL),
    })
CASES.update({
    "wide4 fused bf16": dict(WIDE4, dtype="bf16", fuse=2, **SMALL),
    "wide4 fused trainer bf16": dict(WIDE4, dtype="bf16", fuse=2, need_dx=False, **SMALL),
    "16->[32,128,16] rows8 fused f32": dict(C=16, hidden=[32, 128, 16], ks=[3, 3, 3], dtype="f32", rows=8, fuse=2, **SMALL),
    "32->[96,64,32] rows8 fused bf16": dict(C=32, hidden=[96, 64, 32], ks=[3, 3, 3], dtype="bf16", rows=8, fuse=2, **SMALL),
    "48->[64,16] rows8 fused trainer bf16": dict(C=48, hidden=[64, 16], ks=[3, 3], dtype="bf16", rows=8, fuse=2, need_dx=False,
                                                 **SMALL),
})
SENSITIVITY = {"bench B=8 trainer bf16", "bench B=8 trainer f32"}


def ledger_cases():
    """run_audit's keyword arguments for every case of this file"""
    return list(CASES.values())


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    t0 = time.time()
    yield p
    print(f"\n  test_gpu_launch_audit wall time {time.time() - t0:.1f} s")


def _perturb(v: torch.Tensor, n: int, y: int, x: int) -> torch.Tensor:
    """a copy of v (N, C, H, W) with the largest-magnitude channel of pixel (n, y, x) moved by 5 %"""
    v = v.clone()
    c = int(v[n, :, y, x].abs().argmax())
    v[n, c, y, x] = v[n, c, y, x] * 1.05
    assert v[n, c, y, x].abs() > 0
    return v


def _sensitivity(st, kw):
    geo, B, T = st["geo"], kw["B"], kw["T"]
    y, x = geo.H - 2, geo.W - 4            # (100 x 154 on 8-row tiles: rows 96..99 are the merged strip)
    assert geo.H % 8 and geo.H % 8 <= 4
    hp = dict(st, dG=list(st["dG"]))
    hp["dG"][0] = _perturb(st["dG"][0], (T - 1) * B + B - 1, y, x)
    w = SA.audit(geo, st["Ws"], st["bs"], hp, st["dh_T"], st["dc_T"], False, fwd_ts=[], t_min=T - 1)
    print(f"  one dG[0] element of the last image's merged strip 5 % off: dG err/bound {w['dG']:.1f}")
    assert w["dG"] > 1.0, w
    hp = dict(st, h=list(st["h"]))
    hp["h"][1] = _perturb(st["h"][1], T * B + B - 1, y, x)
    w = SA.audit(geo, st["Ws"], st["bs"], hp, st["dh_T"], st["dc_T"], False, fwd_ts=[T - 1], t_min=T)
    print(f"  one h element of layer 1 at t = T-1 5 % off: h err/bound {w['h']:.1f}")
    assert w["h"] > 1.0, w


@pytest.mark.parametrize("name", list(CASES))
def test_launch_audit(pkg, name):
    kw = CASES[name]
    launches = LP.case_launches(**kw)
    print(f"\n  {name}: " + "  ".join(f"{LP.fmt_body(b)}" + ("+strip" if any(s for _, s in v) else "") + "@"
                                      + "/".join(sorted({k for k, _ in v})) for b, v in sorted(LP.bodies(launches).items())))
    worst, eng, st = run_audit(**kw, tag=name)
    if kw.get("train", True):
        # the ledger's merge_d assumes the split-K scratch holds the bottom layer's d/dh (nint_seq_bwd)
        ly0 = st["geo"].layers[0]
        assert eng.wg_partial.numel() * 4 >= kw["B"] * kw["H"] * kw["W"] * ly0.Chp * st["geo"].es
    if kw.get("wave") is None:
        assert st["wave"] == LP.default_wave(kw["B"], kw["H"], kw["W"], len(kw["hidden"]), eng.n_cu)
    if name in SENSITIVITY:
        _sensitivity(st, kw)
