"""The memory contract of the library (DESIGN.md "Memory contract"), enforced with oracle/guarded_alloc.py:

  * no kernel stores outside the extent of a buffer it was given: every device buffer the package allocates, and every tensor
    the test passes in, is the middle of an arena whose guards (at least 64 KiB and four of the widest slab rows on either
    side) are compared byte for byte afterwards;
  * no result depends on a byte outside an extent or on the prior contents of an ``empty`` buffer: the same work runs three
    times, each with a freshly built model / engine / trainer -- P on plain torch, Z with guards and ``empty`` payloads of
    0x00, N with 0xFF (NaN in bf16 / f32 / f64) -- and every output of Z equals P and of N equals Z bit for bit (integer
    views).  The kernels use no atomics, so run-to-run bit equality is the project's standing rule; P == Z is asserted first,
    so that a miss is attributable: P != Z says the result depends on addresses or on stale memory;
  * the size queries of the C ABI are sufficient: the entries that take a caller's scratch run on buffers carved at exactly
    the queried size, in poison mode, and give the bits of the same call on generous plain buffers.

Shapes: 13 x 37 (ragged in 8-row, 16- and 32-column tiles), 8 x 32 (exact tiles: the last tile ends on the slab's last
byte), 9 x 33 (one over), 3 x 5 (smaller than any tile); B = 2, T = 3 with one scenario at B = 1, T = 1 and one at B = 3.
A guard hit is absorbed by the arena: it is reported, not a GPU fault."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest
import torch

from oracle import guarded_alloc as GA

pytestmark = pytest.mark.gpu

GRIDS = [(13, 37), (8, 32), (9, 33), (3, 5)]
S_FOLD = (5, [20, 12], [5, 3])
S_WIDE = (40, [32, 16, 16], [3, 3, 3])
S_FAM = (64, [32], [3])
S_TINY3 = (4, [8, 8, 4], [3, 3, 3])
S_TINY1 = (3, [5], [3])
S_K7 = (16, [32, 16], [7, 7])
S_K1 = (6, [16], [1])
S_ONE = (1, [16], [3])
S_INF = (5, [16, 8], [9, 3])
BOTH = ("f32", "bf16")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def row_stride(stack, grid):
    """an upper bound of Wh * Cp * es over every slab of the scenario: the halo row (W + 2 P, rounded up generously) times the
    widest channel count (the folded input k * C rounded up to a K chunk, the padded hidden width, the 4 * Ch16 gate columns)
    in f32"""
    C_, hidden, ks = stack
    Wh = grid[1] + 2 * max(k // 2 for k in ks) + 32
    chans = max(ks[0] * C_ + 32, C_ + 32, 4 * (max(hidden) + 16))
    return Wh * chans * 4


@contextlib.contextmanager
def knobs(**kw):
    from nasa_niswan_amd import engine
    old = {k: getattr(engine, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(engine, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(engine, k, v)


def three_runs(name, scenario, stride, self_check=None):
    """scenario(gt) -> {output name: tensor}; gt None = plain torch.  Asserts P == Z, then Z == N, bitwise, both verify()s, and
    that N holds no NaN.  Returns the number of guarded allocations of the N run."""
    t0 = time.time()
    outs, count = {}, 0
    for tag, mode in (("P", None), ("Z", "zero"), ("N", "poison")):
        if mode is None:
            res = scenario(None)
            torch.cuda.synchronize()
        else:
            with GA.patched(mode=mode, row_stride=stride) as gt:
                res = scenario(gt)
                torch.cuda.synchronize()
                count = gt.verify()
                if self_check is not None and mode == "poison":
                    self_check(gt)
                gt.release()
        outs[tag] = {k: (v.dtype, tuple(v.shape), GA.bits(v), v.detach().cpu()) for k, v in res.items() if v is not None}
    P, Z, N = outs["P"], outs["Z"], outs["N"]
    assert set(P) == set(Z) == set(N), (name, sorted(P), sorted(Z), sorted(N))
    for a, b, what in ((P, Z, "plain torch vs guarded zero-filled: the result depends on addresses or stale memory"),
                       (Z, N, "zero-filled vs poisoned: the result depends on a byte the library never wrote")):
        for k in a:
            assert a[k][:2] == b[k][:2], (name, k, a[k][:2], b[k][:2])
            if not torch.equal(a[k][2], b[k][2]):
                va, vb = a[k][3], b[k][3]
                nan = int(torch.isnan(vb).sum()) if vb.is_floating_point() else 0
                ndiff = int((a[k][2] != b[k][2]).sum())
                raise AssertionError(f"{name}: output '{k}' differs ({what}): {ndiff} bytes differ, {nan} NaN in the second run")
    for k, v in N.items():
        if v[3].is_floating_point():
            assert not bool(torch.isnan(v[3]).any()), (name, k, "NaN in the poisoned run")
    print(f"  {name}: {count} guarded allocations, {len(P)} outputs, {time.time() - t0:.2f} s")
    return count


# ------------------------------------------------------------------------------ scenarios
def build_net(pkg, gt, stack, dtype, out=2, rs=False, seed=3):
    from oracle import convlstm_oracle as O
    C_, hidden, ks = stack
    net = pkg.ConvLSTM(C_, hidden, ks, len(hidden), out_channels=out, return_sequence=rs, compute_dtype=dtype).cuda()
    net.load_state_dict(O.synth_params(C_, hidden, ks, len(hidden), out_channels=out, seed=seed))
    if gt is not None:
        gt.guard_module(net)
        _fill_unused_weight_tail(net._engine(torch.device("cuda", torch.cuda.current_device())), gt.fill)
    return net


def _fill_unused_weight_tail(eng, fill):
    """nint_packed_weight_bytes sizes both images by the dgrad image; a FOLDED forward image has fewer K-steps, so the bytes
    behind its sf * (4 Ch16 / 16) * 64 * EPL elements are reserved and never written.  They take the run's fill byte here
    (the engine zero-fills them): a kernel that read them would make the poisoned run differ.  (Layers with the stencil /
    dense-K images behind the MFMA images, Ch <= 8, are left alone: those images start inside that range.)"""
    cfg, ly = eng.cfgs[0], eng.layers[0]
    if not cfg.xfold or cfg.Ch <= 8:
        return
    sf = ly.Cxp // eng.kc * cfg.k + ly.Chp // eng.kc * cfg.k * cfg.k
    nf = sf * (4 * ly.Ch16 // 16) * 64 * (eng.kc // 4) * eng.es
    assert 0 < nf < eng.Wf[0].numel()
    eng.Wf[0][nf:] = fill


def module_scenario(pkg, stack, grid, dtype, B=2, T=3, form="dx", out=2):
    C_, hidden, ks = stack
    L, (H, W) = len(hidden), grid

    def run(gt):
        G = (lambda t: t) if gt is None else gt.guard_copy
        dev = lambda *shape, seed, scale=1.0: G(rnd(*shape, seed=seed, scale=scale).cuda())
        net = build_net(pkg, gt, stack, dtype, out, rs=form == "seq")
        X = dev(B, T, C_, H, W, seed=1)
        R = dev(B, out, H, W, seed=2)
        res = {}
        if form == "nograd":
            with torch.no_grad():
                res["pred"] = net(X)
            return res
        if form == "freeze0":
            net.layers[0].requires_grad_(False)
        else:
            X.requires_grad_(True)
        st = None
        if form == "state":
            st = [(dev(B, ch, H, W, seed=10 + l, scale=0.5).requires_grad_(True), dev(B, ch, H, W, seed=20 + l).requires_grad_(True))
                  for l, ch in enumerate(hidden)]
            pred, states = net(X, st, return_state=True)
            loss = (pred * R).sum()
            for l, (h, c) in enumerate(states):
                loss = loss + (h * dev(B, hidden[l], H, W, seed=30 + l)).sum() + (c * dev(B, hidden[l], H, W, seed=40 + l)).sum()
                res[f"h_T.{l}"], res[f"c_T.{l}"] = h.detach(), c.detach()
        elif form == "seq":
            pred, seq = net(X)
            loss = (pred * R).sum() + (seq * dev(B, T * out, H, W, seed=5)).sum()
            res["seq"] = seq.detach()
        else:
            pred = net(X)
            loss = (pred * R).sum()
        loss.backward()
        res["pred"], res["loss"] = pred.detach(), loss.detach()
        if X.grad is not None:
            res["dX"] = X.grad
        for k, p in net.named_parameters():
            if p.requires_grad:
                res["grad." + k] = p.grad
        if st is not None:
            for l, (h, c) in enumerate(st):
                res[f"dh0.{l}"], res[f"dc0.{l}"] = h.grad, c.grad
            # the carried state: a detached device state out of one call, into the next, and back as tensors
            with torch.no_grad():
                _, carried = net(X, None, return_state="device")
                pred2, carried2 = net(X, carried, return_state="device")
            res["pred.carried"] = pred2
            for l, (h, c) in enumerate(carried2.tensors()):
                res[f"carried.h.{l}"], res[f"carried.c.{l}"] = h, c
        return res
    return run


MODULE_CASES = []
for _g in GRIDS:
    for _d in BOTH:
        MODULE_CASES.append((f"fold-{_g[0]}x{_g[1]}-{_d}", S_FOLD, _g, _d, {}, {}))
        MODULE_CASES.append((f"wide-{_g[0]}x{_g[1]}-{_d}", S_WIDE, _g, _d, {}, {}))
for _d in BOTH:
    for _k in ([dict(XFOLD=False)] + [dict(FORCE_WAVE=w) for w in (0, 1, 2, 4, 5)] + [dict(FUSE_BWD=f) for f in (1, 2)]
               + [dict(FORCE_TILE_ROWS=r) for r in (4, 8)]):
        MODULE_CASES.append((f"fold-13x37-{_d}-" + "-".join(f"{k}{v}" for k, v in _k.items()), S_FOLD, (13, 37), _d, _k, {}))
    for _k in [dict(FORCE_WAVE=w) for w in (0, 4, 5)] + [dict(FUSE_BWD=2)]:
        MODULE_CASES.append((f"wide-13x37-{_d}-" + "-".join(f"{k}{v}" for k, v in _k.items()), S_WIDE, (13, 37), _d, _k, {}))
    for _s, _n in ((S_TINY3, "tiny3"), (S_TINY1, "tiny1")):
        for _r in (0, 1, 2, 8):
            MODULE_CASES.append((f"{_n}-13x37-{_d}-rows{_r}", _s, (13, 37), _d, dict(FORCE_TILE_ROWS=_r), {}))
        for _g in GRIDS[1:]:
            MODULE_CASES.append((f"{_n}-{_g[0]}x{_g[1]}-{_d}", _s, _g, _d, {}, {}))
    for _g in GRIDS:
        for _s, _n in ((S_K7, "k7"), (S_K1, "k1"), (S_ONE, "onechannel")):
            MODULE_CASES.append((f"{_n}-{_g[0]}x{_g[1]}-{_d}", _s, _g, _d, {}, {}))
        MODULE_CASES.append((f"inference-k9-{_g[0]}x{_g[1]}-{_d}", S_INF, _g, _d, {}, dict(form="nograd")))
    # the call forms, on the first stack and (dx, state) on a tiny one
    for _f in ("seq", "state", "freeze0"):
        MODULE_CASES.append((f"fold-13x37-{_d}-{_f}", S_FOLD, (13, 37), _d, {}, dict(form=_f)))
    MODULE_CASES.append((f"tiny3-9x33-{_d}-state", S_TINY3, (9, 33), _d, {}, dict(form="state")))
    MODULE_CASES.append((f"fold-13x37-{_d}-B1T1", S_FOLD, (13, 37), _d, {}, dict(B=1, T=1)))
    MODULE_CASES.append((f"fold-13x37-{_d}-B3", S_FOLD, (13, 37), _d, {}, dict(B=3)))
    MODULE_CASES.append((f"wide-9x33-{_d}-B3-seq", S_WIDE, (9, 33), _d, {}, dict(B=3, form="seq")))
for _w in (1, 2):
    for _g in GRIDS:
        MODULE_CASES.append((f"families-{_g[0]}x{_g[1]}-bf16-wide{_w}", S_FAM, _g, "bf16", dict(FORCE_WIDE=_w), {}))


@pytest.mark.parametrize("name,stack,grid,dtype,kn,kw", MODULE_CASES, ids=[c[0] for c in MODULE_CASES])
def test_module_paths_write_inside_their_buffers_and_read_nothing_stale(pkg, name, stack, grid, dtype, kn, kw):
    with knobs(**kn):
        three_runs(name, module_scenario(pkg, stack, grid, dtype, **kw), row_stride(stack, grid))


# ------------------------------------------------------------------------------ the trainer
def trainer_scenario(pkg, stack, grid, dtype, B=2, T=4, out=2, halo=(2, 3), chunks=1, reset=None, **opts):
    from nasa_niswan_amd.trainer import FusedTrainer
    C_, hidden, ks = stack
    H, W = grid
    Hc, Wc = H - 2 * halo[0], W - 2 * halo[1]
    sq = opts.get("sequence_loss", False)

    def run(gt):
        G = (lambda t: t) if gt is None else gt.guard_copy
        net = build_net(pkg, gt, stack, dtype, out)
        kw = dict(opts)
        if kw.pop("weighted", False):
            kw["loss_weights"] = np.abs(rnd(Hc, Wc, seed=77).numpy()) + 0.1
        if kw.pop("spec", False):
            from nasa_niswan_amd.loss import LossSpec
            kw["loss"] = LossSpec(0.5, 2.0, 1.5, delta=0.7, output_weights=[1.0, 2.0][:out] if out <= 2 else None,
                                  step_weights=[0.0, 0.5, 1.0, 1.0][:T] if sq else None)
        tr = FusedTrainer(net, lr=1e-3, betas=(0.5, 0.999), halo=halo, **kw)
        if gt is not None and tr._weights is not None:        # the weight map, made by the trainer with .to(): guarded too
            tr._weights.on(tr.device, Hc, Wc)
            tr._weights.map = gt.guard_copy(tr._weights.map)
        res = {}
        steps = 2 * kw.get("accumulate_steps", 1) if chunks == 1 else chunks
        for j in range(steps):
            X = G(rnd(B, T, C_, H, W, seed=100 + j).cuda())
            y = G(rnd(*((B, T, out, Hc, Wc) if sq else (B, out, Hc, Wc)), seed=200 + j).cuda())
            if tr.stateful:
                loss = tr.step(X, y, reset=reset if j == chunks - 1 else None)
            else:
                loss = tr.step(X, y)      # (the second step reuses the pooled workspace, _dpred and the moments)
            res[f"loss.{j}"] = loss.detach().clone()
            res[f"dpred.{j}"] = tr._dpred.detach().clone()
        res["bucket"], res["bucket.grad"] = tr.flat.data, tr.flat.grad
        res["exp_avg"], res["exp_avg_sq"] = tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq
        res["stats"] = tr.stats
        if tr.optimizer.guarded:
            res["opt_state"] = tr.optimizer._opt_state
        if tr.state is not None:
            for l, (h, c) in enumerate(tr.state.tensors()):
                res[f"state.h.{l}"], res[f"state.c.{l}"] = h, c
        return res
    return run


TRAINER_VARIANTS = {
    "plain": {},
    "weighted-huber-seq": dict(weighted=True, spec=True, sequence_loss=True),
    "clip": dict(max_grad_norm=0.05),
    "freeze1-decay": dict(freeze_layers=1, weight_decay=1e-2),
    "segments2-accumulate2": dict(bptt_segments=2, accumulate_steps=2),
    "stateful": dict(stateful=True, chunks=2, reset=[False, True]),
    "stateful-clip-skip": dict(stateful=True, chunks=2, reset=[True, False], max_grad_norm=0.05, skip_nonfinite=True),
}
TRAINER_CASES = [(f"fold-13x37-{d}-{v}", S_FOLD, (13, 37), d, v) for d in BOTH for v in TRAINER_VARIANTS]
TRAINER_CASES += [(f"tiny3-9x33-{d}-plain", S_TINY3, (9, 33), d, "plain") for d in BOTH]
TRAINER_CASES += [(f"wide-8x32-{d}-{v}", S_WIDE, (8, 32), d, v) for d in BOTH for v in ("plain", "segments2-accumulate2")]


@pytest.mark.parametrize("name,stack,grid,dtype,variant", TRAINER_CASES, ids=[c[0] for c in TRAINER_CASES])
def test_trainer_steps_write_inside_their_buffers_and_read_nothing_stale(pkg, name, stack, grid, dtype, variant):
    three_runs(name, trainer_scenario(pkg, stack, grid, dtype, **TRAINER_VARIANTS[variant]), row_stride(stack, grid))


# ------------------------------------------------------------------------------ evaluation, streaming, the dataset's slab path
def _dataset(gt, **kw):
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    ds = SyntheticE33OMA_CRNN(device="cuda", **kw)
    if gt is not None:          # the resident record is uploaded with .to(): its arrays into arenas as well
        dv = ds._device_arrays()
        for k in list(dv):
            dv[k] = gt.guard_copy(dv[k])
    return ds


def skill_scenario(pkg, dtype):
    from nasa_niswan_amd.inference import evaluate_skill

    def run(gt):
        ds = _dataset(gt, period="test", padding=(13, 37), sequence_length=3, n_steps=40, grid=(9, 31), levels=2, in_channels=8)
        net = build_net(pkg, gt, (8, [20, 12], [5, 3]), dtype, out=2)
        acc, preds = evaluate_skill(net, ds, batch_size=3, halo=(2, 3), groups=lambda i: i % 3 - (i % 7 == 0),
                                    lat=np.linspace(-40, 40, 9), return_predictions=True)
        pix, counts, sample = acc.sums()
        return {"pix": torch.from_numpy(pix), "sample": torch.from_numpy(sample), "counts": torch.from_numpy(counts), "preds": preds}
    return run


def stream_scenario(pkg, dtype):
    from nasa_niswan_amd.inference import SkillAccumulator, predict_stream

    def run(gt):
        ds = _dataset(gt, period="test", padding=(13, 37), in_channels=5, sequence_length=3, n_steps=70, grid=(9, 31))
        net = build_net(pkg, gt, S_FOLD, dtype, out=1)
        acc = SkillAccumulator(1, 9, 31, device="cuda")
        pred, steps, dropped = predict_stream(net, ds, lanes=2, halo=(2, 3), skill=acc)
        pix, _, sample = acc.sums()
        return {"pred": pred, "steps": torch.from_numpy(steps), "pix": torch.from_numpy(pix), "sample": torch.from_numpy(sample)}
    return run


def slab_scenario(pkg, dtype):
    from nasa_niswan_amd.trainer import FusedTrainer

    def run(gt):
        ds = _dataset(gt, period="train", padding=(13, 37), in_channels=8, sequence_length=3, levels=1, n_steps=24, grid=(9, 31),
                      static_channels=3)
        net = build_net(pkg, gt, (8, [20, 12], [5, 3]), dtype, out=1)
        tr = FusedTrainer(net, lr=1e-3, halo=(2, 3))
        res = {}
        for j, idx in enumerate(([0, 5], [3, 9])):
            sb, y = ds.slab_batch(idx)
            res[f"loss.{j}"] = tr.step(sb, y).detach().clone()
        X, _ = ds.device_batch([1, 2])
        res["X"], res["bucket"], res["bucket.grad"] = X, tr.flat.data, tr.flat.grad
        eng = net._engine(tr.device)
        (ws,) = eng.pool[(2, 3, 13, 37, True, False)]
        res["xs"] = ws.xs                              # the input slab the preproc kernel filled directly, halo ring included
        return res
    return run


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("what", ["skill", "stream", "slab"])
def test_evaluation_streaming_and_the_slab_path(pkg, what, dtype):
    sc = {"skill": skill_scenario, "stream": stream_scenario, "slab": slab_scenario}[what](pkg, dtype)
    three_runs(f"{what}-{dtype}", sc, row_stride((8, [20, 12], [5, 3]), (13, 37)))


# ------------------------------------------------------------------------------ the harness sees a stray byte on the device
def test_a_byte_in_a_workspace_slabs_guard_is_reported_with_its_call_site(pkg):
    """After a passing poisoned run, one byte of the back guard of a Workspace slab is written by a host-issued torch index on
    the arena tensor (no kernel misbehaves): verify() must fail and name the slab's allocation in engine.py."""
    hit = {}

    def self_check(gt):
        slabs = [a for a in gt.find("engine.py") if a.kind == "empty" and a.dtype == torch.uint8 and a.nbytes]
        assert slabs, [a.site for a in gt.arenas]
        a = slabs[0]                                     # the gate stash of layer 0: the first `empty` uint8 slab of a Workspace
        a.arena[a.front + a.nbytes + 5] = 0x3C
        torch.cuda.synchronize()
        with pytest.raises(GA.GuardError) as e:
            gt.verify()
        msg = str(e.value)
        assert a.site in msg and "back guard" in msg and "1 byte(s)" in msg and f"[{a.nbytes + 5}, {a.nbytes + 5}]" in msg, msg
        assert msg.count("guard damaged") == 1 and "may exceed" not in msg, msg
        a.arena[a.front + a.nbytes + 5] = a.fill
        assert gt.verify() > 0
        hit["site"] = a.site

    three_runs("self-check", module_scenario(pkg, S_FOLD, (13, 37), "bf16"), row_stride(S_FOLD, (13, 37)), self_check)
    assert "engine.py" in hit["site"]


# ------------------------------------------------------------------------------ exact-size calls through the C ABI
def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _geom(lib, H, W, Pd):
    from nasa_niswan_amd._lib import NintGeom
    g = NintGeom()
    assert lib.nint_geom_make(C.byref(g), H, W, Pd) == 0
    return g


def _layer(lib, Cx, Ch, k, dt, xfold=0, wide=0):
    from nasa_niswan_amd._lib import NintLayer
    kc = lib.nint_kc(dt)
    rup = lambda a, b: (a + b - 1) // b * b
    ly = NintLayer()
    ly.Cx, ly.Ch, ly.k, ly.xfold, ly.wide = Cx, Ch, k, xfold, wide
    ly.Cxp, ly.Ch16, ly.Chp = rup(k * Cx if xfold else Cx, kc), rup(Ch, 16), rup(Ch, kc)
    return ly


class Exact:
    """buffers for one C-ABI call: `plain` = generous torch buffers (`slack` extra elements behind every scratch), else carved
    by a poisoning GuardedTorch at exactly the size asked for"""

    def __init__(self, plain: bool, stride=0):
        self.gt = None if plain else GA.GuardedTorch("poison", row_stride=stride)

    def empty(self, n, dtype, slack=4096):
        if self.gt is None:
            return torch.full((n + slack,), 0.25, dtype=torch.float32, device="cuda").to(dtype) if dtype.is_floating_point \
                else torch.full((n + slack,), 7, dtype=dtype, device="cuda")
        return self.gt.empty(n, dtype=dtype, device="cuda")

    def zeros(self, n, dtype):
        return torch.zeros(n, dtype=dtype, device="cuda") if self.gt is None else self.gt.zeros(n, dtype=dtype, device="cuda")

    def copy(self, t):
        return t.cuda() if self.gt is None else self.gt.guard_copy(t.cuda())

    def done(self):
        torch.cuda.synchronize()
        return 0 if self.gt is None else self.gt.verify()


def both_ways(name, call, stride=0):
    """call(Exact) -> {name: tensor}: on generous plain buffers, then on exactly sized poisoned ones; bitwise equal, guards whole"""
    a = call(Exact(True))
    torch.cuda.synchronize()
    ex = Exact(False, stride)
    b = call(ex)
    n = ex.done()
    assert set(a) == set(b)
    for k in a:
        assert GA.same_bits(a[k], b[k]), (name, k, "exactly sized poisoned buffers against generous plain ones")
        assert not b[k].is_floating_point() or not bool(torch.isnan(b[k].float()).any()), (name, k, "NaN")
    print(f"  {name}: {n} guarded allocations")


PACK_SHAPES = [(5, 20, 5, 1), (5, 20, 5, 0), (20, 12, 3, 0), (40, 32, 3, 0), (64, 32, 3, 0), (4, 8, 3, 0), (8, 4, 3, 0), (3, 5, 3, 0),
               (16, 32, 7, 0), (6, 16, 1, 0), (1, 16, 3, 1), (5, 16, 9, 1)]


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_pack_weights_at_exactly_the_queried_size_and_both_entries_agree(pkg, dt):
    """nint_pack_weights and nint_pack_weights_layers into images of exactly nint_packed_weight_bytes, poisoned: the guards stay
    whole, the images equal those of the same call on generous buffers (poisoned alike), the two entries give byte-identical
    Wf, Wd and bias_p, and the extents the gate kernels read are fully written: the forward image's sf * (4 Ch16 / 16) * 64 *
    EPL elements (sf K-steps: Cxp / KC * (k folded, k^2 plain) + Chp / KC * k^2), the whole dgrad image (Cxp + Chp) * 4 Ch16 *
    k^2 and the 4 Ch16 biases.  What nint_packed_weight_bytes reserves behind a FOLDED forward image (it has fewer K-steps
    than the dgrad image the size is taken from) and between the stencil / dense-K images of tiny layers is never written,
    and no kernel reads it: the engine zero-fills both images once (Memory contract)."""
    from nasa_niswan_amd._lib import NintLayer
    lib = pkg.load_library()
    es, kc = (2, 32) if dt else (4, 16)
    et = torch.bfloat16 if dt else torch.float32

    def written(i, res):
        Cx, Ch, k, xf = PACK_SHAPES[i]
        xf = int(xf and lib.nint_xfold_pays(Cx, k, dt))
        ly = _layer(lib, Cx, Ch, k, dt, xf)
        sf = ly.Cxp // kc * (k if xf else k * k) + ly.Chp // kc * k * k
        nf = sf * (4 * ly.Ch16 // 16) * 64 * (kc // 4)
        nd = (ly.Cxp + ly.Chp) * 4 * ly.Ch16 * k * k
        assert nf * es <= res[f"Wf.{i}"].numel() and nd * es <= res[f"Wd.{i}"].numel(), (PACK_SHAPES[i], nf, nd)
        for name, n in ((f"Wf.{i}", nf), (f"Wd.{i}", nd)):
            v = res[name][:n * es].view(et).float()
            assert not bool(torch.isnan(v).any()), (PACK_SHAPES[i], name, "an element of the image the kernels read is unwritten")
        assert not bool(torch.isnan(res[f"bias_p.{i}"]).any()), (PACK_SHAPES[i], "bias_p")

    def images(ex, layers_entry):
        res, keep = {}, []
        lys, Ws, bs = [], [], []
        for i, (Cx, Ch, k, xf) in enumerate(PACK_SHAPES):
            xf = int(xf and lib.nint_xfold_pays(Cx, k, dt))
            nbytes = lib.nint_packed_weight_bytes(Cx, Ch, k, dt, xf)
            assert nbytes > 0
            ly = _layer(lib, Cx, Ch, k, dt, xf)
            W = ex.copy(rnd(4 * Ch, Cx + Ch, k, k, seed=i))
            b = ex.copy(rnd(4 * Ch, seed=50 + i))
            # (plain: generous; both poisoned, so that an unwritten element of a read extent shows as NaN)
            full = lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
            Wf = full(nbytes + 4096) if ex.gt is None else ex.gt.empty(nbytes, dtype=torch.uint8, device="cuda")
            Wd = full(nbytes + 4096) if ex.gt is None else ex.gt.empty(nbytes, dtype=torch.uint8, device="cuda")
            bp = full(4 * (4 * ly.Ch16 + 64)).view(torch.float32) if ex.gt is None else ex.gt.empty(4 * ly.Ch16, dtype=torch.float32, device="cuda")
            ly.Wf, ly.Wd, ly.bias_p = Wf.data_ptr(), Wd.data_ptr(), bp.data_ptr()
            keep += [W, b]
            lys.append(ly); Ws.append(W); bs.append(b)
            if not layers_entry:
                assert lib.nint_pack_weights(P(W), P(b), P(Wf), P(Wd), P(bp), Cx, Ch, k, xf, dt, None) == 0, PACK_SHAPES[i]
            res[f"Wf.{i}"], res[f"Wd.{i}"], res[f"bias_p.{i}"] = Wf[:nbytes], Wd[:nbytes], bp[:4 * ly.Ch16]
        if layers_entry:
            for j in range(0, len(lys), 8):       # (NINT_MAX_LAYERS per call)
                n = len(lys[j:j + 8])
                assert lib.nint_pack_weights_layers((C.c_void_p * n)(*[w.data_ptr() for w in Ws[j:j + 8]]),
                                                    (C.c_void_p * n)(*[v.data_ptr() for v in bs[j:j + 8]]),
                                                    (NintLayer * n)(*lys[j:j + 8]), n, dt, None) == 0
        torch.cuda.synchronize()
        return res

    out = {}
    for entry in (False, True):
        a = images(Exact(True), entry)
        ex = Exact(False)
        b = images(ex, entry)
        ex.done()
        for k in a:
            assert GA.same_bits(a[k], b[k]), (k, "layers" if entry else "single", "exactly sized images against generous ones")
        for i in range(len(PACK_SHAPES)):
            written(i, b)
        out[entry] = b
    for k in out[False]:
        assert GA.same_bits(out[False][k], out[True][k]), (k, "nint_pack_weights and nint_pack_weights_layers differ")


WGRAD_SHAPES = [("fold-5-20-k5", 5, 20, 5, 1, 0), ("64-32-narrow", 64, 32, 3, 0, 1), ("64-32-wide", 64, 32, 3, 0, 2),
                ("40-32", 40, 32, 3, 0, 0), ("16-32-k7", 16, 32, 7, 0, 0), ("6-16-k1", 6, 16, 1, 0, 0), ("4-8-tiny", 4, 8, 3, 0, 0)]


@pytest.mark.parametrize("N", [1, 6])
@pytest.mark.parametrize("name,Cx,Ch,k,xf,wide", WGRAD_SHAPES, ids=[s[0] for s in WGRAD_SHAPES])
def test_conv_wgrad_at_exactly_the_queried_workspace(pkg, name, Cx, Ch, k, xf, wide, N):
    """nint_conv_wgrad with a split-K workspace of exactly nint_wgrad_workspace_bytes -- no slack behind it -- on N = 1 and 6
    images of a 13 x 37 grid, both kernel families and a folded x source: NINT_OK (the query is an upper bound whatever N is),
    the guards whole, dW / db the bits of the call on a generous workspace."""
    lib = pkg.load_library()
    dt = 1
    H, W = 13, 37
    xf = int(xf and lib.nint_xfold_pays(Cx, k, dt))
    ly = _layer(lib, Cx, Ch, k, dt, xf, wide)
    g = _geom(lib, H, W, k // 2)
    need = lib.nint_wgrad_workspace_bytes(C.byref(ly), dt, 256)
    assert need > 0 and need % 4 == 0
    bf = torch.bfloat16
    Pd = g.P

    def slab(n, Cp, Cv, seed, scale):
        t = torch.zeros(n, g.Hh, g.Wh, Cp)
        t[:, Pd:Pd + H, Pd:Pd + W, :Cv] = rnd(n, H, W, Cv, seed=seed, scale=scale)
        return t.to(bf)

    def call(ex):
        xs = ex.copy(slab(N, ly.Cxp, (k * Cx if xf else Cx), 1, 1.0))
        hh = ex.copy(slab(N, ly.Chp, Ch, 2, 0.5))
        dG = ex.copy(slab(N, 4 * ly.Ch16, 4 * ly.Ch16, 3, 0.1))
        dW = ex.empty(4 * Ch * (Cx + Ch) * k * k, torch.float32, slack=0)
        db = ex.empty(4 * Ch, torch.float32, slack=0)
        part = ex.empty(need // 4, torch.float32)
        nbytes = need if ex.gt is not None else part.numel() * 4
        rc = lib.nint_conv_wgrad(C.byref(ly), C.byref(g), dt, N, P(dG), P(xs), P(hh), P(dW), P(db), P(part), nbytes, 256, None)
        assert rc == 0, (name, N, rc, "nint_wgrad_workspace_bytes is too small for this N: the query's 'upper bound' is wrong")
        return {"dW": dW, "db": db}

    both_ways(f"wgrad {name} N={N}", call, g.Wh * 4 * ly.Ch16 * 2)


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("seq", [False, True], ids=["last-step", "sequence"])
@pytest.mark.parametrize("Ch,O", [(16, 20), (48, 3), (48, 20)])      # (the last: nout > 512, the register-tiled first stage)
def test_head_backward_at_the_scratch_switch(pkg, dt, seq, Ch, O):
    """nint_head_bwd_acc / nint_head_bwd_seq_acc with a scratch of exactly 256 * nout * 4 bytes (nout = O * (Ch + 1): the switch
    in head.hip to the two-stage reduction) in a poisoned arena, and with one float less, where the one-workgroup-per-output
    kernel runs without touching the scratch.  The exact-size call equals the generous one bit for bit.  The two branches do
    NOT share a summation order (per-workgroup partials folded afterwards against one running sum per output), so they are
    compared at the project's existing head tolerance, 1e-5 of the gradient's largest element (test_gpu_small_kernels)."""
    lib = pkg.load_library()
    B, T, H, W, Pd = 2, 3, 13, 37, 2
    g = _geom(lib, H, W, Pd)
    kc = lib.nint_kc(dt)
    Chp = (Ch + kc - 1) // kc * kc
    et = torch.bfloat16 if dt else torch.float32
    nout = O * (Ch + 1)
    N = T * B if seq else B
    hs = torch.zeros((T + 1) * B, g.Hh, g.Wh, Chp)
    hs[:, Pd:Pd + H, Pd:Pd + W, :Ch] = rnd((T + 1) * B, H, W, Ch, seed=4)
    w = rnd(O, Ch, seed=5, scale=0.3)
    dp = rnd(B, (T if seq else 1) * O, H, W, seed=6)

    def make(scratch_floats):
        def call(ex):
            h, wd, dpd = ex.copy(hs.to(et)), ex.copy(w), ex.copy(dp)
            dw, db = ex.empty(O * Ch, torch.float32, slack=0), ex.empty(O, torch.float32, slack=0)
            dh = ex.empty(N * H * W * Chp, et, slack=0)
            scr = ex.empty(scratch_floats, torch.float32)
            nbytes = scratch_floats * 4 if ex.gt is not None else scr.numel() * 4
            if scratch_floats < 256 * nout:
                nbytes = scratch_floats * 4                      # (the plain run takes the same branch)
            if seq:
                rc = lib.nint_head_bwd_seq_acc(P(h), B, T, Ch, Chp, O, P(wd), P(dpd), None, P(dh), P(dw), P(db), 0, C.byref(g), dt,
                                               P(scr), nbytes, None)
            else:
                rc = lib.nint_head_bwd_acc(P(h), T * B, B, Ch, Chp, O, P(wd), P(dpd), P(dh), P(dw), P(db), 0, C.byref(g), dt,
                                           P(scr), nbytes, None)
            assert rc == 0, rc
            call.last = {"dw": dw.clone(), "db": db.clone()}
            return {"dw": dw, "db": db, "dh": dh}
        return call

    at, below = make(256 * nout), make(256 * nout - 1)
    both_ways(f"head_bwd seq={seq} Ch={Ch} O={O} dt={dt} at the switch", at, g.Wh * Chp * 4)
    a = at.last
    both_ways(f"head_bwd seq={seq} Ch={Ch} O={O} dt={dt} one float below", below, g.Wh * Chp * 4)
    b = below.last
    for k in ("dw", "db"):
        err = float((a[k].double() - b[k].double()).abs().max())
        lim = 1e-5 * float(a[k].double().abs().max()) + 1e-9
        print(f"    {k}: two-stage against one-workgroup-per-output {err:.3e} (limit {lim:.3e})")
        assert err <= lim, (k, err, lim)


@pytest.mark.parametrize("N,O,grid,crop,Ch", [(2, 2, (13, 37), (9, 31), 12), (3, 1, (8, 32), (8, 32), 16), (70, 1, (3, 5), (2, 3), 5)])
def test_skill_passes_at_exactly_the_queried_scratch(pkg, N, O, grid, crop, Ch):
    """nint_skill_accum and nint_head_skill_accum with nint_skill_scratch_bytes of scratch, poisoned (N = 70: split internally)"""
    from nasa_niswan_amd._lib import NINT_SKILL_PIX, NINT_SKILL_SAMPLE
    lib = pkg.load_library()
    (H, W), (Hc, Wc) = grid, crop
    oy, ox = (H - Hc) // 2, (W - Wc) // 2
    need = lib.nint_skill_scratch_bytes(N, O, Hc, Wc)
    assert need > 0 and need % 8 == 0
    nslots = 2
    slots = (C.c_int32 * N)(*[(n % 3) - 1 for n in range(N)])
    pred, y = rnd(N, O, H, W, seed=1), rnd(N, O, Hc, Wc, seed=2)
    row_w = torch.cos(torch.linspace(-0.7, 0.7, Hc, dtype=torch.float64))
    for dt in (0, 1):
        Pd = 1
        g = _geom(lib, H, W, Pd)
        kc = lib.nint_kc(dt)
        Chp = (Ch + kc - 1) // kc * kc
        et = torch.bfloat16 if dt else torch.float32
        hs = torch.zeros(N, g.Hh, g.Wh, Chp)
        hs[:, Pd:Pd + H, Pd:Pd + W, :Ch] = rnd(N, H, W, Ch, seed=3)
        w, b = rnd(O, Ch, seed=4, scale=0.3), rnd(O, seed=5)

        def call(ex):
            res = {}
            for fused in (False, True):
                pix = ex.zeros(nslots * NINT_SKILL_PIX * O * Hc * Wc, torch.float64)
                sample = ex.empty(N * O * NINT_SKILL_SAMPLE, torch.float64, slack=0)
                scr = ex.empty(need // 8, torch.float64)
                nbytes = need if ex.gt is not None else scr.numel() * 8
                yd, rw = ex.copy(y), ex.copy(row_w)
                hd, wd, bd, pd = ex.copy(hs.to(et)), ex.copy(w), ex.copy(b), ex.copy(pred)      # (alive until the launch has run)
                if fused:
                    po = ex.empty(N * O * Hc * Wc, torch.float32, slack=0)
                    rc = lib.nint_head_skill_accum(P(hd), 0, N, Ch, Chp, O, P(wd), P(bd), P(yd), slots, nslots,
                                                   P(rw), P(pix), P(sample), P(po), P(scr), nbytes, C.byref(g), oy, ox, Hc, Wc, dt, None)
                    res["pred_out"] = po
                else:
                    rc = lib.nint_skill_accum(P(pd), P(yd), slots, nslots, P(rw), P(pix), P(sample), P(scr), nbytes, N, O, H, W,
                                              oy, ox, Hc, Wc, None)
                assert rc == 0, (fused, rc)
                torch.cuda.synchronize()
                res[f"pix.{int(fused)}"], res[f"sample.{int(fused)}"] = pix, sample
            return res
        both_ways(f"skill N={N} O={O} {grid} dt={dt}", call, g.Wh * Chp * 4)
        if dt == 0:
            # one byte less is refused before any launch
            ex = Exact(True)
            assert lib.nint_skill_accum(P(ex.copy(pred)), P(ex.copy(y)), slots, nslots, None, P(ex.zeros(nslots * 5 * O * Hc * Wc, torch.float64)),
                                        P(ex.empty(N * O * 8, torch.float64)), P(ex.empty(need // 8, torch.float64)), need - 1, N, O, H, W, oy, ox,
                                        Hc, Wc, None) == -1


@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_grad_norm_and_the_guarded_grouped_adam_at_exactly_the_queried_scratch(pkg, n):
    from nasa_niswan_amd._lib import NINT_MAX_OPT_GROUPS, NINT_OPT_STATE, NintOptGroup
    lib = pkg.load_library()
    need = lib.nint_grad_norm_scratch_bytes()
    assert need > 0 and need % 8 == 0
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2, scale=0.1)
    cut = n // 3
    rows = [(0, cut, 1e-3, 0.0), (cut, n, 5e-4, 1e-2)] if cut else [(0, n, 1e-3, 1e-2)]
    tab = (NintOptGroup * len(rows))(*[NintOptGroup(*r) for r in rows])

    def call(ex):
        gd = ex.copy(g0)
        out = ex.empty(2, torch.float64, slack=0)
        scr = ex.empty(need // 8, torch.float64)
        nbytes = need if ex.gt is not None else scr.numel() * 8
        assert lib.nint_grad_norm_flat(P(gd), n, 0.5, P(out), P(scr), nbytes, None) == 0
        p, m, v = ex.copy(p0), ex.zeros(n, torch.float32), ex.zeros(n, torch.float32)
        state, gstate = ex.zeros(NINT_OPT_STATE, torch.float64), ex.zeros(2 * NINT_MAX_OPT_GROUPS, torch.float64)
        scr2 = ex.empty(need // 8, torch.float64)
        for _ in range(2):
            assert lib.nint_adam_flat_groups_guarded(P(p), P(gd), P(m), P(v), tab, len(tab), 0.5, 0.999, 1e-8, 0.5, 0.05, 1, P(state), P(gstate),
                                                     P(scr2), nbytes if ex.gt is None else need, None) == 0
        return {"norm": out, "p": p, "m": m, "v": v, "state": state, "gstate": gstate[:2 * len(rows)]}

    both_ways(f"grad norm + grouped guarded adam n={n}", call)
    ex = Exact(True)
    assert lib.nint_grad_norm_flat(P(ex.copy(g0)), n, 1.0, P(ex.empty(2, torch.float64)), P(ex.empty(need // 8, torch.float64)), need - 8, None) == -1


@pytest.mark.parametrize("N,O,grid,halo", [(2, 2, (13, 37), (2, 3)), (3, 1, (8, 32), (0, 0)), (6, 5, (100, 154), (5, 5))])
def test_loss_entries_at_exactly_their_scratch_constants(pkg, N, O, grid, halo):
    """nint_loss_mse_l1_crop, _weighted and nint_loss_crop_spec with loss_out of exactly NINT_LOSS_SCRATCH_FLOATS /
    NINT_LOSS_SPEC_SCRATCH_FLOATS floats, poisoned (the largest grid fills the partial-sum launch: 6 * 5 * 90 * 144 elements)"""
    from nasa_niswan_amd._lib import NINT_LOSS_SCRATCH_FLOATS, NINT_LOSS_SPEC_SCRATCH_FLOATS, NINT_LOSS_STATS, NintLossSpec
    lib = pkg.load_library()
    (H, W), (oy, ox) = grid, halo
    Hc, Wc = H - 2 * oy, W - 2 * ox
    pred, y = rnd(N, O, H, W, seed=1), rnd(N, O, Hc, Wc, seed=2)
    wm = rnd(Hc, Wc, seed=3).abs()
    wm[0, 0] = 0.0
    wsum = float(wm.double().sum())
    ow = rnd(O, seed=4).abs() + 0.1

    def call(ex):
        res = {}
        pd, yd, wd, od = ex.copy(pred), ex.copy(y), ex.copy(wm), ex.copy(ow)
        for name in ("plain", "weighted", "spec"):
            dp = ex.empty(N * O * H * W, torch.float32, slack=0)
            stats = ex.zeros(NINT_LOSS_STATS, torch.float64)
            scr = ex.empty(NINT_LOSS_SPEC_SCRATCH_FLOATS if name == "spec" else NINT_LOSS_SCRATCH_FLOATS, torch.float32)
            if name == "plain":
                rc = lib.nint_loss_mse_l1_crop(P(pd), P(yd), P(dp), P(scr), P(stats), N, O, H, W, oy, ox, Hc, Wc, None)
            elif name == "weighted":
                rc = lib.nint_loss_mse_l1_crop_weighted(P(pd), P(yd), P(wd), wsum, P(dp), P(scr), P(stats), N, O, H, W, oy, ox, Hc, Wc, None)
            else:
                sp = NintLossSpec()
                sp.mse, sp.l1, sp.huber, sp.delta = 0.5, 2.0, 1.5, 0.7
                sp.ow, sp.now, sp.osum = od.data_ptr(), O, float(ow.double().sum())
                rc = lib.nint_loss_crop_spec(P(pd), P(yd), P(wd), wsum, C.byref(sp), P(dp), P(scr), P(stats), N, O, H, W, oy, ox, Hc, Wc, None)
            assert rc == 0, (name, rc)
            res[f"loss.{name}"], res[f"dpred.{name}"], res[f"stats.{name}"] = scr[:1], dp, stats
        return res

    both_ways(f"loss N={N} O={O} {grid}", call)
