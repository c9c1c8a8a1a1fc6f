"""How NaN and inf spread through the device path, and that a bad batch leaves no trace.

One element of the input (or of a given state) is NaN, +inf, -inf or 1e30 (tests/nonfinite_cases.py).  Where the result is
non-finite is compared elementwise with the CPU oracle's sets -- an exact statement about which pixels, taps, tiles, time
steps and lanes every launch read -- the finite part under the standing gates, and everything the bad element cannot reach
bit for bit with the device's own clean run.  Then path by path: a subject that ran a bad call and a clean one against a twin
that never saw the bad call, bit for bit; and a stateful trainer with skip_nonfinite, whose bad lane restarts from the zero
state instead of carrying the NaN into every later chunk.

The (b) figures of `compare` are inside the standing gates (f32 outputs rtol 1e-4 / atol 1e-5, f32 gradients 1e-3 max|ref|,
bf16 rel-L2 2e-2; worst measured over its gate: f32 1e-2 in group 1 and 2.3e-2 in the state cases of group 2, bf16 0.46) with
one exception, measured and set as the issue prescribes: the bias gradient of the 7-channel stack S4 in bf16, rel-L2 2.034e-2
at worst over tile rows 1 / 2 / 8 and the three places, gate 4.07e-2 (nonfinite_cases.MEASURED_GATES).  Each test prints its
worst figures.

THREE places where the device's non-finite SET differs from the oracle's are known: dX of a NaN case where
layer 0's input folds, dW of layer 0 with an inf in the last grid row (`deviations`), and the channel-padding columns of dh /
dG / dc after a NaN pass (`BWD_PAD`).  For the first two, every case of group 1 and 2 -- every tile height, wave mode and fuse
mask -- asserts the statement that does hold (NC.compare_within: the device's set covers the oracle's, stays inside it widened
as the cause allows, lane 1 and everything outside keep the clean run's bits), the exact set is a strict expected failure per
stack and place, and the measured size of the deviation is asserted beside it.  Stack S5 does not fold: there dX of a NaN is
compared exactly, under every wave mode and fuse mask.  The file prints its wall time (7 s on one MI355X)."""
import math
import time

import numpy as np
import pytest
import torch

import nonfinite_cases as NC
from oracle import stored_audit as SA

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
FUSE_MASKS = [0x40000404, 0x40000202, 0x40020404]       # tests/test_gpu_stored_audit.py
ALL_VALUES = list(NC.VALUES)
ALL_PLACES = list(range(len(NC.PLACES)))
HALO = (2, 2)
HC, WC = NC.H - 2 * HALO[0], NC.W - 2 * HALO[1]
NAN = float("nan")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    t0 = time.time()        # (this file's tests only: the clock starts at its first test, not at collection)
    yield p
    print(f"\n  test_gpu_nonfinite wall time {time.time() - t0:.1f} s")


# --------------------------------------------------------------------------- helpers
def make_net(pkg, stack, dtype, rows=0, fuse=None, seed=0):
    """a module of the stack with its engine built under FORCE_TILE_ROWS = rows (and FUSE_BWD = fuse for its workspaces: the
    caller keeps that knob set while it runs the module, see `knobs`)"""
    from nasa_niswan_amd import engine
    s = NC.STACKS[stack]
    net = pkg.ConvLSTM(s["C"], s["hidden"], s["ks"], len(s["hidden"]), out_channels=NC.OUT, compute_dtype=dtype).cuda()
    net.load_state_dict(NC.params_of(stack, seed))
    engine.FORCE_TILE_ROWS = rows
    try:
        net._engine(next(net.parameters()).device)
    finally:
        engine.FORCE_TILE_ROWS = 0
    return net


class knobs:
    """FORCE_WAVE / FUSE_BWD for the calls inside, restored after"""

    def __init__(self, wave=None, fuse=None):
        self.wave, self.fuse = wave, fuse

    def __enter__(self):
        from nasa_niswan_amd import engine
        self.keep = (engine.FORCE_WAVE, engine.FUSE_BWD)
        engine.FORCE_WAVE = self.wave
        if self.fuse is not None:
            engine.FUSE_BWD = self.fuse

    def __exit__(self, *exc):
        from nasa_niswan_amd import engine
        engine.FORCE_WAVE, engine.FUSE_BWD = self.keep


def device_pass(net, X, wgt):
    """net(x) with autograd on loss = (pred * wgt).sum(): {pred, dX, <parameter name>: .grad} on the CPU"""
    x = X.cuda().requires_grad_(True)
    net.zero_grad(set_to_none=True)
    pred = net(x)
    (pred * wgt.cuda()).sum().backward()
    res = {"pred": pred.detach().cpu(), "dX": x.grad.cpu()}
    for k, p in net.named_parameters():
        res[k] = p.grad.detach().cpu().clone()
    return res


def assert_same(a, b, what=""):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert NC.same_bits(a[k], b[k]), f"{what} {k}: differs bit for bit"


LAST = 2              # PLACES[2]: the last pixel (last row, last column) at the last step
W0 = "layers.0.conv.weight"


def deviations(stack, dtype, value, place, ref):
    """{tensor: reach} for the tensors of a case whose NON-FINITE SET is known to differ from the reference's (DESIGN.md 4.12,
    found by this file).  They leave the exact comparison, and in its place NC.compare_within runs on them under every knob
    setting: the device's set covers the oracle's, stays inside `reach`, and outside it nothing moves.  The exact sets are
    pinned below as strict expected failures with the measured counts.
      dX of a NaN case where layer 0's input folds (NC.folds: S1 - S4, not S5): the folded input gradient is computed over all
        k x k taps with zero weights off the centre column, and NaN * 0 widens the set by k/2 columns each way
      dW of layer 0 with an inf in the last grid row: the weight-gradient kernels sum over the slack rows below the grid (and,
        where the input is not folded, the slack columns beside it), where dG is a stored zero, and 0 * inf makes more taps of
        the bad input channel non-finite"""
    out = {}
    if value == "nan" and NC.folds(stack, dtype):
        out["dX"] = NC.widened(NC.nonfinite(ref["dX"]), NC.STACKS[stack]["ks"][0] // 2)
    if value in ("pinf", "ninf") and place == LAST:
        reach = torch.zeros_like(ref[W0], dtype=torch.bool)
        reach[:, NC.bad_channel(stack)] = True
        out[W0] = reach
    return out


def spread_cases(pkg, stack, dtype, values, places, rows=0, wave=None, fuse=None):
    """every (value, place) through one module under the given knobs; all failures reported together"""
    net = make_net(pkg, stack, dtype, rows)
    log, failed = [], []
    with knobs(wave, fuse):
        clean = device_pass(net, *NC.batch(stack))
        for place in places:
            ns = NC.nan_set(stack, place)
            for value in values:
                tag = f"{stack} {dtype} rows={rows} wave={wave} fuse={fuse} {value}@{NC.PLACES[place]}"
                dev = device_pass(net, *NC.batch(stack, value, place))
                ref = NC.oracle_run(stack, value, place)
                known = deviations(stack, dtype, value, place, ref)
                gates = NC.measured_gates(stack, dtype)
                try:
                    NC.compare(dev, ref, clean, ns, dtype, log=log, tag=tag, keys=set(ref) - set(known), gates=gates)
                    for k, reach in known.items():
                        NC.compare_within(dev, ref, clean, k, reach, dtype, lanes=k == "dX", log=log, tag=tag, gates=gates)
                except AssertionError as e:
                    failed.append(str(e))
        again = device_pass(net, *NC.batch(stack))
    worst = {}
    for _, k, err, gate in log:
        kind = "out" if NC.is_forward_key(k) else "grad"
        worst[kind] = max(worst.get(kind, 0.0), err / gate)
    print(f"  {stack} {dtype} rows={rows} wave={wave} fuse={fuse if fuse is None else hex(fuse)}: {len(values) * len(places)} cases, "
          "worst err / gate " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())), flush=True)
    assert not failed, "\n".join(failed)
    assert_same(again, clean, "the clean pass after the bad ones")


# --------------------------------------------------------------------------- 1. spread, net(x) with autograd
@pytest.mark.parametrize("rows", [0, 4, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s1_every_value_and_place(pkg, dtype, rows):
    """folded thin input, P = 2, eight padded hidden channels in layer 0 (the columns whose pre-activation is inf * 0 unless
    the gate kernel pins it to zero), tiny top layer"""
    spread_cases(pkg, "S1", dtype, ALL_VALUES, ALL_PLACES, rows=rows)


@pytest.mark.parametrize("wave", [0, 1, 4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s2_merged_grids(pkg, dtype, wave):
    spread_cases(pkg, "S2", dtype, ALL_VALUES, [NC.SEAM], wave=wave)


@pytest.mark.parametrize("fuse", FUSE_MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s2_fused_schedules(pkg, dtype, fuse):
    spread_cases(pkg, "S2", dtype, ALL_VALUES, [NC.SEAM], fuse=fuse)


@pytest.mark.parametrize("rows", [1, 2, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s3_tiny_families(pkg, dtype, rows):
    """1 / 2 / 8: the stencil, dense-K and padded-tile gate kernels of an 8-channel layer"""
    spread_cases(pkg, "S3", dtype, ["nan", "pinf"], ALL_PLACES, rows=rows)


@pytest.mark.parametrize("rows", [1, 2, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s4_tiny_families_with_a_padding_channel(pkg, dtype, rows):
    """7 hidden channels: the stencil's last quad and the dense-K kernel's last pair hold one channel of zero weights"""
    spread_cases(pkg, "S4", dtype, ["nan", "pinf"], ALL_PLACES, rows=rows)


@pytest.mark.parametrize("rows", [0, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s5_unfolded_input(pkg, dtype, rows):
    """32 input channels do not fold: the plain x path of layer 0, forward and dgrad -- dX of a NaN compared EXACTLY"""
    assert not NC.folds("S5", dtype)
    spread_cases(pkg, "S5", dtype, ALL_VALUES, ALL_PLACES, rows=rows)


@pytest.mark.parametrize("wave", [0, 1, 4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s5_merged_grids(pkg, dtype, wave):
    """the exact dX probe on the paired dgrad launches and the BPTT pairs"""
    spread_cases(pkg, "S5", dtype, ALL_VALUES, [NC.SEAM], wave=wave)


@pytest.mark.parametrize("fuse", FUSE_MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_s5_fused_schedules(pkg, dtype, fuse):
    spread_cases(pkg, "S5", dtype, ALL_VALUES, [NC.SEAM], fuse=fuse)


# --------------------------------------------------------------------------- 1b. the known deviations of a set, pinned one by one
def one_case(pkg, stack, dtype, value, place):
    net = make_net(pkg, stack, dtype)
    return device_pass(net, *NC.batch(stack, value, place)), device_pass(net, *NC.batch(stack))


def extra(dev, ref, key):
    """(elements non-finite on the device only, on the oracle only)"""
    got, want = NC.nonfinite(dev[key]), NC.nonfinite(ref[key])
    return int((got & ~want).sum()), int((want & ~got).sum())


# (stack, place) -> elements of dX that are non-finite on the device beyond the oracle's set, measured (f32 and bf16 alike):
# whole pixels, k/2 columns each side of the set.  S4 has S3's input and fold; S5 does not fold and is exact (group 1).
DX_EXTRA = {("S1", 0): 370, ("S1", 1): 390, ("S1", 2): 270, ("S2", 1): 1287,
            ("S3", 0): 72, ("S3", 1): 172, ("S3", 2): 48, ("S4", 0): 72, ("S4", 1): 172, ("S4", 2): 48}
DX_FOLD = "the folded input gradient: NaN * 0 at the zero-weight taps off the centre column widens dX's set by k/2 columns"


@pytest.mark.xfail(strict=True, reason=DX_FOLD)
@pytest.mark.parametrize("stack,place", list(DX_EXTRA))
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_dx_set_is_the_oracles(pkg, dtype, stack, place):
    dev, clean = one_case(pkg, stack, dtype, "nan", place)
    NC.compare(dev, NC.oracle_run(stack, "nan", place), clean, NC.nan_set(stack, place), dtype, keys=["dX"])


@pytest.mark.parametrize("stack,place", list(DX_EXTRA))
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_dx_set_is_the_oracles_within_the_fold(pkg, dtype, stack, place):
    """what holds instead (and under every knob, in group 1): the device's set covers the oracle's and stays inside it widened by
    k/2 columns each way; outside that, and in lane 1, dX has the clean run's bits.  The measured size of the deviation is
    asserted, so a change of it is noticed."""
    dev, clean = one_case(pkg, stack, dtype, "nan", place)
    ref = NC.oracle_run(stack, "nan", place)
    NC.compare_within(dev, ref, clean, "dX", deviations(stack, dtype, "nan", place, ref)["dX"], dtype)
    assert extra(dev, ref, "dX") == (DX_EXTRA[stack, place], 0)


# (stack, value) -> entries of layer 0's dW non-finite on the device beyond the oracle's set, +-inf at the last pixel, measured.
# S3: the oracle's 128 (2 x 2 taps inside the grid, 32 gate channels) and the 64 of two taps that look up from the slack row.
# S1 (k = 5, 96 gate channels, 3 x 3 taps inside): one slack row in f32 (3 more taps), two in bf16 (6) -- the reduction's pixel
# tiles differ with the storage type.  S5 (not folded, 64 gate channels): all 9 taps, the 5 beyond the 2 x 2 from the slack
# row and the slack column.
DW_EXTRA = {("S1", "pinf"): dict(f32=288, bf16=576), ("S1", "ninf"): dict(f32=288, bf16=576), ("S3", "pinf"): 64,
            ("S4", "pinf"): 56, ("S5", "pinf"): 320}
DW_SLACK = "the weight-gradient kernels sum over the slack rows below the grid: a stored zero dG times the inf of the last row"


@pytest.mark.xfail(strict=True, reason=DW_SLACK)
@pytest.mark.parametrize("stack,value", list(DW_EXTRA))
@pytest.mark.parametrize("dtype", DTYPES)
def test_inf_in_the_last_row_dw_set_is_the_oracles(pkg, dtype, stack, value):
    dev, clean = one_case(pkg, stack, dtype, value, LAST)
    NC.compare(dev, NC.oracle_run(stack, value, LAST), clean, NC.nan_set(stack, LAST), dtype, keys=[W0])


@pytest.mark.parametrize("stack,value", list(DW_EXTRA))
@pytest.mark.parametrize("dtype", DTYPES)
def test_inf_in_the_last_row_dw_set_stays_in_its_channel(pkg, dtype, stack, value):
    """what holds instead (and under every knob, in group 1): the oracle's entries are non-finite, every other non-finite one
    is of the same input channel, the finite ones are inside the gate; the measured size of the deviation is asserted"""
    dev, clean = one_case(pkg, stack, dtype, value, LAST)
    ref = NC.oracle_run(stack, value, LAST)
    NC.compare_within(dev, ref, clean, W0, deviations(stack, dtype, value, LAST, ref)[W0], dtype, lanes=False)
    n = DW_EXTRA[stack, value]
    assert extra(dev, ref, W0) == (n[dtype] if isinstance(n, dict) else n, 0)


# --------------------------------------------------------------------------- 2. spread through a given state
def state_data(stack):
    rng = np.random.default_rng(4121)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    hid = NC.STACKS[stack]["hidden"]
    h0 = [0.5 * f(NC.B, ch, NC.H, NC.W) for ch in hid]
    c0 = [f(NC.B, ch, NC.H, NC.W) for ch in hid]
    Rh = [f(NC.B, ch, NC.H, NC.W) for ch in hid]
    Rc = [f(NC.B, ch, NC.H, NC.W) for ch in hid]
    return h0, c0, Rh, Rc


def device_state_pass(net, X, wgt, h0, c0, Rh, Rc):
    x = X.cuda().requires_grad_(True)
    hs = [v.cuda().requires_grad_(True) for v in h0]
    cs = [v.cuda().requires_grad_(True) for v in c0]
    net.zero_grad(set_to_none=True)
    pred, out = net(x, list(zip(hs, cs)), return_state=True)
    loss = (pred * wgt.cuda()).sum()
    res = {}
    for l, (h, c) in enumerate(out):
        loss = loss + (h * Rh[l].cuda()).sum() + (c * Rc[l].cuda()).sum()
        res[f"h_T.{l}"], res[f"c_T.{l}"] = h.detach().cpu(), c.detach().cpu()
    loss.backward()
    res["pred"], res["dX"] = pred.detach().cpu(), x.grad.cpu()
    for k, p in net.named_parameters():
        res[k] = p.grad.detach().cpu().clone()
    for l in range(len(hs)):
        res[f"dh0.{l}"], res[f"dc0.{l}"] = hs[l].grad.cpu(), cs[l].grad.cpu()
    return res


@pytest.mark.parametrize("part", ["all but dX", pytest.param("dX", marks=pytest.mark.xfail(strict=True, reason=(
    "the folded input gradient again (test_nan_dx_set_is_the_oracles); measured 390 (h0) / 370 (c0) elements more than the "
    "oracle's 3510 / 2425")))])
@pytest.mark.parametrize("which,layer", [("h", 0), ("c", 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_through_a_given_state(pkg, dtype, which, layer, part):
    """one NaN in h0 of layer 0 / c0 of layer 1 (lane 0, the seam): pred, h_T, c_T, dX, dh0, dc0 and the parameter gradients
    are non-finite where the oracle's are; the rest of lane 0 and all of lane 1 keep the clean run's bits"""
    stack = "S1"
    X, wgt = NC.batch(stack)
    h0, c0, Rh, Rc = state_data(stack)
    params = NC.params_of(stack)
    ref_clean = NC.oracle_pass(params, X, wgt, h0, c0, (Rh, Rc))
    _, y, x = NC.PLACES[NC.SEAM]
    bad = [v.clone() for v in (h0 if which == "h" else c0)]
    bad[layer][0, NC.STACKS[stack]["hidden"][layer] // 2, y, x] = NAN
    hb, cb = (bad, c0) if which == "h" else (h0, bad)
    ref = NC.oracle_pass(params, X, wgt, hb, cb, (Rh, Rc))
    assert all(int(NC.nonfinite(v).sum()) == 0 for v in ref_clean.values())
    lane = [k for k, v in ref.items() if v.dim() == 4 and v.shape[0] == NC.B and "conv" not in k] + ["dX"]
    ns = {k: NC.nonfinite(ref[k][0]) for k in lane}
    assert 0 < int(ns["pred"].sum()) < ns["pred"].numel() / 2
    net = make_net(pkg, stack, dtype)
    clean = device_state_pass(net, X, wgt, h0, c0, Rh, Rc)
    dev = device_state_pass(net, X, wgt, hb, cb, Rh, Rc)
    log = []
    NC.compare(dev, ref, clean, ns, dtype, lane_keys=lane, log=log, tag=f"NaN in {which}0 of layer {layer} {dtype}",
               keys=["dX"] if part == "dX" else set(ref) - {"dX"})
    # ("all but dX": dX under the statement that holds of a folded input's gradient, and the measured size of its deviation)
    NC.compare_within(dev, ref, clean, "dX", NC.widened(NC.nonfinite(ref["dX"]), NC.STACKS[stack]["ks"][0] // 2), dtype, log=log)
    assert extra(dev, ref, "dX") == ({"h": 390, "c": 370}[which], 0)
    print(f"  NaN in {which}0 of layer {layer} {dtype} ({part}): worst err / gate {max([e / g for _, _, e, g in log] or [0.0]):.2e}")
    assert_same(device_state_pass(net, X, wgt, h0, c0, Rh, Rc), clean, "the clean pass after the bad one")


# --------------------------------------------------------------------------- 3. slab invariants after a bad pass
def slab_pass(eng, ws, X, dstate):
    """forward + backward in `ws` (run_audit's route): every slab read back, and copies of dW / db / dx"""
    eng.forward(ws, X.cuda())
    for l, (dh, dc) in enumerate(dstate):
        eng.set_state_grads(ws, l, dh.cuda(), dc.cuda())
    dWs, dbs, dx = eng.backward(ws, need_dx=True)
    torch.cuda.synchronize()
    st = SA.read_workspace(eng, ws, dx)
    out = dict(st["raw"])
    for l, (dW, db) in enumerate(zip(dWs, dbs)):
        out[f"dW{l}"], out[f"db{l}"] = dW.detach().cpu().clone(), db.detach().cpu().clone()
    out["dx"] = dx.detach().cpu().clone()
    return SA.geo_of(eng, ws), st["raw"], out


BWD_PAD = pytest.mark.xfail(strict=True, reason=(
    "after the NaN pass the channel-padding columns of dh (S1: Ch = 24 of 32; S2 bf16: Ch = 16 of Chp = 32), and from them "
    "those of dG and dc, hold NaN: the dgrad launch computes them as dG * 0 (zero weight rows).  Measured S1: dh0 1456 (f32) / "
    "1664 (bf16), dc0 1664 elements; S2 bf16: dh0 3952.  They sit next to real NaNs of the same pixels, reach nothing the "
    "reference keeps finite, and the next pass overwrites them (asserted below)"))


def forward_slab(name):
    return name == "xs" or name.rstrip("0123456789") in ("h", "c", "gates")


@pytest.mark.parametrize("stack,dtype,slabs", [
    ("S1", "f32", "forward"), ("S1", "bf16", "forward"), ("S2", "f32", "forward"), ("S2", "bf16", "forward"),
    pytest.param("S1", "f32", "backward", marks=BWD_PAD), pytest.param("S1", "bf16", "backward", marks=BWD_PAD),
    ("S2", "f32", "backward"), pytest.param("S2", "bf16", "backward", marks=BWD_PAD)])
def test_slab_invariants_after_bad_passes(pkg, dtype, stack, slabs):
    """NaN pass, +inf pass, clean pass in ONE workspace: the padding of every slab (halo, slack, channel-padding columns;
    oracle/stored_audit.py::check_padding) holds after each, and the clean pass leaves the bytes of a fresh engine's.
    `slabs`: the NaN pass's check in two parts -- x, h, c and the stash; dG, dh, dc (a known deviation where a layer has
    channel padding)"""
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    s = NC.STACKS[stack]
    L = len(s["hidden"])
    params = NC.params_of(stack)
    g = torch.Generator().manual_seed(4123)
    dstate = [(0.1 * torch.randn(NC.B, h, NC.H, NC.W, generator=g), 0.1 * torch.randn(NC.B, h, NC.H, NC.W, generator=g))
              for h in s["hidden"]]

    def engine_and_ws():
        eng = SeqEngine([LayerCfg(s["C"] if l == 0 else s["hidden"][l - 1], s["hidden"][l], s["ks"][l]) for l in range(L)],
                        dtype, "cuda")
        eng.pack_weights([params[f"layers.{l}.conv.weight"].cuda() for l in range(L)],
                         [params[f"layers.{l}.conv.bias"].cuda() for l in range(L)])
        return eng, eng.acquire(NC.B, NC.T, NC.H, NC.W, True, False)

    eng, ws = engine_and_ws()
    try:
        for value in ("nan", "pinf"):
            geo, raw, _ = slab_pass(eng, ws, NC.batch(stack, value, NC.SEAM)[0], dstate)
            if value == "nan":
                raw = {k: v for k, v in raw.items() if forward_slab(k) == (slabs == "forward")}
            bad = SA.check_padding(geo, raw)
            assert bad == [], (stack, dtype, value, bad)
        geo, raw, got = slab_pass(eng, ws, NC.batch(stack)[0], dstate)
        assert SA.check_padding(geo, raw) == []
    finally:
        eng.release(ws)
    eng2, ws2 = engine_and_ws()
    try:
        _, _, want = slab_pass(eng2, ws2, NC.batch(stack)[0], dstate)
    finally:
        eng2.release(ws2)
    assert_same(got, want, f"{stack} {dtype}: the clean pass after the bad ones against a fresh engine's")


# --------------------------------------------------------------------------- 4. nothing left behind, path by path
@pytest.mark.parametrize("wave", [0, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_forgets_a_bad_call(pkg, dtype, wave):
    """net(x): the workspace pool and the read-modify-write pieces of the paired launches"""
    X, wgt = NC.batch("S2")
    with knobs(wave):
        subject, twin = make_net(pkg, "S2", dtype), make_net(pkg, "S2", dtype)
        bad = device_pass(subject, NC.batch("S2", "nan", NC.SEAM)[0], wgt)
        assert int(NC.nonfinite(bad["pred"]).sum()) > 0
        assert_same(device_pass(subject, X, wgt), device_pass(twin, X, wgt), f"net(x) {dtype} wave={wave}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_state_call_forgets_a_bad_call(pkg, dtype):
    """net(x, return_state="device"): a bad call, then a clean call from no state, against a fresh module's first call"""
    X, _ = NC.batch("S1")
    subject, twin = make_net(pkg, "S1", dtype), make_net(pkg, "S1", dtype)
    with torch.no_grad():
        _, st_bad = subject(NC.batch("S1", "nan", NC.SEAM)[0].cuda(), return_state="device")
        assert any(int(NC.nonfinite(h).sum()) > 0 for h, _ in st_bad.tensors())
        p1, s1 = subject(X.cuda(), return_state="device")
        p2, s2 = twin(X.cuda(), return_state="device")
    assert NC.same_bits(p1, p2)
    for l in range(2):
        assert torch.equal(s1.h[l], s2.h[l]) and NC.same_bits(s1.c[l], s2.c[l]), l


def trainer_of(pkg, stack, dtype, B=NC.B, **kw):
    from nasa_niswan_amd.trainer import FusedTrainer
    net = make_net(pkg, stack, dtype)
    return FusedTrainer(net, lr=1e-3, betas=(0.5, 0.999), halo=HALO, **kw)


def chunks(stack, n, B=NC.B, T=NC.T, seq=False, seed=0):
    """n clean (X, y) pairs on the device; y is the (Hc, Wc) crop's target, per step with `seq`"""
    rng = np.random.default_rng(4124 + seed)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32)).cuda()
    C = NC.STACKS[stack]["C"]
    return [(f(B, T, C, NC.H, NC.W), f(B, T, NC.OUT, HC, WC) if seq else f(B, NC.OUT, HC, WC)) for _ in range(n)]


def poison_x(stack, X, lane=0, t=None):
    tt, y, x = NC.PLACES[NC.SEAM]
    X = X.clone()
    X[lane, tt if t is None else t, NC.bad_channel(stack), y, x] = NAN
    return X


def poison_y(y):
    y = y.clone()
    y[(0, 0) + (0,) * (y.dim() - 4) + (3, 3)] = NAN        # y[0, 0, 3, 3]; with a sequence target the first step's
    return y


def trainer_bits(tr):
    out = {"flat": tr.flat.data, "exp_avg": tr.optimizer.exp_avg, "exp_avg_sq": tr.optimizer.exp_avg_sq}
    if tr.state is not None:
        for l, (h, c) in enumerate(zip(tr.state.h, tr.state.c)):
            out[f"state.h{l}"], out[f"state.c{l}"] = h, c
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_twins(subject, twin, loss_s, loss_t, applied, skipped, what):
    assert not math.isnan(loss_t) and loss_s == loss_t, (what, loss_s, loss_t)
    assert_same(trainer_bits(subject), trainer_bits(twin), what)
    st = subject.grad_stats()
    assert (st["applied"], st["skipped"]) == (applied, skipped), (what, st)
    assert twin.grad_stats()["applied"] == applied, (what, twin.grad_stats())


@pytest.mark.parametrize("where", ["X", "y"])
@pytest.mark.parametrize("kw", [dict(), dict(sequence_loss=True), dict(bptt_segments=3)], ids=["plain", "seq", "segments"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_trainer_forgets_a_skipped_step(pkg, dtype, kw, where):
    """clean step, bad step, clean step against a twin that ran the two clean steps: loss, parameters and both moments
    bit for bit.  bptt_segments = 3 on T = 3: the NaN of X sits in the middle segment's time step."""
    seq = bool(kw.get("sequence_loss"))
    (X0, y0), (X1, y1), (X2, y2) = chunks("S2", 3, seq=seq)
    subject = trainer_of(pkg, "S2", dtype, skip_nonfinite=True, **kw)
    twin = trainer_of(pkg, "S2", dtype, skip_nonfinite=True, **kw)
    subject.step(X0, y0)
    bad = subject.step(poison_x("S2", X1), y1) if where == "X" else subject.step(X1, poison_y(y1))
    assert math.isnan(float(bad))
    ls = float(subject.step(X2, y2))
    twin.step(X0, y0)
    lt = float(twin.step(X2, y2))
    assert_twins(subject, twin, ls, lt, 2, 1, f"trainer {dtype} {kw} bad {where}")
    assert twin.grad_stats()["skipped"] == 0


@pytest.mark.parametrize("bad_at", [0, 1])
@pytest.mark.parametrize("where", ["X", "y"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulation_drops_the_whole_group(pkg, dtype, where, bad_at):
    """accumulate_steps = 2: a clean group, a group whose first / second micro-batch is bad (dropped: nothing moves), a clean
    group -- the twin's two groups"""
    data = chunks("S1", 6)
    subject = trainer_of(pkg, "S1", dtype, skip_nonfinite=True, accumulate_steps=2)
    twin = trainer_of(pkg, "S1", dtype, skip_nonfinite=True, accumulate_steps=2)
    for X, y in data[:2]:
        subject.step(X, y)
        twin.step(X, y)
    keep = trainer_bits(subject)
    for i, (X, y) in enumerate(data[2:4]):
        if i == bad_at:
            X, y = (poison_x("S1", X), y) if where == "X" else (X, poison_y(y))
        subject.step(X, y)
    assert_same(trainer_bits(subject), keep, "the dropped group")
    for X, y in data[4:]:
        ls, lt = float(subject.step(X, y)), float(twin.step(X, y))
    assert_twins(subject, twin, ls, lt, 2, 1, f"accumulate {dtype} bad {where} at {bad_at}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_skill_maps_carry_a_bad_window_on_its_cells_only(pkg, dtype):
    """SkillAccumulator.update_from_pred over three windows, the middle one with a NaN at the seam: the per-cell sums that
    contain the prediction (sum p, sum p^2, sum (y-p)^2) are non-finite exactly on the crop of that window's NaN set, and have
    the bits of a run whose middle window is clean everywhere else; the sums of y alone do not notice"""
    from nasa_niswan_amd.inference import SkillAccumulator
    net = make_net(pkg, "S1", dtype)
    data = chunks("S1", 3, seed=2)
    inside = NC.nan_set("S1", NC.SEAM)["pred"][:, HALO[0]:HALO[0] + HC, HALO[1]:HALO[1] + WC]
    assert 0 < int(inside.sum()) < inside.numel()
    maps = []
    for bad in (True, False):
        acc = SkillAccumulator(NC.OUT, HC, WC)
        for i, (X, y) in enumerate(data):
            with torch.no_grad():
                pred = net(poison_x("S1", X) if bad and i == 1 else X)
            acc.update_from_pred(pred, y, HALO)
        maps.append(acc.pix[0].cpu())
    got, want = maps
    assert int(NC.nonfinite(want).sum()) == 0
    for plane, with_p in enumerate((False, True, False, True, True)):        # sum y, sum p, sum y^2, sum p^2, sum (y-p)^2
        if with_p:
            assert torch.equal(NC.nonfinite(got[plane]), inside), plane
            assert NC.same_bits(got[plane][~inside], want[plane][~inside]), plane
        else:
            assert NC.same_bits(got[plane], want[plane]), plane


# --------------------------------------------------------------------------- 5. stateful training survives a bad chunk
STATEFUL = [dict(T=NC.T), dict(T=2, bptt_segments=2)]


@pytest.mark.parametrize("kw", STATEFUL, ids=["plain", "segments"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stateful_trainer_survives_a_bad_chunk(pkg, dtype, kw):
    """B = 3, a NaN in lane 1 of the second chunk's X: the step is skipped and lane 1 starts the third chunk from the zero
    state, the other lanes from the state they carried.  The twin's second chunk has clean X and one NaN in y (skipped by the
    loss, every state finite) and its third step resets lane 1 by hand: loss, parameters, moments and the carried state after
    the third step agree bit for bit."""
    kw = dict(kw)
    T = kw.pop("T")
    (X0, y0), (X1, y1), (X2, y2) = chunks("S1", 3, B=3, T=T)
    subject = trainer_of(pkg, "S1", dtype, stateful=True, skip_nonfinite=True, **kw)
    twin = trainer_of(pkg, "S1", dtype, stateful=True, skip_nonfinite=True, **kw)
    subject.step(X0, y0)
    assert math.isnan(float(subject.step(poison_x("S1", X1, lane=1, t=T - 1), y1)))
    ls = float(subject.step(X2, y2))
    twin.step(X0, y0)
    assert math.isnan(float(twin.step(X1, poison_y(y1))))
    lt = float(twin.step(X2, y2, reset=[False, True, False]))
    assert_twins(subject, twin, ls, lt, 2, 1, f"stateful {dtype} {kw}")
    assert twin.grad_stats()["skipped"] == 1
    assert all(bool(torch.isfinite(c).all()) for c in subject.state.c)


@pytest.mark.parametrize("kw", STATEFUL, ids=["plain", "segments"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_guard_adds_nothing_to_finite_data(pkg, dtype, kw):
    """stateful + skip_nonfinite against stateful + max_grad_norm = 1e9 alone (the same guarded launch, no skip, no lane
    check) over three finite chunks: bit for bit"""
    kw = dict(kw)
    T = kw.pop("T")
    data = chunks("S1", 3, B=3, T=T, seed=1)
    a = trainer_of(pkg, "S1", dtype, stateful=True, skip_nonfinite=True, **kw)
    b = trainer_of(pkg, "S1", dtype, stateful=True, max_grad_norm=1e9, **kw)
    for X, y in data:
        la, lb = float(a.step(X, y)), float(b.step(X, y))
    assert la == lb and not math.isnan(la)
    assert_same(trainer_bits(a), trainer_bits(b), f"guard on finite data {dtype} {kw}")
    assert a.grad_stats()["applied"] == 3 and a.grad_stats()["skipped"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_the_guard_the_nan_is_carried(pkg, dtype):
    """skip_nonfinite = False: the reference's arithmetic -- the carried state keeps the NaN and the third loss is NaN"""
    (X0, y0), (X1, y1), (X2, y2) = chunks("S1", 3, B=3)
    tr = trainer_of(pkg, "S1", dtype, stateful=True)
    tr.step(X0, y0)
    tr.step(poison_x("S1", X1, lane=1, t=NC.T - 1), y1)
    lanes = [torch.isfinite(c.view(3, -1)).all(dim=1).tolist() for c in tr.state.c]
    assert lanes == [[True, False, True]] * 2, lanes
    assert math.isnan(float(tr.step(X2, y2)))
