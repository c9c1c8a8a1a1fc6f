"""Cases and the comparator of the non-finite spread tests (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite.py;
DESIGN.md 4.12).  Pure: numpy / torch on the CPU, nothing of the device.

One element of the input (or of a given state) is replaced by NaN, +inf, -inf or 1e30.  WHERE the result is non-finite is an
exact, tolerance-free statement about which pixels, taps, tiles, time steps and lanes a launch read; the CPU oracle
(oracle/convlstm_oracle.py, f32) says where the reference's arithmetic puts them:
  NaN    spreads through the receptive field (pred, dX) and into every weight gradient; every finite element keeps the
         bits of the clean run
  +-inf  saturates the gates of layer 0: pred and dX stay finite and differ from the clean run inside the NaN case's set
         only; the weight gradient of layer 0 is non-finite at the bad input channel's in-grid taps (inf * dG)
  1e30   the same as +-inf with everything finite

`compare` holds a device result against that: (a) equal non-finite sets, (b) the standing numeric gates over the finite part,
(c) the other lane bit-identical to the device's own clean run, (d) lane 0 outside the NaN case's set bit-identical too."""
import functools
import math

import numpy as np
import torch

from oracle import convlstm_oracle as O

B, T, H, W, OUT = 2, 3, 13, 37, 2        # two tile rows, two 32-column tiles, ragged in both
STACKS = {
    "S1": dict(C=5, hidden=[24, 8], ks=[5, 3]),             # folded thin input, P = 2, 8 padded hidden channels, tiny top layer
    "S2": dict(C=33, hidden=[16, 32, 16], ks=[3, 5, 3]),    # no channel padding in f32, merged grids and BPTT pairs; its input
                                                            # FOLDS (99 channels in fewer 64-byte chunks than 3 x 33: `folds`)
    "S3": dict(C=4, hidden=[8], ks=[3]),                    # the stencil / dense-K / padded-tile families
    "S4": dict(C=4, hidden=[7], ks=[3]),                    # the same families with a padding channel of their own (odd width)
    "S5": dict(C=32, hidden=[16, 32, 16], ks=[3, 5, 3]),    # S2 with an input that does NOT fold: the plain first-layer x path,
                                                            # forward and dgrad, and the exact dX set of a NaN
}


def folds(stack: str, dtype: str) -> bool:
    """the library's rule for folding layer 0's horizontal taps into the channels (nint_xfold_pays): k * C channels take fewer
    64-byte chunks than k times C's.  S1 - S4 fold in both storage types, S5 in neither (asserted in test_nonfinite_cpu.py)"""
    C, k = STACKS[stack]["C"], STACKS[stack]["ks"][0]
    kc = 32 if dtype == "bf16" else 16
    cdiv = lambda a, b: -(-a // b)
    return k > 1 and cdiv(k * C, kc) < cdiv(C, kc) * k
VALUES = {"nan": math.nan, "pinf": math.inf, "ninf": -math.inf, "big": 1e30}
PLACES = [(0, 0, 0), (1, 7, 31), (2, 12, 36)]     # (t, y, x): grid corner at the first step, the tile seam, the last pixel at the last step
SEAM = 1
LANE_KEYS = ("pred", "dX")


def bad_channel(stack: str) -> int:
    """the channel in the middle of C (S1: X[0, t, 3, y, x])"""
    return (STACKS[stack]["C"] + 1) // 2


def params_of(stack: str, seed: int = 0):
    s = STACKS[stack]
    return O.synth_params(s["C"], s["hidden"], s["ks"], len(s["hidden"]), out_channels=OUT, seed=seed)


def clean_batch(stack: str, B_: int = B, T_: int = T, seed: int = 0):
    """(X, wgt): the clean input and the weights of loss = (pred * wgt).sum()"""
    rng = np.random.default_rng(4120 + seed)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    return f(B_, T_, STACKS[stack]["C"], H, W), f(B_, OUT, H, W)


def batch(stack: str, value=None, place=None):
    """(X, wgt) with X[0, t, bad_channel, y, x] = VALUES[value] (value None: the clean batch)"""
    X, wgt = clean_batch(stack)
    if value is not None:
        t, y, x = PLACES[place]
        X[0, t, bad_channel(stack), y, x] = VALUES[value]
    return X, wgt


def oracle_pass(params, X, wgt, h0=None, c0=None, state_wgt=None):
    """f32 CPU autograd of the reference's arithmetic: {pred, dX, <parameter name>: its gradient}; with a given state also
    h_T.l, c_T.l and the gradients dh0.l, dc0.l, the loss extended by sum (h_T * Rh) + sum (c_T * Rc) over `state_wgt`"""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    x = X.clone().requires_grad_(True)
    res = {}
    if h0 is None:
        pred = O.convlstm_forward(x, leaf)
        loss = (pred * wgt).sum()
    else:
        h0 = [v.clone().requires_grad_(True) for v in h0]
        c0 = [v.clone().requires_grad_(True) for v in c0]
        pred, hs, cs = O.convlstm_forward(x, leaf, return_states=True, h0=h0, c0=c0)
        loss = (pred * wgt).sum()
        for l, (h, c) in enumerate(zip(hs, cs)):
            loss = loss + (h * state_wgt[0][l]).sum() + (c * state_wgt[1][l]).sum()
            res[f"h_T.{l}"], res[f"c_T.{l}"] = h.detach(), c.detach()
    loss.backward()
    res["pred"], res["dX"] = pred.detach(), x.grad
    for k, v in leaf.items():
        res[k] = v.grad
    if h0 is not None:
        for l in range(len(h0)):
            res[f"dh0.{l}"], res[f"dc0.{l}"] = h0[l].grad, c0[l].grad
    return res


@functools.lru_cache(maxsize=None)
def oracle_run(stack: str, value=None, place=None):
    """the oracle's result of one case, computed once and shared (read-only)"""
    X, wgt = batch(stack, value, place)
    return oracle_pass(params_of(stack), X, wgt)


def nonfinite(t: torch.Tensor) -> torch.Tensor:
    return ~torch.isfinite(t)


def nan_set(stack: str, place: int, keys=LANE_KEYS):
    """the influence region of a place: lane 0's non-finite sets of the NaN case, per key"""
    r = oracle_run(stack, "nan", place)
    return {k: nonfinite(r[k][0]) for k in keys}


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def is_forward_key(k: str) -> bool:
    return k == "pred" or k.startswith("h_T") or k.startswith("c_T")


# Gates of (b) that a measured rounding error set (twice the worst measured over the parametrisation), keyed
# (stack, dtype, key); the standing gates hold everywhere else.
#   S4 bf16, the bias gradient of the one 7-channel layer (28 numbers): rel-L2 2.005e-2 ... 2.034e-2 against the f32 oracle at
#   every place of the +inf case, the same to four digits under the stencil, dense-K and MFMA gate kernels (tile rows 1 / 2 /
#   8), with equal non-finite sets and the f32 run of the same case inside its 1e-3 gate: bf16 rounding of dG, not a wrong read
MEASURED_GATES = {("S4", "bf16", "layers.0.conv.bias"): 2 * 2.034e-2}


def measured_gates(stack, dtype):
    return {k: g for (s, d, k), g in MEASURED_GATES.items() if (s, d) == (stack, dtype)}


def _numbers(k, dev, ref, fin, dtype, gates, log, tag):
    """(b): the elements `fin` of one tensor under the standing gate of its kind"""
    if not bool(fin.any()):
        return
    a, b = dev[fin].double(), ref[fin].double()
    if dtype == "bf16":
        err, gate = float((a - b).norm() / (b.norm() + 1e-30)), 2e-2
    elif is_forward_key(k):
        err, gate = float(((a - b).abs() / (1e-5 + 1e-4 * b.abs())).max()), 1.0       # (in units of atol + rtol |ref|)
    else:
        err, gate = float((a - b).abs().max()), 1e-3 * float(b.abs().max())
    gate = (gates or {}).get(k, gate)               # (`gates`: measured_gates(stack, dtype) of the case)
    if log is not None:
        log.append((tag, k, err, gate))
    assert err <= gate, (tag, k, dtype, err, gate)


def widened(m: torch.Tensor, p: int) -> torch.Tensor:
    """m grown by p columns each way"""
    out = m.clone()
    for d in range(1, p + 1):
        out |= shift_mask(m, 0, d) | shift_mask(m, 0, -d)
    return out


def compare_within(device, oracle, clean_device, key, reach, dtype, lanes=True, log=None, tag="", gates=None):
    """The statement that holds of a tensor with a KNOWN deviation of its non-finite set, for every knob
    setting the exact comparison would have run under: the device's set covers the oracle's and lies inside `reach` (the
    oracle's set widened as the deviation's cause allows); the elements finite on both sides are within the standing gates;
    and with `lanes`, lane 1 and everything of lane 0 outside `reach` have the clean run's bits.  The exact set stays pinned
    beside it as a strict expected failure."""
    dev, ref = device[key].detach().float().cpu(), oracle[key]
    assert dev.shape == ref.shape == reach.shape, (tag, key, tuple(dev.shape), tuple(ref.shape), tuple(reach.shape))
    got, want = nonfinite(dev), nonfinite(ref)
    assert bool((reach | ~want).all()), (tag, key, "the reach does not cover the oracle's set")
    n = int((want & ~got).sum())
    assert n == 0, f"{tag} {key}: {n} elements the oracle has non-finite are finite"
    n = int((got & ~reach).sum())
    assert n == 0, f"{tag} {key}: {n} non-finite elements beyond the reach of the known deviation"
    _numbers(key, dev, ref, ~got & ~want, dtype, gates, log, tag)
    if lanes:
        d, clean = device[key].detach().cpu(), clean_device[key].detach().cpu()
        assert not bool(reach[1:].any())
        assert same_bits(d[1:], clean[1:]), f"{tag} {key}: lane 1 differs from the clean run"
        keep = ~reach[0]
        n = int((bits(d[0])[keep] != bits(clean[0])[keep]).sum())
        assert n == 0, f"{tag} {key}: {n} elements of lane 0 outside the widened region differ from the clean run"


def compare(device, oracle, clean_device, nan_set, dtype, lane_keys=LANE_KEYS, log=None, tag="", keys=None, gates=None):
    """AssertionError unless `device` ({key: tensor}, the keys of `oracle`) is the oracle's result of the case:
      (a) the non-finite sets of every tensor are elementwise equal to the oracle's (isfinite, not NaN-versus-inf)
      (b) finite elements are within the standing gates: f32 outputs rtol 1e-4 / atol 1e-5, f32
          gradients max-abs <= 1e-3 max|ref| over the finite part, bf16 rel-L2 <= 2e-2 over the finite part
      (c) lane 1 of the `lane_keys` tensors is bit-identical to `clean_device`, the device's own clean run with the same knobs
      (d) lane 0 of them is bit-identical to the clean run outside `nan_set[key]`, the NaN case's non-finite set for the place
    `log`: a list that receives (tag, key, measured error, gate) for every (b) figure, before it is asserted.
    `keys`: the tensors to hold against the oracle (default: all of the oracle's) -- a test that pins one known deviation on
    its own runs the comparison in two parts, which together cover every key."""
    assert set(oracle) <= set(device), sorted(set(oracle) - set(device))
    if keys is not None:
        assert set(keys) <= set(oracle), sorted(set(keys) - set(oracle))
        oracle = {k: v for k, v in oracle.items() if k in keys}
        lane_keys = [k for k in lane_keys if k in keys]
    for k, ref in oracle.items():
        dev = device[k].detach().float().cpu()
        assert dev.shape == ref.shape, (tag, k, tuple(dev.shape), tuple(ref.shape))
        bad_d, bad_o = nonfinite(dev), nonfinite(ref)
        if not torch.equal(bad_d, bad_o):                                                    # (a)
            extra, missing = int((bad_d & ~bad_o).sum()), int((~bad_d & bad_o).sum())
            raise AssertionError(f"{tag} {k}: non-finite set differs from the oracle's: {extra} extra, {missing} missing "
                                 f"(oracle {int(bad_o.sum())} of {ref.numel()})")
        _numbers(k, dev, ref, ~bad_o, dtype, gates, log, tag)                                # (b)
    for k in lane_keys:
        dev, clean = device[k].detach().cpu(), clean_device[k].detach().cpu()
        assert same_bits(dev[1:], clean[1:]), f"{tag} {k}: lane 1 differs from the clean run"      # (c)
        keep = ~nan_set[k]
        assert keep.shape == dev[0].shape, (tag, k, tuple(keep.shape), tuple(dev[0].shape))
        n = int((bits(dev[0])[keep] != bits(clean[0])[keep]).sum())                             # (d)
        assert n == 0, f"{tag} {k}: {n} elements of lane 0 outside the influence region differ from the clean run"


# --------------------------------------------------------------------------- faults for the comparator's self-checks
def shift_mask(m: torch.Tensor, dy: int, dx: int) -> torch.Tensor:
    """m moved by (dy, dx) over its last two axes, False shifted in"""
    out = torch.zeros_like(m)
    Hh, Ww = m.shape[-2:]
    ys, yd = (slice(0, Hh - dy), slice(dy, Hh)) if dy >= 0 else (slice(-dy, Hh), slice(0, Hh + dy))
    xs, xd = (slice(0, Ww - dx), slice(dx, Ww)) if dx >= 0 else (slice(-dx, Ww), slice(0, Ww + dx))
    out[..., yd, xd] = m[..., ys, xs]
    return out


def dilate(m: torch.Tensor) -> torch.Tensor:
    out = m.clone()
    for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        out |= shift_mask(m, dy, dx)
    return out


def erode(m: torch.Tensor) -> torch.Tensor:
    return ~dilate(~m)
