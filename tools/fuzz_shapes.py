#!/usr/bin/env python3
"""Random-shape screen of the whole sequence path against the CPU oracle (prediction, all gradients, input gradient):
layer counts 1-4, kernel sizes 1/3/5/7, ragged grids, thin and thick channel counts, B = 1-5, T = 1-4, both storage types,
the merged-grid launches forced on and off, both tile heights and the library's choice.
    python tools/fuzz_shapes.py [--n 40] [--seed 0]

The draw is separate from the run: ``draw_case(rng, it, mode, ...)`` is pure (no GPU, no library load) and returns a case
description; ``main()`` runs what it drew.  ``--list`` prints the drawn cases of any mode as JSON lines and exits without
importing the package; ``--only N`` replays the stream up to case N and runs it alone, printing every tensor's error.

Modes that start from the zero state and use the last prediction alone: plain (``net(x)``), ``--trainer``, ``--cell``,
``--dataset`` (and the ``--big`` / ``--wide`` variants of the plain one).  Their random streams are those of the first
version of this tool: one generator per run, shape draw, mode-specific values, then the data.

Modes for the carried state, segments and the trainer's options.  Each case has a generator of its own (seed, mode, case
number), so ``--only`` needs no replay; shapes come from the shared draw under caps that keep a case's CPU autograd short
(hidden from {4, 8, 16, 24, 32, 48, 64}, grid 5-30 x 9-50, out from {1, 2, 5, 20}); every mode-specific value is drawn
after the shape.
  --state       ``ConvLSTM(..., return_sequence=<drawn>)`` called as ``net(x, state, return_state=True)`` with the state None,
                (h0, c0) tensors per layer (h scaled by 0.5) or tensors for a drawn subset of lanes (the rest zero); random
                cotangents on pred, the sequence, every h_T and c_T; against ``oracle.convlstm_forward(h0=, c0=)`` under CPU
                autograd: pred, seq, h_T, c_T, dX, dh0, dc0 of every layer and every parameter gradient.  Every third case
                chains two calls on the halves of a 2T window through ``return_state="device"`` / ``state=<ConvLSTMState>``
                and compares the second call's pred, sequence and final state with the oracle on the whole window (values
                only: the device state is detached by contract).
  --train-opts  ``FusedTrainer.step`` with drawn ``bptt_segments`` n in {1..4} x S in {1, 2, 3} (T = n S), ``accumulate_steps``
                in {1, 2}, ``loss_weights`` (none, an (Hc,) vector, an (Hc, Wc) map; non-negative, some exactly zero),
                ``max_grad_norm`` (None, or 0.5 / 2 times the reference norm: a clipped and an unclipped step),
                ``sequence_loss`` (n = 1 only) and a halo: the loss of every call, and ``tr.flat.grad`` after the last call of
                a group, against CPU autograd over the WHOLE window (segments are a memory device, not a truncation; with
                two micro-batches the bucket is the sum of the two windows' gradients; with clipping the bucket stays the
                unclipped gradient and ``grad_stats()["last_norm"]`` is checked against the f64 norm of the reference bucket
                times grad_scale under the loss's relative gate).
  --stateful    two consecutive chunks through ``FusedTrainer(stateful=True, bptt_segments=n)``, n in {1, 2, 3}, the second with
                a drawn per-lane ``reset``.  Each chunk is checked from what the device held when it started: the parameters
                (``tr.flat.data``) and the carried state (``tr.state.tensors()``) are read back before chunk 2, and the oracle
                runs chunk 2 from exactly those (reset lanes zeroed, state detached) -- Adam's sign sensitivity between the
                chunks never enters a gate.  Loss, bucket and carried state after each chunk.
  --finetune    two steps of ``FusedTrainer(freeze_layers=f, weight_decay=wd, layer_lr_scale=scales)`` with f drawn from 0 .. L
                (nothing frozen ... the head alone), wd from {0, 1e-2, 0.1} and one scale per layer.  Each step is checked from
                the parameters and moments the device held before it: the loss and the trained gradients against CPU autograd
                (in bf16 the layers' weights: its biases and head sums cancel, the f32 cases gate them), the new weights against
                ``torch.optim.AdamW`` (biases in zero-decay groups) stepping on the DEVICE's gradient at rtol 2e-6 / atol 1e-7,
                and the frozen regions of the gradient bucket, the weights and both moments bit-unchanged.  The L1 kink
                (below) is not treated here: a case that lands on it shows as a gradient miss in bf16.  --self-check: the
                reference's AdamW loses its weight decay; the reference trains the frozen layers too.
  --sampled     ``ConvLSTM(feedback=True)(x[, state], free_mask=M[, feedback_grad=True])`` (scheduled sampling) with
                a drawn stack, grid, number of feedback channels, storage type, boundary, input layout, state and (B, T) feed
                mask of a drawn density.  Forward: bit for bit the open-loop pass over the input with the predictions
                substituted where the mask says, and against tests/sampled_model.py.  Where no image is fed at step 0: outputs,
                every parameter gradient and dx under drawn cotangents against the model under CPU autograd.  --self-check:
                the reference of the first case with a mixed step feeds every image from the first fed step on.
  --residual    ``ConvLSTM(feedback=True, residual=True)(x[, state], free_from=F | free_mask=M[, feedback_grad=True])`` (the residual
                head, DESIGN.md 4.22: p_t = x_t[feedback channels] + head(h_t)) with a drawn stack, grid, number of feedback
                channels, storage type, boundary, input layout, state, and either a first fed step F >= 1 (T: nothing fed) or a
                (B, T) feed mask with column 0 clear.  Forward: bit for bit the residual open-loop pass over the input with the
                predictions substituted where fed, and against tests/residual_model.py.  Then outputs, every parameter gradient
                and dx (the skip add on the unfed feedback channels, zeros on the fed ones) under drawn cotangents against the
                model under CPU autograd.  --self-check: the reference of the first case loses the base (the non-residual
                model, tests/sampled_model.py).
  --noise       ``ConvLSTM(x, input_noise=InputNoise(std, channels=(c0, n), seed, draw, step0, lane0))`` (the input noise, DESIGN.md
                4.23) with a drawn stack, grid, noise span, sigma per channel (one may be 0), storage type, boundary, input
                layout and generator key.  Outputs, every parameter gradient and dx under drawn cotangents against the CPU
                oracle under autograd on the PRE-NOISED input, built on the host by tests/noise_model.py from its own Philox;
                an all-zero std is the pass without the argument, bit for bit.  --self-check: the reference of the first
                case sees the clean input.
  --self-check  (with one of these modes) after the first passing case to which a fault applies, the REFERENCE is corrupted on
                the host and the same comparison of the same device results must fail: --state: the oracle gets a zero c0
                for the last layer; --train-opts with n >= 2: the oracle back-propagates the last segment only (truncated
                BPTT); with accumulation: one window is left out of the sum; --stateful: the oracle ignores the reset.
                Nothing is launched for it.  The run fails if a fault of its mode found no case to be tried on.

Gates (all modes): f32 max abs error / max |ref| <= 1e-3; bf16 rel-L2 <= 3e-2; the trainer's loss (and the gradient norm)
relative 2e-6 (f32) / 2e-2 (bf16).  bf16 bias gradients and the head's bf16 weight gradient are sums that cancel and are gated
on their factors (check_bias_grad, check_head_wgrad).  The stored factors are those of the workspace the step ran in: key
(B, T, H, W, True, has_init).  With two micro-batches of one resident window each (n = 1) the workspace holds, after EVERY
call, that call's window whole: the bucket is read after each call and each window's own contribution (the bucket minus
what it held before) is gated on that window's stored dG, top h and dpred, all three factors.  A segmented window (n >= 2)
keeps S steps resident and its workspace ends holding segment 0: there the reduction factor cannot be formed from one
slab, so the stored dG of segment 0 is compared with the oracle's dG of those steps (the summands, and with them the entry
gradients every later segment handed down) and the sums take the coherent bound alone; a dropped or doubled tile of the
accumulating fold is then seen by the f32 cases (tests/test_fuzz_draw_cpu.py requires them in the seeded runs).  A stateful
trainer's carried state IS the h the head read, and ``tr._dpred`` the last segment's d loss / d pred, so there the head's
factors are complete whatever n is.

The L1 term of the trainer's loss is not differentiable at pred = y.  In the trainer modes the oracle keeps its own
subgradient everywhere except at cells where its own |d| = |pred - y| is within what the standing gate lets a prediction be
off (LIM * max |pred|; in bf16 the adopted cells together within the rel-L2 gate's budget) AND the device stands on the other
side; there it takes the device's sign.  The device's d loss / d pred must be a value of (2 d + sign d) w / cnt on every
weighted cell (|dpred cnt / w| >= 1), its own prediction d + y read back from it passes the standing gate (``pred.N``), and
d loss / d pred itself is gated (``dpred.N``): device_side.  Measured: 1 cell of 356 in seed 215 --train-opts #1 takes the
weight gradient from 3.9e-2 to 4.4e-3 rel-L2 and the head's bias gradient from 1.9e-1 to 8.2e-4.  Every adopted cell is
printed (count, largest |d|, bound), with --only also when there is none.
``--force-dtype`` (with --only) replays a case in the other storage type.

``--guarded`` (every mode): the device side of each case runs inside ``oracle.guarded_alloc.patched(mode="poison")`` -- every
buffer the package allocates sits between guards of at least 64 KiB and four slab rows, ``torch.empty`` payloads hold 0xFF
(NaN), the case's inputs and the module's parameters go into arenas of their own (``_dev``, ``_net``).  The draw, the oracle
and the comparison are unchanged (``--list`` prints the same lines); every gate fails on a NaN in the device result
(tests/test_guarded_alloc_cpu.py), so a poisoned byte that reaches a result is a miss, and after each case every guard byte is
compared: a damaged guard prints the allocation's call site, the byte range and the case's replay line.  With ``--self-check``
one guard byte is flipped by a host write after the first passing case and the check has to fail."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = engine = O = stored_dG = None          # the package and the oracle: loaded by main() once it has something to run

WAVES = [None, 0, 1, 4, 2, 5, 4]            # engine.FORCE_WAVE by case number
TILE_ROWS = [0, 0, 4, 8]                    # engine.FORCE_TILE_ROWS by case number
OLD_MODES = ("plain", "trainer", "cell", "dataset")
NEW_MODES = ("state", "train_opts", "stateful", "finetune")       # (a new mode goes LAST: case_rng keys a stream by position)
# ... and the modes with a stream per case that have a draw and a run of their own, behind them (positions as above)
STREAM_MODES = NEW_MODES + ("closed_loop",)
# ... and the modes added since.  STREAM_MODES itself is pinned by the tests of the modes it lists, so a later mode continues the
# numbering here: ALL_STREAM_MODES is what case_rng indexes, and no earlier mode's position moves.
LATE_MODES = ("rollout",)
ALL_STREAM_MODES = STREAM_MODES + LATE_MODES
# ... and ALL_STREAM_MODES is pinned in turn (tests/test_rollout_cpu.py).  The modes behind it have a tuple and a stream key of their
# own (case_rng), so that no earlier mode's draws move.
SAMPLED_MODES = ("sampled",)
SAMPLED_KEY = 1000              # the stream key of SAMPLED_MODES[i] is SAMPLED_KEY + i
# ... and SAMPLED_MODES is pinned too (tests/test_sampled_cpu.py): the residual head's mode has its own tuple and key
RESIDUAL_MODES = ("residual",)
RESIDUAL_KEY = 2000             # the stream key of RESIDUAL_MODES[i] is RESIDUAL_KEY + i
# ... and RESIDUAL_MODES is pinned in turn (tests/test_residual_cpu.py): the input noise's mode continues the same way
NOISE_MODES = ("noise",)
NOISE_KEY = 3000                # the stream key of NOISE_MODES[i] is NOISE_KEY + i
# ... and NOISE_MODES is pinned as well (tests/test_gpu_fuzz_noise.py): the ensemble statistics' mode continues the same way
ENSEMBLE_MODES = ("ensemble",)
ENSEMBLE_KEY = 4000             # the stream key of ENSEMBLE_MODES[i] is ENSEMBLE_KEY + i
LIM = {"f32": 1e-3, "bf16": 3e-2}
LOSS_LIM = {"f32": 2e-6, "bf16": 2e-2}


GUARD = None        # --guarded: the oracle.guarded_alloc.GuardedTorch of the case that is running


def _dev(t):
    """a host tensor of the case on the device; --guarded: in a guarded arena of its own"""
    t = t.cuda()
    return t if GUARD is None else GUARD.guard_copy(t)


def _net(net):
    """the module on the device; --guarded: every parameter in a guarded arena"""
    net = net.cuda()
    return net if GUARD is None else GUARD.guard_module(net)


def case_row_stride(case) -> int:
    """an upper bound of the widest slab row Wh * Cp * es of a case (the guards are four of them, at least 64 KiB): the halo row
    W + 2 P, rounded up generously, times the widest channel count -- the folded input k * C, or the 4 * Ch16 gate columns --
    in f32.  Pure."""
    if case["mode"] == "dataset":
        W, ks, C, hidden = case["gw"] + 2 * case["px"], [case["k0"]], 3 * case["levels"] + 2, [16]
    else:
        W, ks, C, hidden = case["W"], case["ks"], case["C"], case["hidden"]
    return (W + 2 * max(k // 2 for k in ks) + 32) * max(max(ks) * C + 32, 4 * (max(hidden) + 16)) * 4


def replay_line(args, case) -> str:
    """the command that runs this case alone"""
    flags = "".join(f" --{m.replace('_', '-')}" for m in ("big", "wide") if getattr(args, m))
    mode = "" if args.mode == "plain" else " --" + args.mode.replace("_", "-")
    return (f"python tools/fuzz_shapes.py --seed {args.seed} --n {max(args.n, case['it'] + 1)}{mode}{flags}"
            f"{' --guarded' if args.guarded else ''} --only {case['it']}")


@contextlib.contextmanager
def guarded_case(args, case, state):
    """--guarded: the device side of the case allocates through a poisoning GuardedTorch (the package's `torch` is the proxy
    for the duration, the case's own tensors go through _dev / _net); afterwards every guard byte is compared.  A damaged
    guard prints the case's replay line.  --self-check: after the first passing case one guard byte is flipped by a
    host-issued write and verify() has to fail (`state["guard"]`)."""
    global GUARD
    if not args.guarded:
        yield
        return
    from oracle import guarded_alloc as GA
    with GA.patched(mode="poison", row_stride=case_row_stride(case)) as gt:
        GUARD = gt
        try:
            yield
            torch.cuda.synchronize()
            try:
                n = gt.verify()
            except GA.GuardError as e:
                print(f"GUARD HIT {case['tag']}\n{e}\nreplay: {replay_line(args, case)}", flush=True)
                raise SystemExit(f"guard damaged in {case['tag']}; replay: {replay_line(args, case)}")
            state["arenas"] = state.get("arenas", 0) + n
            if args.guard_self_check and not state.get("guard"):
                a = next(a for a in reversed(gt.arenas) if a.nbytes)
                pos = a.front + a.nbytes + 1
                a.arena[pos] ^= 0x01

                def must_fail():
                    try:
                        gt.verify()
                    except GA.GuardError as e:
                        raise AssertionError(str(e))
                expect_failure(case["tag"], "one flipped byte in a back guard", must_fail)
                a.arena[pos] ^= 0x01
                gt.verify()
                state["guard"] = True
        finally:
            GUARD = None
            gt.release()


def _load():
    global pkg, engine, O, stored_dG
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import nasa_niswan_amd as pkg_
    from nasa_niswan_amd import engine as engine_
    from oracle import convlstm_oracle as O_
    from oracle.stored_audit import stored_dG as stored_dG_
    pkg, engine, O, stored_dG = pkg_, engine_, O_, stored_dG_
    pkg.load_library()


# ---------------------------------------------------------------------------------------------------- sums that cancel
def check_bias_grad(tag, name, db, dbo, dG_stored, dG_oracle, dtype):
    """The bias gradient is a sum that cancels (tests/test_gpu_bias_grad.py): bf16 mode is gated on its two factors instead of
    on a loose end-to-end figure -- (1) the REDUCTION: db equals the f32 column sum of the dG slab the kernels STORED (1e-5 of
    its max: a dropped or doubled tile shows here whatever the cancellation); (2) the SUMMANDS: the stored slab against the
    oracle's dG, elementwise (rel-L2 <= 3e-2, the gate of every other gradient).  What is then left between db and the oracle's
    db is a sum of per-element errors that are partly coherent (the bf16 rounding of one weight moves a whole column the same
    way), so its only honest bound is the coherent one, (3) |err| <= 3e-2 * ||dG_col||_1 -- measured up to 10 x the
    incoherent estimate 3e-2 * ||dG_col||_2 (fuzz seed 11 #9: 128 hidden channels, 7x7, 17 x 14 grid).  Returns the plain
    rel-L2 against the oracle for the log (worst seen: 7.7e-2, a B = 1, T = 1 top layer)."""
    db, dbo, go = db.double(), dbo.double(), dG_oracle.double()
    if dG_stored is not None:
        gs = dG_stored.double()
        colsum = gs.sum(dim=(0, 2, 3))
        e1 = float((db - colsum).abs().max() / (colsum.abs().max() + 1e-30))
        assert e1 <= 1e-5, (tag, name, "bias gradient is not the column sum of the stored dG slab", e1)
        e2 = float((gs - go).norm() / (go.norm() + 1e-30))
        assert e2 <= 3e-2, (tag, name, "stored dG slab against the oracle's dG", e2)
    bound = 3e-2 * go.abs().sum(dim=(0, 2, 3)) + 1e-30
    worst = float(((db - dbo).abs() / bound).max())
    assert worst <= 1.0, (tag, name, "bias gradient outside the coherent-error bound", worst)
    return float((db - dbo).norm() / (dbo.norm() + 1e-30))


def check_head_wgrad(tag, dW, dWo, h_stored, h_oracle, dpred, dpred_oracle=None):
    """The head's weight gradient dW[o][c] = sum_{b,y,x} dpred[b][o][y][x] * h[b][c][y][x] is, with a random-sign dpred, a sum
    that cancels like the bias gradients (seed 601 #125: 7,772 pixels, |dW| ~ 0.1-0.6, error 5.5e-2 relative under EVERY launch
    schedule while the prediction is 1.3e-3 off: profiles/r04_h_head_wgrad_case.txt).  Gated on its factors, as check_bias_grad:
    (1) the REDUCTION: dW equals the f64 sum over the h slab the forward pass STORED, to 1e-5 of the L1 norm of the summands;
    (2) the SUMMANDS: the stored h against the oracle's (rel-L2 <= 3e-2); (3) what is left against the oracle's dW within the
    coherent bound 3e-2 * sum |dpred| |h|.  Returns the plain rel-L2 for the log.
    The images may be those of several steps or windows (a sequence cotangent, two micro-batches).  ``dpred_oracle``: where the
    device formed dpred itself (the trainer's loss pass), the oracle's own for (3); ``h_stored`` None (no single slab holds
    the summands: see the module docstring): (3) alone."""
    dW, dWo = dW.double().reshape(dWo.shape[0], -1), dWo.double().reshape(dWo.shape[0], -1)
    ho = h_oracle.double()
    dpo = (dpred if dpred_oracle is None else dpred_oracle).double()
    if h_stored is not None:
        hs, dp = h_stored.double(), dpred.double()
        ref = torch.einsum("bohw,bchw->oc", dp, hs)
        l1s = torch.einsum("bohw,bchw->oc", dp.abs(), hs.abs()) + 1e-30
        e1 = float(((dW - ref).abs() / l1s).max())
        assert e1 <= 1e-5, (tag, "head weight gradient is not the sum over the stored h slab", e1)
        e2 = float((hs - ho).norm() / (ho.norm() + 1e-30))
        assert e2 <= 3e-2, (tag, "stored h of the top layer against the oracle's", e2)
    bound = 3e-2 * torch.einsum("bohw,bchw->oc", dpo.abs(), ho.abs()) + 1e-30
    worst = float(((dW - dWo).abs() / bound).max())
    assert worst <= 1.0, (tag, "head weight gradient outside the coherent-error bound", worst)
    return float((dW - dWo).norm() / (dWo.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------------- the draw (pure)
def case_rng(seed: int, mode: str, it: int):
    """the generator of one case of a state / options mode: its own stream, so a case replays without the ones before it"""
    if mode in SAMPLED_MODES:
        return np.random.default_rng([int(seed), SAMPLED_KEY + SAMPLED_MODES.index(mode), int(it)])
    if mode in RESIDUAL_MODES:
        return np.random.default_rng([int(seed), RESIDUAL_KEY + RESIDUAL_MODES.index(mode), int(it)])
    if mode in NOISE_MODES:
        return np.random.default_rng([int(seed), NOISE_KEY + NOISE_MODES.index(mode), int(it)])
    if mode in ENSEMBLE_MODES:
        return np.random.default_rng([int(seed), ENSEMBLE_KEY + ENSEMBLE_MODES.index(mode), int(it)])
    return np.random.default_rng([int(seed), 1 + ALL_STREAM_MODES.index(mode), int(it)])


def _halo(rng, H, W):
    # (cropped grid >= 2 x 2)
    return int(rng.integers(0, min(4, (H - 2) // 2 + 1))), int(rng.integers(0, min(4, (W - 2) // 2 + 1)))


def draw_case(rng, it: int, mode: str = "plain", big: bool = False, wide: bool = False) -> dict:
    """One case from ``rng``: the shared shape draw, the knobs that rotate with the case number ``it``, then the values of
    ``mode``.  Pure: numpy only.  ``case["draws"]`` lists (name, shape) of the standard-normal tensors the run then draws from
    the same generator, in order (``draw_data``); a replay that skips the case draws and drops them."""
    if mode == "closed_loop":
        return draw_closed_loop(rng, it)
    if mode == "rollout":
        return draw_rollout(rng, it)
    if mode == "sampled":
        return draw_sampled(rng, it)
    if mode == "residual":
        return draw_residual(rng, it)
    if mode == "noise":
        return draw_noise(rng, it)
    if mode == "ensemble":
        return draw_ensemble(rng, it)
    new = mode in NEW_MODES
    L = int(rng.integers(1, 5))
    hidden = [int(rng.choice([4, 8, 16, 24, 32, 48, 64] if new else [4, 8, 16, 24, 32, 48, 64, 64, 128])) for _ in range(L)]
    ks = [int(rng.choice([1, 3, 3, 5, 5, 7])) for _ in range(L)]
    C = int(rng.choice([1, 3, 5, 7, 16, 33, 62, 100, 126]))
    out = int(rng.choice([1, 2, 5, 20] if new else [1, 2, 5, 20, 20, 200]))
    B, T = int(rng.integers(1, 6)), int(rng.integers(1, 5))
    H, W = (int(rng.integers(5, 31)), int(rng.integers(9, 51))) if new else (int(rng.integers(5, 40)), int(rng.integers(9, 70)))
    if big:
        H, W, B, T = int(rng.integers(60, 111)), int(rng.integers(100, 171)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
    dtype = "f32" if it % 2 == 0 else "bf16"
    wave, rows, widef = WAVES[it % 7], TILE_ROWS[it % 4], 0
    if wide:
        widef = [2, 2, 1][it % 3]
        dtype = "bf16"
        hidden = [int(rng.choice([32, 64, 64, 128])) if rng.random() < 0.8 else h_ for h_ in hidden]
        ks = [int(rng.choice([3, 3, 5, 7])) if k_ == 1 else k_ for k_ in ks]
        C = int(rng.choice([32, 62, 64, 126, 128])) if rng.random() < 0.7 else C
    case = dict(it=it, mode=mode, L=L, hidden=hidden, ks=ks, C=C, out=out, B=B, T=T, H=H, W=W, dtype=dtype, wave=wave, rows=rows,
                wide=widef)
    shape_tag = f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} wide={widef}"
    case["tag"] = shape_tag
    if mode == "plain":
        case["draws"] = [("X", (B, T, C, H, W)), ("wgt", (B, out, H, W))]
    elif mode == "dataset":
        levels = int(rng.integers(1, 5))
        gh, gw = int(rng.integers(4, 24)), int(rng.integers(6, 48))
        # (px >= 1: with NO longitude halo the reference's `data[..., -0:]` slice returns the whole row and the output is
        # 2W wide -- dataset.py:67-80; `padding=None` is its way of not padding.  That accident is not reproduced.)
        py, px = int(rng.integers(0, min(6, gh - 1))), int(rng.integers(1, min(6, gw)))
        pad_mode = ["reference", "reflect"][it % 2]
        seq = int(rng.integers(1, 5))
        # the windows of the "train" period of a record of 12 + seq steps (dataset.reference_split: the first 70 %, and no
        # window past the record's end); main() asserts it is what the dataset says
        nwin = min(int(round(0.7 * (12 + seq))), 13)
        nidx = int(rng.integers(1, 4))
        idx = [int(v) for v in rng.integers(0, nwin, size=nidx)]
        k0 = int(rng.choice([3, 5]))
        case.update(levels=levels, gh=gh, gw=gw, py=py, px=px, pad_mode=pad_mode, seq=seq, nwin=nwin, idx=idx, k0=k0, draws=[],
                    tag=f"#{it} dataset levels={levels} grid={gh}x{gw} pad=({py},{px}) {pad_mode} T={seq} {dtype}")
    elif mode == "cell":
        Ch, k = hidden[0], ks[0]
        has_bias = bool(it % 5)
        draws = [("Wt", (4 * Ch, C + Ch, k, k))] + ([("bt", (4 * Ch,))] if has_bias else [])
        draws += [("x", (B, C, H, W)), ("h", (B, Ch, H, W)), ("c", (B, Ch, H, W)), ("gh", (B, Ch, H, W)), ("gc", (B, Ch, H, W))]
        case.update(has_bias=has_bias, draws=draws,
                    tag=f"#{it} cell Cx={C} Ch={Ch} k={k} B={B} {H}x{W} {dtype} bias={has_bias} rows={rows}")
    elif mode == "trainer":
        hy, hx = _halo(rng, H, W)
        out, B = max(out, 2), max(B, 2)          # (keeps the reference's .squeeze() a no-op; the tag keeps the drawn values)
        case.update(out=out, B=B, halo=[hy, hx], draws=[("X", (B, T, C, H, W)), ("y", (B, out, H - 2 * hy, W - 2 * hx))])
    elif mode == "state":
        rs = bool(rng.integers(0, 2))
        form = ["none", "full", "lanes"][int(rng.integers(0, 3))]
        lanes = [bool(v) for v in rng.integers(0, 2, size=B)]
        if form == "lanes" and not any(lanes):
            lanes[int(rng.integers(0, B))] = True
        chain = it % 3 == 2
        Tx = 2 * T if chain else T
        draws = [("X", (B, Tx, C, H, W)), ("R", (B, out, H, W)), ("RS", (B, T * out, H, W))]
        for l, ch in enumerate(hidden):
            draws += [(f"{n}.{l}", (B, ch, H, W)) for n in ("h0", "c0", "Rh", "Rc")]
        case.update(return_sequence=rs, form=form, lanes=lanes if form == "lanes" else None, chain=chain, draws=draws,
                    tag=shape_tag + f" state={form}{'' if form != 'lanes' else [int(v) for v in lanes]} seq={int(rs)}"
                    + (" chain" if chain else ""))
    elif mode == "train_opts":
        n, S = int(rng.choice([1, 2, 3, 4])), int(rng.choice([1, 2, 3]))
        acc = int(rng.choice([1, 2]))
        wform = ["none", "row", "map"][int(rng.integers(0, 3))]
        clip = [None, None, 0.5, 2.0][int(rng.integers(0, 4))]      # max_grad_norm as a multiple of the reference norm
        sq = bool(rng.integers(0, 2)) and n == 1                    # (the trainer refuses sequence_loss with segments)
        hy, hx = _halo(rng, H, W)
        out, B, T = max(out, 2), max(B, 2), n * S
        Hc, Wc = H - 2 * hy, W - 2 * hx
        draws = []
        for j in range(acc):
            draws += [(f"X.{j}", (B, T, C, H, W)), (f"y.{j}", (B, T, out, Hc, Wc) if sq else (B, out, Hc, Wc))]
        if wform != "none":
            draws += [("w", (Hc,) if wform == "row" else (Hc, Wc)), ("wzero", (Hc,) if wform == "row" else (Hc, Wc))]
        case.update(out=out, B=B, T=T, n=n, S=S, acc=acc, wform=wform, clip=clip, sequence_loss=sq, halo=[hy, hx], draws=draws,
                    tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                        f"halo=({hy},{hx}) n={n} S={S} acc={acc} w={wform} clip={clip} seqloss={int(sq)}")
    elif mode == "stateful":
        n, S = int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 3]))
        out, B, T = max(out, 2), max(B, 2), n * S
        kind = ["none", "partial", "full"][int(rng.integers(0, 3))]
        mask = [bool(v) for v in rng.integers(0, 2, size=B)]
        if kind == "partial":                                       # at least one lane reset and one kept
            a = int(rng.integers(0, B))
            mask[a], mask[(a + 1 + int(rng.integers(0, B - 1))) % B] = True, False
        reset = {"none": None, "partial": mask, "full": True if it % 2 == 0 else [True] * B}[kind]
        hy, hx = _halo(rng, H, W)
        Hc, Wc = H - 2 * hy, W - 2 * hx
        draws = [(f"{v}.{j}", sh) for j in range(2) for v, sh in (("X", (B, T, C, H, W)), ("y", (B, out, Hc, Wc)))]
        case.update(out=out, B=B, T=T, n=n, S=S, reset_kind=kind, reset=reset, halo=[hy, hx], draws=draws,
                    tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                        f"halo=({hy},{hx}) n={n} S={S} reset={kind if reset is None or reset is True else [int(v) for v in reset]}")
    elif mode == "finetune":
        f = int(rng.integers(0, L + 1))                             # frozen layers: none ... all (the head alone)
        wd = [0.0, 1e-2, 0.1][int(rng.integers(0, 3))]
        scales = [float(rng.choice([0.1, 0.25, 0.5, 1.0])) for _ in range(L)]
        hy, hx = _halo(rng, H, W)
        out, B = max(out, 2), max(B, 2)
        Hc, Wc = H - 2 * hy, W - 2 * hx
        draws = [(f"{v}.{j}", sh) for j in range(2) for v, sh in (("X", (B, T, C, H, W)), ("y", (B, out, Hc, Wc)))]
        case.update(out=out, B=B, f=f, wd=wd, scales=scales, halo=[hy, hx], draws=draws,
                    tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                        f"halo=({hy},{hx}) f={f} wd={wd} scales={scales}")
    else:
        raise ValueError(mode)
    return case


def draw_closed_loop(rng, it: int) -> dict:
    """--closed-loop: a stack, a grid, O feedback channels (the last O of C), the first fed step (T: nothing is fed), a tensor
    state or none (step 0 can only be fed from one), both storage types, cyclic longitude or zero padding, the thin-input fold
    allowed or off.  Pure."""
    L = int(rng.integers(1, 4))
    hidden = [int(rng.choice([4, 8, 16, 24, 32, 64])) for _ in range(L)]
    ks = [int(rng.choice([1, 3, 3, 5, 5])) for _ in range(L)]
    C = int(rng.choice([1, 3, 4, 6, 16, 33, 40, 62]))
    out = min(C, int(rng.choice([1, 1, 2, 3, 20])))
    B, T = int(rng.integers(1, 4)), int(rng.integers(2, 6))
    H, W = int(rng.integers(5, 21)), int(rng.integers(9, 41))
    dtype = "f32" if it % 2 == 0 else "bf16"
    wave, rows = WAVES[it % 7], TILE_ROWS[it % 4]
    cyclic, fold, with_state = (bool(rng.integers(0, 2)) for _ in range(3))
    fb_from = int(rng.integers(0 if with_state else 1, T + 1))
    draws = [("X", (B, T, C, H, W))]
    if with_state:
        for l, ch in enumerate(hidden):
            draws += [(f"{n}.{l}", (B, ch, H, W)) for n in ("h0", "c0")]
    return dict(it=it, mode="closed_loop", L=L, hidden=hidden, ks=ks, C=C, out=out, B=B, T=T, H=H, W=W, dtype=dtype, wave=wave,
                rows=rows, wide=0, cyclic=cyclic, fold=fold, with_state=with_state, fb_from=fb_from, draws=draws,
                tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                    f"closed loop from {fb_from} cyclic={int(cyclic)} fold={int(fold)} state={int(with_state)}")


def draw_rollout(rng, it: int) -> dict:
    """--rollout: a stack, a grid, O feedback channels, the first fed step F >= 1 (1, the middle, T-1, or T: nothing is fed), both
    storage types, cyclic longitude or zero padding, the thin-input fold allowed or off, and cotangents on the per-step outputs,
    on the last one, or on both.  Pure."""
    L = int(rng.integers(1, 4))
    hidden = [int(rng.choice([4, 8, 16, 24, 32, 64])) for _ in range(L)]
    ks = [int(rng.choice([1, 3, 3, 5, 5])) for _ in range(L)]
    C = int(rng.choice([1, 3, 4, 6, 16, 33, 40, 62]))
    out = min(C, int(rng.choice([1, 1, 2, 3, 20])))
    B, T = int(rng.integers(1, 4)), int(rng.integers(3, 7))
    H, W = int(rng.integers(5, 21)), int(rng.integers(9, 41))
    dtype = "f32" if it % 2 == 0 else "bf16"
    wave, rows = WAVES[it % 7], TILE_ROWS[it % 4]
    cyclic, fold = (bool(rng.integers(0, 2)) for _ in range(2))
    fb_from = [1, T // 2, T - 1, T][int(rng.integers(0, 4))]
    cot = ["seq", "last", "both"][int(rng.integers(0, 3))]
    draws = [("X", (B, T, C, H, W)), ("dseq", (B, T * out, H, W)), ("dpred", (B, out, H, W))]
    return dict(it=it, mode="rollout", L=L, hidden=hidden, ks=ks, C=C, out=out, B=B, T=T, H=H, W=W, dtype=dtype, wave=wave,
                rows=rows, wide=0, cyclic=cyclic, fold=fold, fb_from=fb_from, cot=cot, draws=draws,
                tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                    f"roll-out from {fb_from} cyclic={int(cyclic)} fold={int(fold)} cotangents={cot}")


def draw_sampled(rng, it: int) -> dict:
    """--sampled: a stack, a grid, O feedback channels, both storage types, cyclic longitude or zero padding, the thin-input fold
    allowed or off, a tensor state or none, a (B, T) feed mask of a drawn density (column 0 only with a state: then the case is
    checked forward only) and cotangents on the per-step outputs or on the last one.  Pure."""
    L = int(rng.integers(1, 4))
    hidden = [int(rng.choice([4, 8, 16, 24, 32, 64])) for _ in range(L)]
    ks = [int(rng.choice([1, 3, 3, 5, 5])) for _ in range(L)]
    C = int(rng.choice([1, 3, 4, 6, 16, 33, 40, 62]))
    out = min(C, int(rng.choice([1, 1, 2, 3, 20])))
    B, T = int(rng.integers(1, 5)), int(rng.integers(3, 7))
    H, W = int(rng.integers(5, 21)), int(rng.integers(9, 41))
    dtype = "f32" if it % 2 == 0 else "bf16"
    wave, rows = WAVES[it % 7], TILE_ROWS[it % 4]
    cyclic, fold, with_state = (bool(rng.integers(0, 2)) for _ in range(3))
    density = float(rng.choice([0.0, 0.25, 0.5, 0.5, 0.5, 0.75, 0.75, 1.0]))
    mask = (rng.random((B, T)) < density).astype(int)
    if not with_state:
        mask[:, 0] = 0
    cot = ["seq", "last"][int(rng.integers(0, 2))]
    draws = [("X", (B, T, C, H, W)), ("dseq", (B, T * out, H, W)), ("dpred", (B, out, H, W))]
    if with_state:
        for l, ch in enumerate(hidden):
            draws += [(f"{n}.{l}", (B, ch, H, W)) for n in ("h0", "c0")]
    rows_ = "/".join("".join(str(int(v)) for v in r) for r in mask)
    return dict(it=it, mode="sampled", L=L, hidden=hidden, ks=ks, C=C, out=out, B=B, T=T, H=H, W=W, dtype=dtype, wave=wave,
                rows=rows, wide=0, cyclic=cyclic, fold=fold, with_state=with_state, density=density, mask=mask.tolist(), cot=cot,
                draws=draws,
                tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                    f"sampled mask={rows_} cyclic={int(cyclic)} fold={int(fold)} state={int(with_state)} cotangents={cot}")


def draw_residual(rng, it: int) -> dict:
    """--residual: a stack, a grid, O feedback channels, both storage types, cyclic longitude or zero padding, the thin-input fold
    allowed or off, a tensor state or none, and what is fed -- a first fed step F in {1, the middle, T-1, T: nothing} or a (B, T)
    feed mask of a drawn density with column 0 clear (a residual head is never fed at step 0) -- and cotangents on the per-step
    outputs, on the last one, or on both.  Pure."""
    L = int(rng.integers(1, 4))
    hidden = [int(rng.choice([4, 8, 16, 24, 32, 64])) for _ in range(L)]
    ks = [int(rng.choice([1, 3, 3, 5, 5])) for _ in range(L)]
    C = int(rng.choice([1, 3, 4, 6, 16, 33, 40, 62]))
    out = min(C, int(rng.choice([1, 1, 2, 3, 20])))
    B, T = int(rng.integers(1, 5)), int(rng.integers(3, 7))
    H, W = int(rng.integers(5, 21)), int(rng.integers(9, 41))
    dtype = "f32" if it % 2 == 0 else "bf16"
    wave, rows = WAVES[it % 7], TILE_ROWS[it % 4]
    cyclic, fold, with_state, masked = (bool(rng.integers(0, 2)) for _ in range(4))
    fb_from = [1, max(T // 2, 1), T - 1, T][int(rng.integers(0, 4))]
    density = float(rng.choice([0.25, 0.5, 0.5, 0.75, 1.0]))
    mask = (rng.random((B, T)) < density).astype(int)
    mask[:, 0] = 0
    cot = ["seq", "last", "both"][int(rng.integers(0, 3))]
    draws = [("X", (B, T, C, H, W)), ("dseq", (B, T * out, H, W)), ("dpred", (B, out, H, W))]
    if with_state:
        for l, ch in enumerate(hidden):
            draws += [(f"{n}.{l}", (B, ch, H, W)) for n in ("h0", "c0")]
    what = "mask=" + "/".join("".join(str(int(v)) for v in r) for r in mask) if masked else f"from {fb_from}"
    return dict(it=it, mode="residual", L=L, hidden=hidden, ks=ks, C=C, out=out, B=B, T=T, H=H, W=W, dtype=dtype, wave=wave,
                rows=rows, wide=0, cyclic=cyclic, fold=fold, with_state=with_state, fb_from=fb_from,
                mask=mask.tolist() if masked else None, cot=cot, draws=draws,
                tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                    f"residual {what} cyclic={int(cyclic)} fold={int(fold)} state={int(with_state)} cotangents={cot}")


def draw_noise(rng, it: int) -> dict:
    """--noise: a stack, a grid, a noise span [c0, c0 + n) anywhere in the input's channels with a sigma per channel (one of them
    may be 0), both storage types, cyclic longitude or zero padding, the thin-input fold allowed or off, the generator's key
    (seed, draw, step0, lane0 -- step0 near 2^32 now and then), and cotangents on the per-step outputs and the last one.  Pure."""
    L = int(rng.integers(1, 4))
    hidden = [int(rng.choice([4, 8, 16, 24, 32, 64])) for _ in range(L)]
    ks = [int(rng.choice([1, 3, 3, 5, 5])) for _ in range(L)]
    C = int(rng.choice([1, 3, 4, 6, 16, 33, 40, 62]))
    out = min(C, int(rng.choice([1, 2, 3])))            # (the CPU model of the stack is the closed-loop one: O <= C)
    n = int(rng.integers(1, C + 1))
    c0 = int(rng.integers(0, C - n + 1))
    B, T = int(rng.integers(1, 5)), int(rng.integers(2, 6))
    H, W = int(rng.integers(5, 21)), int(rng.integers(9, 41))
    dtype = "f32" if it % 2 == 0 else "bf16"
    wave, rows = WAVES[it % 7], TILE_ROWS[it % 4]
    cyclic, fold = (bool(rng.integers(0, 2)) for _ in range(2))
    sigma = [float(v) for v in rng.choice([0.03125, 0.0625, 0.125, 0.25], size=n)]
    if n > 1 and bool(rng.integers(0, 2)):
        sigma[int(rng.integers(0, n))] = 0.0
    key = dict(seed=int(rng.integers(0, 1 << 32)), draw=int(rng.integers(0, 1 << 16)),
               step0=[0, 3, (1 << 32) - 1][int(rng.integers(0, 3))], lane0=int(rng.integers(0, 64)))
    draws = [("X", (B, T, C, H, W)), ("dseq", (B, T * out, H, W)), ("dpred", (B, out, H, W))]
    return dict(it=it, mode="noise", L=L, hidden=hidden, ks=ks, C=C, out=out, B=B, T=T, H=H, W=W, dtype=dtype, wave=wave,
                rows=rows, wide=0, cyclic=cyclic, fold=fold, c0=c0, n=n, sigma=sigma, key=key, draws=draws,
                tag=f"#{it} C={C} hidden={hidden} k={ks} out={out} B={B} T={T} {H}x{W} {dtype} wave={wave} rows={rows} "
                    f"noise span=[{c0},{c0 + n}) zero-sigma={int(0.0 in sigma)} step0={key['step0']} cyclic={int(cyclic)} fold={int(fold)}")


def draw_ensemble(rng, it: int) -> dict:
    """--ensemble: nint_ens_accum alone -- members M, samples N (now and then beyond one launch's 64), outputs, a grid and a crop
    window in it, slots with -1 among them and one slot that no sample names, and where the members lie: contiguous, or a
    roll-out's (lanes, T, O, H, W) buffer read in place, the samples in shuffled order and one of them twice.  Pure."""
    M = int(rng.choice([2, 3, 4, 5, 8, 16, 33, 64]))
    N = int(rng.choice([1, 2, 3, 5, 8, 70])) if M <= 8 else int(rng.integers(1, 5))
    O = int(rng.choice([1, 2, 4, 5, 9]))
    H, W = int(rng.integers(3, 25)), int(rng.integers(3, 45))
    Hc, Wc = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
    oy, ox = int(rng.integers(0, H - Hc + 1)), int(rng.integers(0, W - Wc + 1))
    used = int(rng.integers(1, 4))
    slots = [int(v) for v in rng.integers(-1, used, size=N)]
    layout = "contiguous" if it % 2 == 0 else "rollout"
    T, spinup = int(rng.integers(2, 5)), 1
    order = [int(v) for v in rng.permutation(N)]
    if layout == "rollout" and N > 1:
        order[-1] = order[0]                                      # one sample twice: overlapping reads
    return dict(it=it, mode="ensemble", M=M, N=N, O=O, H=H, W=W, oy=oy, ox=ox, Hc=Hc, Wc=Wc, slots=slots, nslots=used + 1,
                layout=layout, T=T, spinup=spinup, order=order, row_w=bool(rng.integers(0, 2)), integer=bool(it % 3 == 0),
                draws=[], tag=f"#{it} ensemble M={M} N={N} O={O} {H}x{W} crop {Hc}x{Wc}@({oy},{ox}) slots={used}+1 {layout} "
                               f"{'integer' if it % 3 == 0 else 'normal'} data")


def draw_data(rng, case) -> dict:
    """the standard-normal tensors of a case, f32, from the generator that drew it"""
    return {name: torch.from_numpy(rng.standard_normal(sh).astype(np.float32)) for name, sh in case["draws"]}


def draw_cases(seed: int, n: int, mode: str = "plain", big: bool = False, wide: bool = False):
    """the cases a run with these arguments executes, in order (pure; the data is drawn and dropped where a stream is shared)"""
    cases = []
    rng = np.random.default_rng(seed)
    for it in range(n):
        if mode in ALL_STREAM_MODES + SAMPLED_MODES + RESIDUAL_MODES + NOISE_MODES + ENSEMBLE_MODES:
            cases.append(draw_case(case_rng(seed, mode, it), it, mode))
        else:
            cases.append(draw_case(rng, it, mode, big, wide))
            for _, sh in cases[-1]["draws"]:
                rng.standard_normal(sh)
    return cases


# ---------------------------------------------------------------------------------------------------- comparison
def _err(dtype, a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)) if dtype == "f32" else float((a - b).norm() / (b.norm() + 1e-30))


def compare(tag, dtype, res, ref, verbose=False):
    """Every entry of ``ref`` against ``res`` under the standing gates; returns the worst gated figure.  Names: ``loss*`` /
    ``norm`` are scalars under the loss's relative gate; ``grad.layers.N.conv.bias`` and ``grad.conv.weight`` in bf16 go to
    check_bias_grad / check_head_wgrad with the factors under the ``_`` keys (``_dG`` [per layer, or None], ``_dG0`` [segment
    0's stored slab and ``ref["_dG0"]`` the oracle's dG of those steps], ``_h``, ``_dpred``; ``_win``: per micro-batch its own
    contribution to the bucket under ``grad`` with its own ``_dG``, ``_h``, ``_dpred``, each gated on all three factors).  ``verbose`` (--only): every
    figure is printed and the first miss is raised after the last one."""
    w, misses = 0.0, []

    def gate(ok, *info):
        if not ok:
            if not verbose:
                raise AssertionError(info)
            print(f"     MISS {info[1:]}", flush=True)
            misses.append(info)

    for k, b in ref.items():
        if k.startswith("_"):
            continue
        a = res[k]
        if k.startswith("loss") or k == "norm":
            e = abs(a - b) / abs(b)
            if verbose:
                print(f"     {k}: {a:.8g} oracle {b:.8g}  rel {e:.3e}", flush=True)
            gate(e <= LOSS_LIM[dtype], tag, k, a, b, e)
            w = max(w, e)
            continue
        a, b = a.double(), b.double()
        gate(a.shape == b.shape, tag, k, tuple(a.shape), tuple(b.shape))
        gate(bool(torch.isfinite(a).all()), tag, k, "not finite")
        try:
            if dtype == "bf16" and k.startswith("grad.layers.") and k.endswith("bias"):
                l = int(k.split(".")[2])
                if res.get("_dG0") is not None:
                    e2 = _err(dtype, res["_dG0"][l], ref["_dG0"][l])
                    if verbose:
                        print(f"     stored dG of segment 0, layer {l}: rel-L2 {e2:.3e}", flush=True)
                    gate(e2 <= 3e-2, tag, k, "stored dG of segment 0 against the oracle's dG of those steps", e2)
                for j, (wd, wo) in enumerate(zip(res.get("_win") or [], ref.get("_win") or [])):
                    ej = check_bias_grad(f"{tag} window {j}", k, wd["grad"][k], wo["grad"][k], wd["_dG"][l], wo["_dG"][l], dtype)
                    if verbose:
                        print(f"     {k}, window {j}'s own: rel-L2 {ej:.3e} (all three factors)", flush=True)
                stored = res["_dG"][l] if res.get("_dG") is not None else None
                e = check_bias_grad(tag, k, a, b, stored, ref["_dG"][l], dtype)
                if verbose:
                    print(f"     {k}: rel-L2 {e:.3e} (gated on its factors)", flush=True)
                continue
            if dtype == "bf16" and k == "grad.conv.weight":
                for j, (wd, wo) in enumerate(zip(res.get("_win") or [], ref.get("_win") or [])):
                    ej = check_head_wgrad(f"{tag} window {j}", wd["grad"][k], wo["grad"][k], wd["_h"], wo["_h"], wd["_dpred"], wo["_dpred"])
                    if verbose:
                        print(f"     {k}, window {j}'s own: rel-L2 {ej:.3e} (all three factors)", flush=True)
                e = check_head_wgrad(tag, a, b, res.get("_h"), ref["_h"], res["_dpred"] if res.get("_h") is not None else ref["_dpred"],
                                     ref["_dpred"])
                if verbose:
                    print(f"     {k}: rel-L2 {e:.3e} (gated on its factors)", flush=True)
                continue
        except AssertionError as err:
            gate(False, *err.args[0])
            continue
        e = _err(dtype, a, b)
        if verbose:
            print(f"     {k}: {'max-rel' if dtype == 'f32' else 'rel-L2'} {e:.3e}  |ref| {float(b.norm()):.3e}", flush=True)
        gate(e <= LIM[dtype], tag, k, e)
        w = max(w, e)
    if misses:
        raise AssertionError(misses[0])
    return w


def _named_grads(net, flat):
    return {"grad." + k: flat.grad_view(i).detach().clone().cpu() for i, (k, _) in enumerate(net.named_parameters())}


def _top_h_images(eng, ws, slots):
    L = len(eng.cfgs)
    return torch.cat([eng.h_last(ws, L - 1, slot=s).cpu() for s in slots])


# ---------------------------------------------------------------------------------------------------- --state
def state_inputs(case, d):
    """(h0, c0) per layer as the call receives them (None for the zero state): h scaled by 0.5, unlisted lanes zero"""
    if case["form"] == "none":
        return None, None
    keep = torch.ones(case["B"]) if case["form"] == "full" else torch.tensor([1.0 if v else 0.0 for v in case["lanes"]])
    keep = keep.view(-1, 1, 1, 1)
    L = case["L"]
    return [0.5 * d[f"h0.{l}"] * keep for l in range(L)], [d[f"c0.{l}"] * keep for l in range(L)]


def state_oracle(case, d, params, corrupt=False):
    """``corrupt`` (--self-check): the last layer's c0 is zero"""
    L, T, out = case["L"], case["T"], case["out"]
    h0, c0 = state_inputs(case, d)
    if corrupt:
        assert c0 is not None
        c0 = c0[:-1] + [torch.zeros_like(c0[-1])]
    ref = {}
    if case["chain"]:
        with torch.no_grad():
            pred, seq, hs, cs = O.convlstm_forward(d["X"], params, return_states=True, return_sequence=True, h0=h0, c0=c0)
        ref["pred"] = pred
        if case["return_sequence"]:
            ref["seq"] = seq[:, T * out:]
        for l in range(L):
            ref[f"h_T.{l}"], ref[f"c_T.{l}"] = hs[l], cs[l]
        return ref
    leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    Xo = d["X"].clone().requires_grad_(True)
    if h0 is not None:
        h0, c0 = [t.clone().requires_grad_(True) for t in h0], [t.clone().requires_grad_(True) for t in c0]
    pre, toph = {}, []
    pred, seq, hs, cs = O.convlstm_forward(Xo, leaf, return_states=True, return_sequence=True, h0=h0, c0=c0, preact=pre, top_h=toph)
    loss = (pred * d["R"]).sum()
    if case["return_sequence"]:
        loss = loss + (seq * d["RS"]).sum()
    for l in range(L):
        loss = loss + (hs[l] * d[f"Rh.{l}"]).sum() + (cs[l] * d[f"Rc.{l}"]).sum()
    loss.backward()
    ref["pred"] = pred.detach()
    if case["return_sequence"]:
        ref["seq"] = seq.detach()
    for l in range(L):
        ref[f"h_T.{l}"], ref[f"c_T.{l}"] = hs[l].detach(), cs[l].detach()
    ref["dX"] = Xo.grad
    if h0 is not None:
        for l in range(L):
            ref[f"dh0.{l}"], ref[f"dc0.{l}"] = h0[l].grad, c0[l].grad
    for k, v in leaf.items():
        ref["grad." + k] = v.grad
    ref["_dG"] = [torch.cat([pre[(l, t)].grad for t in range(T)]) for l in range(L)]
    ref["_h"] = torch.cat([h.detach() for h in toph]) if case["return_sequence"] else toph[-1].detach()
    ref["_dpred"] = _head_cotangents(case, d)
    return ref


def _head_cotangents(case, d):
    """what multiplies the top layer's h in the head's weight gradient: with a sequence the T blocks of RS in step order,
    pred's cotangent R joining the last"""
    if not case["return_sequence"]:
        return d["R"]
    T, out = case["T"], case["out"]
    blocks = [d["RS"][:, t * out:(t + 1) * out] for t in range(T)]
    blocks[-1] = blocks[-1] + d["R"]
    return torch.cat(blocks)


def state_device(case, d, params):
    L, T, B, H, W = case["L"], case["T"], case["B"], case["H"], case["W"]
    net = pkg.ConvLSTM(case["C"], case["hidden"], case["ks"], L, out_channels=case["out"], return_sequence=case["return_sequence"],
                       compute_dtype=case["dtype"])
    net = _net(net)
    net.load_state_dict(params)
    h0, c0 = state_inputs(case, d)
    rs, res = case["return_sequence"], {}
    if case["chain"]:
        st = None if h0 is None else [(_dev(h), _dev(c)) for h, c in zip(h0, c0)]
        with torch.no_grad():
            dev = net(_dev(d["X"][:, :T]), st, return_state="device")[-1]
            assert isinstance(dev, pkg.ConvLSTMState)
            o2 = net(_dev(d["X"][:, T:]), dev, return_state=True)
        torch.cuda.synchronize()
        res["pred"] = o2[0].cpu()
        if rs:
            res["seq"] = o2[1].cpu()
        for l, (h, c) in enumerate(o2[-1]):
            res[f"h_T.{l}"], res[f"c_T.{l}"] = h.cpu(), c.cpu()
        return res
    Xd = _dev(d["X"]).requires_grad_(True)
    st = None
    if h0 is not None:
        hd, cd = [_dev(t).requires_grad_(True) for t in h0], [_dev(t).requires_grad_(True) for t in c0]
        st = list(zip(hd, cd))
    o = net(Xd, st, return_state=True)
    pred, states = o[0], o[-1]
    loss = (pred * _dev(d["R"])).sum()
    if rs:
        loss = loss + (o[1] * _dev(d["RS"])).sum()
    for l, (h, c) in enumerate(states):
        loss = loss + (h * _dev(d[f"Rh.{l}"])).sum() + (c * _dev(d[f"Rc.{l}"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    res["pred"] = pred.detach().cpu()
    if rs:
        res["seq"] = o[1].detach().cpu()
    for l, (h, c) in enumerate(states):
        res[f"h_T.{l}"], res[f"c_T.{l}"] = h.detach().cpu(), c.detach().cpu()
    res["dX"] = Xd.grad.cpu()
    if h0 is not None:
        for l in range(L):
            res[f"dh0.{l}"], res[f"dc0.{l}"] = hd[l].grad.cpu(), cd[l].grad.cpu()
    for k, p in net.named_parameters():
        res["grad." + k] = p.grad.cpu()
    if case["dtype"] == "bf16":
        eng = net._engine(Xd.device)
        (ws,) = eng.pool[(B, T, H, W, True, h0 is not None)]
        res["_dG"] = [stored_dG(eng, ws, l).cpu() for l in range(L)]
        res["_h"] = _top_h_images(eng, ws, range(1, T + 1) if rs else [T])
        res["_dpred"] = _head_cotangents(case, d)
    return res


# ---------------------------------------------------------------------------------------------------- the trainer's windows
def weights_of(case, d):
    """the drawn loss weights as the trainer receives them (None, an (Hc,) vector or an (Hc, Wc) map, f32): |N(0, 1)| with
    about a quarter of the entries exactly zero (never all of them)"""
    if case["wform"] == "none":
        return None
    w = d["w"].abs().numpy().astype(np.float32)
    w[d["wzero"].numpy() < -0.67] = 0.0
    if not (w > 0).any():
        w.flat[0] = 1.0
    return w


def window_loss(p, y, halo, w, sgn=None):
    """crop + MSE + L1 of the uncropped p (B, O', H, W) against y (B, ..., Hc, Wc) -- oracle.loss_mse_l1 -- or with a map
    w (Hc, Wc) the weighted mean of tests/weighted_loss_model.loss_torch, restated: a cell of weight 0 enters nothing,
    cnt = N O' sum(w) with the sum of the f32 map taken in f64.  Returns (loss, loss for the gradient, d, cnt): with ``sgn``
    (crop-shaped, values -1 / 0 / +1) the second has the L1 term as sum w sgn d where sgn != 0 -- the same value up to
    2 w |d| / cnt at the cells where sgn is not d's own sign, and there the subgradient ``sgn`` (see device_side)."""
    Hc, Wc = y.shape[-2], y.shape[-1]
    pc = O.crop_pred(p, halo, (Hc, Wc))
    yv = y.reshape(pc.shape)
    if w is None:
        wt, dlt, cnt = torch.ones(Hc, Wc), pc - yv, float(pc.numel())
        loss = O.loss_mse_l1(yv, pc)
    else:
        wt = torch.from_numpy(w)
        dlt = torch.where(wt > 0, pc - yv, torch.zeros_like(pc))
        cnt = float(dlt.numel() // (Hc * Wc)) * float(w.astype(np.float64).sum())
        loss = (wt * dlt * dlt).sum() / cnt + (wt * dlt.abs()).sum() / cnt
    if sgn is None:
        return loss, loss, dlt, cnt
    l1 = torch.where(sgn != 0, sgn * dlt, dlt.abs())
    return loss, (wt * dlt * dlt).sum() / cnt + (wt * l1).sum() / cnt, dlt, cnt


def device_side(dp_dev, p_shape, y, halo, w, sq, d_or, dtype):
    """The L1 term's derivative sign(d) jumps at d = pred - y = 0.  Where |d| is below the error of the device's prediction
    the device and the oracle may stand on different sides, and d loss / d pred then differs by 2 w / cnt at that cell --
    with a small crop a few such cells are several per cent of everything downstream (seed 215 --train-opts #1, bf16, one
    1x1 layer, 15 x 8 crop, B = 2: the SAME window trained alone, unsegmented, unweighted misses 3e-2 with 3.1e-2 on the layer's
    weights and 4.0e-2 on the head's bias, while f32 agrees to 1.1e-6 -- no kernel is wrong, the reference is not
    differentiable there).  The oracle keeps its OWN subgradient everywhere except at the cells that can legitimately stand on
    the other side, and what it takes from the device is bounded three ways:
      (a) q = dpred cnt / w must be a value of 2 d + sign d on every cell that carries weight: |q| >= 1 (or exactly 0).  A
          loss pass with the wrong sign at |d| < 1/2 gives |q| = 1 - 2 |d| < 1 and fails here; returned as ``qmin``.
      (b) then d_dev = (q - sign q) / 2 is the device's own d, hence its prediction d_dev + y on the crop, gated against the
          oracle's like any prediction (``pred.N``); a wrong sign at |d| >= 1/2 puts d_dev off by 1 there.  d loss / d pred
          itself is gated too (``dpred.N``) against the oracle's.
      (c) a cell whose sign differs is ADOPTED (the oracle uses the device's sign there) only where the oracle's own |d| is
          within what gate (b) lets a prediction be off: |d| <= LIM * max |pred| (f32: exactly the per-cell bound of the
          max-abs gate; bf16: below anything the rel-L2 gate implies per cell, since max |pred| <= ||pred||_2), and in bf16
          the adopted cells together within sum d^2 <= (LIM ||pred||_2)^2, which the rel-L2 gate implies for cells that
          truly changed sides (|d| <= |error| there); smallest |d| first.  Everywhere else, and for every cell in f32 beyond
          1e-3 of the largest prediction, the plain oracle stands and a device on the other side shows in ``dpred.N`` and in
          every gradient.
    Returns (sgn, d_dev, live, stats): sgn is +-1 at the adopted cells and 0 elsewhere (crop-shaped, p's layout); stats =
    dict(flips, refused [sign differs, not adopted], maxd [largest adopted |d|], bound, qmin)."""
    Hc, Wc = y.shape[-2], y.shape[-1]
    B = p_shape[0]
    dp = dp_dev.double()
    if sq:      # images t B + b -> (B, T O', H, W)
        T = dp.shape[0] // B
        dp = dp.view(T, B, *dp.shape[1:]).transpose(0, 1).reshape(p_shape)
    dpc = O.crop_pred(dp.view(p_shape), halo, (Hc, Wc))
    wt = torch.ones(Hc, Wc, dtype=torch.float64) if w is None else torch.from_numpy(w).double()
    cnt = float(dpc.numel() // (Hc * Wc)) * float(wt.sum())
    live = (wt > 0).expand_as(dpc)
    q = torch.where(live, dpc * cnt / torch.where(wt > 0, wt, torch.ones_like(wt)), torch.zeros_like(dpc))
    sgn_dev = torch.sign(q)
    d_dev = (q - sgn_dev) / 2
    on = live & (q != 0)
    qmin = float(q.abs()[on].min()) if bool(on.any()) else 1.0
    d_or = d_or.double()
    pr = torch.where(live, d_or + y.reshape(d_or.shape).double(), torch.zeros_like(d_or))
    bound = LIM[dtype] * float(pr.abs().max())
    differs = on & (sgn_dev != torch.sign(d_or))
    adopt = differs & (d_or.abs() <= bound)
    if dtype == "bf16" and bool(adopt.any()):
        idx = adopt.flatten().nonzero().flatten()
        order = idx[torch.argsort(d_or.flatten()[idx].abs())]
        within = torch.cumsum(d_or.flatten()[order] ** 2, 0) <= (LIM[dtype] * float(pr.norm())) ** 2
        adopt = torch.zeros_like(adopt).flatten()
        adopt[order[within]] = True
        adopt = adopt.view(differs.shape)
    sgn = torch.where(adopt, sgn_dev, torch.zeros_like(sgn_dev)).float()
    stats = dict(flips=int(adopt.sum()), refused=int((differs & ~adopt).sum()), cells=int(live.sum()),
                 maxd=float(d_or.abs()[adopt].max()) if bool(adopt.any()) else 0.0, bound=bound, qmin=qmin)
    return sgn, d_dev, live, stats


def oracle_window(leaf, X, y, halo, w, sq, h0=None, c0=None, last_only=0, dp_dev=None, dtype="f32"):
    """One window through the oracle under autograd: the loss backward into ``leaf`` (gradients ADD across calls, as the
    bucket's do).  ``last_only`` = S (--self-check): truncated BPTT, the steps before the last S run without a graph.
    ``dp_dev``: the device's d loss / d pred of this window (device_side; ``dtype`` sizes its bounds).
    Returns dict(loss, hs, cs, dG [per layer], h, dpred, and with dp_dev pred / pred_dev / kink): the final state, and the
    oracle's own summands of the bias gradients (dG, all steps) and of the head's weight gradient (top h and d loss / d pred,
    image order t B + b)."""
    B, T = X.shape[:2]
    t0 = 0
    if last_only:
        t0 = T - last_only
        with torch.no_grad():
            _, h0, c0 = O.convlstm_forward(X[:, :t0], leaf, return_states=True, h0=h0, c0=c0)
    pre, toph = {}, []
    pred, seq, hs, cs = O.convlstm_forward(X[:, t0:], leaf, return_states=True, return_sequence=True, h0=h0, c0=c0, preact=pre,
                                           top_h=toph)
    p = seq if sq else pred
    p.retain_grad()
    sgn = d_dev = live = kink = None
    if dp_dev is not None:
        with torch.no_grad():
            d_or = window_loss(p.detach(), y, halo, w)[2]
        sgn, d_dev, live, kink = device_side(dp_dev, p.shape, y, halo, w, sq, d_or, dtype)
    loss, loss_g, dlt, _ = window_loss(p, y, halo, w, sgn)
    loss_g.backward()
    L, Tg, Oc = len(hs), T - t0, pred.shape[1]
    r = dict(loss=float(loss.detach()), hs=[h.detach() for h in hs], cs=[c.detach() for c in cs])
    if dp_dev is not None:
        # the prediction on the cells that carry weight, as d = pred - y (y is common to both sides), scaled for the gate by
        # the prediction itself: pred = d + y
        yv = y.reshape(dlt.shape).double()
        z = torch.zeros_like(d_dev)
        r["pred"], r["pred_dev"] = torch.where(live, dlt.detach().double() + yv, z), torch.where(live, d_dev + yv, z)
        r["kink"] = kink
    r["dG"] = [torch.cat([pre[(l, t)].grad for t in range(Tg)]) for l in range(L)]
    if sq:
        r["h"] = torch.cat([h.detach() for h in toph])
        r["dpred"] = p.grad.view(B, Tg, Oc, *p.shape[-2:]).transpose(0, 1).reshape(Tg * B, Oc, *p.shape[-2:])
    else:
        r["h"], r["dpred"] = toph[-1].detach(), p.grad
    return r


def check_kink(tag, name, kink, verbose):
    """bound (a) of device_side, and the record of what was adopted (printed with --only, and whenever a cell was)"""
    if verbose or kink["flips"] or kink["refused"]:
        print(f"     {name}: {kink['flips']} of {kink['cells']} cells on the other side of d = 0 adopted (largest |d| "
              f"{kink['maxd']:.3e}, bound {kink['bound']:.3e}), {kink['refused']} beyond the bound; min |dpred cnt / w| "
              f"{kink['qmin']:.7f}", flush=True)
    assert kink["qmin"] >= 1.0 - 1e-5, (tag, name, "d loss / d pred is no value of (2 d + sign d) w / cnt", kink["qmin"])
    assert kink["flips"] == 0 or kink["maxd"] <= kink["bound"], (tag, name, kink)


def _stored_factors(case, net, tr, has_init):
    """bf16: what the step left in its workspace -- the whole window's dG, top h and dpred (one resident window), or segment
    0's dG alone (n >= 2: the S-step training workspace ends on the first segment)"""
    L, B, T, H, W, S = case["L"], case["B"], case["T"], case["H"], case["W"], case["S"]
    eng = net._engine(tr.device)
    if case["n"] > 1:
        (ws,) = eng.pool[(B, S, H, W, True, True)]
        return {"_dG0": [stored_dG(eng, ws, l).cpu() for l in range(L)]}
    (ws,) = eng.pool[(B, T, H, W, True, has_init)]
    sq = case.get("sequence_loss", False)
    return {"_dG": [stored_dG(eng, ws, l).cpu() for l in range(L)], "_h": _top_h_images(eng, ws, range(1, T + 1) if sq else [T]),
            "_dpred": tr._dpred.detach().clone().cpu().view(-1, case["out"], H, W)}


def _ref_factors(ref, wins, S, B, n):
    ref["_dG"] = [torch.cat([r["dG"][l] for r in wins]) for l in range(len(wins[0]["dG"]))]
    ref["_h"], ref["_dpred"] = torch.cat([r["h"] for r in wins]), torch.cat([r["dpred"] for r in wins])
    if n > 1:
        ref["_dG0"] = [g[:S * B] for g in wins[-1]["dG"]]       # (the last window run: its first S steps)
    if "grad" in wins[0]:       # each window's own contribution to the bucket, with its own summands
        ref["_win"] = [{"grad": r["grad"], "_dG": r["dG"], "_h": r["h"], "_dpred": r["dpred"]} for r in wins]


# ---------------------------------------------------------------------------------------------------- --train-opts
def train_opts_oracle(case, d, params, corrupt=None, dp_dev=None):
    """``corrupt`` (--self-check): "truncate" = only the last segment is back-propagated; "drop" = the first window is left
    out of the sum.  ``dp_dev``: per window the device's d loss / d pred (device_signs); without it the plain oracle, whose
    gradient norm sizes max_grad_norm before anything runs on the device."""
    halo, w = tuple(case["halo"]), weights_of(case, d)
    if w is not None and w.ndim == 1:
        w = np.ascontiguousarray(np.broadcast_to(w[:, None], (len(w), case["W"] - 2 * halo[1])))
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    ref, wins = {}, []
    before = {k: torch.zeros_like(v) for k, v in leaf.items()}
    for j in range(case["acc"]):
        r = oracle_window(leaf, d[f"X.{j}"], d[f"y.{j}"], halo, w, case["sequence_loss"],
                          last_only=case["S"] if corrupt == "truncate" else 0, dp_dev=None if dp_dev is None else dp_dev[j],
                          dtype=case["dtype"])
        ref[f"loss.{j}"] = r["loss"]
        if dp_dev is not None:
            ref[f"pred.{j}"], ref[f"_pred_dev.{j}"], ref[f"_kink.{j}"] = r["pred"], r["pred_dev"], r["kink"]
            ref[f"dpred.{j}"] = r["dpred"]
        r["grad"] = {"grad." + k: v.grad.detach() - before[k] for k, v in leaf.items()}
        before = {k: v.grad.detach().clone() for k, v in leaf.items()}
        wins.append(r)
        if corrupt == "drop" and j == 0:
            for v in leaf.values():
                v.grad = None
    for k, v in leaf.items():
        ref["grad." + k] = v.grad.detach()
    ref["_norm"] = float(torch.cat([v.grad.double().flatten() for v in leaf.values()]).norm()) / case["acc"]
    if case["clip"] is not None:
        ref["norm"] = ref["_norm"]
    if corrupt is None:
        _ref_factors(ref, wins, case["S"], case["B"], case["n"])
    else:       # the factors are not the fault's subject: the summands' lists keep the device's shapes
        full = train_opts_oracle(case, d, params, dp_dev=dp_dev)
        for k in ("_dG", "_h", "_dpred", "_dG0", "_win"):
            if k in full:
                ref[k] = full[k]
    return ref


def train_opts_device(case, d, params, ref):
    from nasa_niswan_amd.trainer import FusedTrainer
    net = _net(pkg.ConvLSTM(case["C"], case["hidden"], case["ks"], case["L"], out_channels=case["out"], compute_dtype=case["dtype"]))
    net.load_state_dict(params)
    mg =None if case["clip"] is None else case["clip"] * ref["_norm"]
    tr = FusedTrainer(net, lr=1e-3, halo=tuple(case["halo"]), sequence_loss=case["sequence_loss"], loss_weights=weights_of(case, d),
                      max_grad_norm=mg, bptt_segments=case["n"], accumulate_steps=case["acc"])
    res = {"_dp": []}
    # bf16, one resident window per call: after EVERY call the workspace holds that window whole, so each window's own
    # contribution to the bucket (the bucket minus what it held before the call) is gated on that window's stored factors
    per_window = case["dtype"] == "bf16" and case["n"] == 1
    wins, before = [], None
    for j in range(case["acc"]):
        res[f"loss.{j}"] = float(tr.step(_dev(d[f"X.{j}"]), _dev(d[f"y.{j}"])))
        res["_dp"].append(tr._dpred.detach().clone().cpu())
        res[f"dpred.{j}"] = res["_dp"][-1].view(-1, case["out"], case["H"], case["W"])
        if per_window:
            torch.cuda.synchronize()
            now = _named_grads(net, tr.flat)
            win = _stored_factors(case, net, tr, False)
            win["grad"] = now if before is None else {k: now[k] - before[k] for k in now}
            wins.append(win)
            before = now
    torch.cuda.synchronize()
    res.update(_named_grads(net, tr.flat))
    if mg is not None:
        st = tr.grad_stats()
        assert st["calls"] == 1 and st["applied"] == 1, (case["tag"], st)
        assert (st["clipped"] == 1) == (case["clip"] < 1.0), (case["tag"], st, "clip decision")
        res["norm"] = st["last_norm"]
    if per_window:
        res["_win"] = wins
    elif case["dtype"] == "bf16":
        res.update(_stored_factors(case, net, tr, False))
    return res


# ---------------------------------------------------------------------------------------------------- --stateful
def stateful_run(case, d, params, self_check):
    """both chunks, device and oracle interleaved (chunk 2's reference starts from what the device held); returns
    (worst figure, True if the self-check was tried)"""
    from nasa_niswan_amd.trainer import FusedTrainer
    L, B, halo, dtype, tag = case["L"], case["B"], tuple(case["halo"]), case["dtype"], case["tag"]
    net = _net(pkg.ConvLSTM(case["C"], case["hidden"], case["ks"], L, out_channels=case["out"], compute_dtype=dtype))
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=1e-3, halo=halo, stateful=True, bptt_segments=case["n"])
    worst, tried = 0.0, False
    p, h0, c0 = params, None, None
    for j in range(2):
        reset = case["reset"] if j == 1 else None
        res = {"loss": float(tr.step(_dev(d[f"X.{j}"]), _dev(d[f"y.{j}"]), reset=reset))}
        torch.cuda.synchronize()
        res.update(_named_grads(net, tr.flat))
        dp_dev = tr._dpred.detach().clone().cpu()
        held = [(h.cpu(), c.cpu()) for h, c in tr.state.tensors()]
        for l, (h, c) in enumerate(held):
            res[f"h_T.{l}"], res[f"c_T.{l}"] = h, c
        if dtype == "bf16":
            res.update(_stored_factors(case, net, tr, True))
            if case["n"] > 1:       # the carried state is the h the head read, and dpred is the last segment's: the head's factors
                res["_h"], res["_dpred"] = held[-1][0], tr._dpred.detach().clone().cpu().view(-1, case["out"], case["H"], case["W"])

        def oracle(ignore_reset=False):
            hs, cs = h0, c0
            if hs is not None and reset is not None and not ignore_reset:
                m = [True] * B if reset is True else reset
                keep = torch.tensor([0.0 if v else 1.0 for v in m]).view(-1, 1, 1, 1)
                hs, cs = [h * keep for h in hs], [c * keep for c in cs]
            leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
            r = oracle_window(leaf, d[f"X.{j}"], d[f"y.{j}"], halo, None, False, h0=hs, c0=cs, dp_dev=dp_dev, dtype=dtype)
            ref = {"loss": r["loss"], "pred": r["pred"], "_pred_dev": r["pred_dev"], "dpred": r["dpred"], "_kink": r["kink"]}
            for k, v in leaf.items():
                ref["grad." + k] = v.grad.detach()
            for l in range(L):
                ref[f"h_T.{l}"], ref[f"c_T.{l}"] = r["hs"][l], r["cs"][l]
            _ref_factors(ref, [r], case["S"], B, case["n"])
            return ref

        ref = oracle()
        res["pred"], res["dpred"] = ref["_pred_dev"], dp_dev.view(-1, case["out"], case["H"], case["W"])
        check_kink(tag, f"chunk {j + 1}", ref["_kink"], case.get("verbose", False))
        worst = max(worst, compare(f"{tag} chunk {j + 1}", dtype, res, ref, verbose=case.get("verbose", False)))
        if self_check and j == 1 and reset is not None:
            def ignoring():
                bad = oracle(ignore_reset=True)
                compare(tag, dtype, dict(res, pred=bad["_pred_dev"]), bad)
            expect_failure(tag, "the oracle ignores the reset", ignoring)
            tried = True
        # what chunk 2 starts from: the parameters and the state as the device holds them now
        p = {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}
        h0, c0 = [h for h, _ in held], [c for _, c in held]
    return worst, tried


# ---------------------------------------------------------------------------------------------------- --finetune
def finetune_run(case, d, params, self_check, tried):
    """Two steps of FusedTrainer(freeze_layers=f, weight_decay, layer_lr_scale), each checked from the parameters and moments
    the device held before it: the loss and the trained gradients against CPU autograd (bf16: the layers' weights; its
    biases and head sums cancel and are gated through the f32 cases), the frozen regions of the bucket, weights and moments
    bit-unchanged, and the new weights against torch.optim.AdamW stepping on the DEVICE's gradient (rtol 2e-6, atol 1e-7: the
    gate nint_adam_flat is held to).  Returns the worst gradient figure."""
    from nasa_niswan_amd.trainer import FusedTrainer
    L, f, wd, scales, halo, dtype, tag = case["L"], case["f"], case["wd"], case["scales"], tuple(case["halo"]), case["dtype"], case["tag"]
    lr, sentinel = 1e-3, 4321.5
    net = _net(pkg.ConvLSTM(case["C"], case["hidden"], case["ks"], L, out_channels=case["out"], compute_dtype=dtype))
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=lr, halo=halo, freeze_layers=f, weight_decay=wd, layer_lr_scale=scales)
    names = [k for k, _ in net.named_parameters()]
    frozen = lambda k: k.startswith("layers.") and int(k.split(".")[1]) < f
    n0 = tr.optimizer.n0
    assert n0 == tr.flat.offsets[2 * f], (tag, "first trained element")
    tr.flat.grad[:n0] = sentinel
    start = tr.flat.data[:n0].clone()
    worst = 0.0

    def adamw(p_before, m_before, v_before, grads, step, fault=None):
        leaf = {k: v.clone().requires_grad_(True) for k, v in p_before.items()}
        groups = []
        for k in names:
            if frozen(k) and fault != "unfrozen":
                continue
            l = int(k.split(".")[1]) if k.startswith("layers.") else L - 1
            decay = wd if leaf[k].dim() > 1 and fault != "no_decay" else 0.0
            groups.append(dict(params=[leaf[k]], lr=lr * scales[l], weight_decay=decay))
        opt = torch.optim.AdamW(groups, lr=lr, betas=(0.5, 0.999), eps=1e-8, foreach=False)
        for g in groups:
            (q,) = g["params"]
            k = next(n for n in names if leaf[n] is q)
            opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m_before[k].clone(), "exp_avg_sq": v_before[k].clone()}
            q.grad = grads[k].clone() if not frozen(k) else torch.ones_like(q)
        opt.step()
        return {k: v.detach() for k, v in leaf.items()}

    def close(new, want, what):
        for k in names:
            a, b = new[k], want[k]
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (tag, what, k, float((a - b).abs().max()))

    for j in range(2):
        view = lambda buf: {k: buf[o:o + p.numel()].view(p.shape).detach().clone().cpu() for (k, p), o in zip(net.named_parameters(), tr.flat.offsets)}
        p0, m0, v0 = view(tr.flat.data), view(tr.optimizer.exp_avg), view(tr.optimizer.exp_avg_sq)
        X, y = d[f"X.{j}"], d[f"y.{j}"]
        loss = float(tr.step(_dev(X), _dev(y)))
        torch.cuda.synchronize()
        leaf = {k: v.clone().requires_grad_(not frozen(k)) for k, v in p0.items()}
        lo = O.loss_mse_l1(y, O.crop_pred(O.convlstm_forward(X, leaf), halo, y.shape[-2:]))
        lo.backward()
        lo = float(lo.detach())
        assert abs(loss - lo) <= LOSS_LIM[dtype] * abs(lo), (tag, f"step {j + 1} loss", loss, lo)
        g_dev = view(tr.flat.grad)
        for k in names:
            if frozen(k):
                assert bool((g_dev[k] == sentinel).all()), (tag, "a frozen region of the gradient bucket was written", k)
                continue
            a, b = g_dev[k].double(), leaf[k].grad.double()
            assert torch.isfinite(a).all(), (tag, k)
            if dtype == "bf16" and not (k.startswith("layers.") and a.dim() > 1):
                continue
            e = _err(dtype, a, b)
            if case.get("verbose"):
                print(f"     step {j + 1} grad.{k}: {e:.3e}", flush=True)
            assert e <= LIM[dtype], (tag, f"step {j + 1}", k, e)
            worst = max(worst, e)
        new = view(tr.flat.data)
        close(new, adamw(p0, m0, v0, g_dev, j + 1), f"step {j + 1}: weights against torch.optim.AdamW on the device's gradient")
        if self_check:
            for name, what, applies in (("no_decay", "the reference's AdamW has no weight decay", wd > 0),
                                        ("unfrozen", "the reference trains the frozen layers too", f > 0)):
                if applies and not tried.get(name):
                    expect_failure(tag, what, lambda: close(new, adamw(p0, m0, v0, g_dev, j + 1, fault=name), what))
                    tried[name] = True
    assert torch.equal(tr.flat.data[:n0], start), (tag, "a frozen weight moved")
    assert not tr.optimizer.exp_avg[:n0].any() and not tr.optimizer.exp_avg_sq[:n0].any(), (tag, "a frozen moment was written")
    return worst


def expect_failure(tag, what, fn):
    try:
        fn()
    except AssertionError as e:
        msg = " ".join(str(e).split())
        print(f"self-check ok: {what} -> the comparison fails ({msg[:160]})", flush=True)
        return
    raise SystemExit(f"SELF-CHECK FAILED {tag}: {what}, and every gate still passes -- the screen cannot see this fault")


# ---------------------------------------------------------------------------------------------------- main
def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--big", action="store_true", help="module mode on grids around the bench size (60-110 x 100-170, ragged), B = 1-3, T = 1-3")
    ap.add_argument("--wide", action="store_true", help="module mode on shapes the 8-wave 128-column weight-gradient kernel holds (bf16, hidden 32 / 64 / 128), the family forced on and off (nint_layer.wide = 2 / 1)")
    ap.add_argument("--dataset", action="store_true", help="the device preproc (z-score, level fusion, cyclic / reflect halo padding) of a resident synthetic record, as a batch tensor and through the model's input slab, against oracle/preproc_oracle.py instead")
    ap.add_argument("--cell", action="store_true", help="ConvLSTMCell(x, h, c) with a given state (forward, all five gradients) against oracle.cell_forward instead")
    ap.add_argument("--trainer", action="store_true", help="FusedTrainer.step (fused head / loss pass, flat gradient bucket) against oracle.train_step instead")
    ap.add_argument("--state", action="store_true", help="ConvLSTM.forward(x, state, return_state=...) with a drawn state and cotangents on every output, against oracle.convlstm_forward(h0=, c0=)")
    ap.add_argument("--train-opts", action="store_true", help="FusedTrainer.step with drawn bptt_segments, accumulate_steps, loss_weights, max_grad_norm, sequence_loss: losses and the bucket against CPU autograd over the whole window")
    ap.add_argument("--stateful", action="store_true", help="two chunks through FusedTrainer(stateful=True), the second with a drawn reset, each checked from the state and parameters the device held")
    ap.add_argument("--finetune", action="store_true", help="two steps of FusedTrainer with a drawn number of frozen layers (0 ... all), weight decay and per-layer lr scales: loss and trained gradients against CPU autograd, the update against torch.optim.AdamW, the frozen regions untouched")
    ap.add_argument("--closed-loop", action="store_true", help="ConvLSTM(feedback=True)(x[, state], free_from=s): the per-step predictions of a drawn stack, grid, number of feedback channels, first fed step, state, storage type, boundary condition and input layout against the CPU model tests/closed_loop_model.py, and bit for bit against the open-loop pass over the input with those predictions substituted")
    ap.add_argument("--rollout", action="store_true", help="ConvLSTM(feedback=True)(x, free_from=F, feedback_grad=True): outputs, every parameter gradient and dx of a drawn stack, grid, number of feedback channels, first fed step F >= 1, storage type, boundary condition, input layout and cotangents (per step, last step, both) against the CPU model tests/rollout_model.py under CPU autograd in f64")
    ap.add_argument("--sampled", action="store_true", help="ConvLSTM(feedback=True)(x[, state], free_mask=M[, feedback_grad=True]): a drawn stack, grid, number of feedback channels, storage type, boundary condition, input layout, state and (B, T) feed mask of a drawn density.  Forward: the per-step predictions against the CPU model tests/sampled_model.py and bit for bit against the open-loop pass over the input with those predictions substituted where the mask says.  Without a fed image at step 0: outputs, every parameter gradient and dx under drawn cotangents (per step or last step) against the model under CPU autograd in f64.  --self-check: the reference of the first case with a mixed step is computed as if every image were fed from the first fed step on")
    ap.add_argument("--residual", action="store_true", help="ConvLSTM(feedback=True, residual=True)(x[, state], free_from=F | free_mask=M[, feedback_grad=True]): a drawn stack, grid, number of feedback channels, storage type, boundary condition, input layout, state and first fed step F >= 1 or (B, T) feed mask with column 0 clear.  Forward: the per-step predictions p_t = x_t[feedback channels] + head(h_t) against the CPU model tests/residual_model.py and bit for bit against the residual open-loop pass over the input with those predictions substituted where fed.  Then outputs, every parameter gradient and dx under drawn cotangents against the model under CPU autograd in f64.  --self-check: the reference of the first case is the non-residual model (the base dropped)")
    ap.add_argument("--noise", action="store_true", help="ConvLSTM(x, input_noise=InputNoise(std, channels=(c0, n), seed, draw, step0, lane0)): a drawn stack, grid, noise span, sigma per channel (one may be 0), storage type, boundary condition, input layout and generator key.  The noisy pass -- outputs, every parameter gradient and dx under drawn cotangents -- against the CPU oracle under autograd in f64 on the PRE-NOISED input, which tests/noise_model.py builds on the host from its own Philox and normals; a pass with an all-zero std is the pass without the argument, bit for bit.  --self-check: the reference of the first case is the clean input")
    ap.add_argument("--ensemble", action="store_true", help="nint_ens_accum alone: drawn members, samples (beyond one launch's 64 too), outputs, grid, crop window, slots with -1 and an empty slot, and the members contiguous or read in place from a roll-out's (lanes, T, O, H, W) buffer with shuffled, overlapping sample offsets.  Integer data: every plane, sample column and bin bit for bit against the numpy model tests/ensemble_model.py; normal data: the maps and bins bit for bit, the sample rows within the any-order bound of their f64 addends")
    ap.add_argument("--self-check", action="store_true", help="with --state / --train-opts / --stateful / --finetune / --sampled / --residual: corrupt the reference after the first passing case and require the comparison to fail")
    ap.add_argument("--guarded", action="store_true", help="every mode: the device side of each case allocates through oracle/guarded_alloc.py in poison mode (guards around every buffer, `empty` payloads 0xFF), its inputs and parameters in arenas of their own; the comparison stays what it is and every guard byte is checked after each case.  With --self-check (any mode): one guard byte is flipped after the first passing case and the check has to fail (the reference is then not corrupted)")
    ap.add_argument("--list", action="store_true", help="print the drawn cases as JSON lines and exit (no GPU, the package is not imported)")
    ap.add_argument("--only", type=int, default=-1, help="replay the random stream up to this iteration and run it alone, printing every tensor's error")
    ap.add_argument("--force-wave", type=int, default=None, help="with --only: nint_seq.wave for the replayed case instead of the rotation's value")
    ap.add_argument("--force-dtype", choices=["f32", "bf16"], default=None, help="with --only: the storage type of the replayed case instead of the alternation's (is the miss the arithmetic's, or the storage type's?)")
    args = ap.parse_args(argv)
    modes = [m for m in ("dataset", "cell", "trainer", "state", "train_opts", "stateful", "finetune", "closed_loop", "rollout", "sampled",
                         "residual", "noise", "ensemble") if getattr(args, m)]
    if len(modes) > 1 and not all(m in OLD_MODES for m in modes):
        ap.error("one of --state / --train-opts / --stateful / --finetune / --closed-loop / --rollout / --sampled / --residual at a time, and none of the other modes with it")
    args.mode = modes[0] if modes else "plain"          # (--dataset before --cell before --trainer, as ever)
    if args.mode == "ensemble" and (args.self_check or args.guarded):
        ap.error("--ensemble has no reference to corrupt and allocates its own buffers: not with --self-check / --guarded")
    if args.mode in ("closed_loop", "rollout", "sampled", "residual", "noise", "ensemble") and (args.big or args.wide):
        ap.error("--closed-loop / --rollout / --sampled / --residual / --noise draw their own shapes: not with --big / --wide")
    if args.self_check and args.mode not in NEW_MODES + SAMPLED_MODES + RESIDUAL_MODES + NOISE_MODES and not args.guarded:
        ap.error("--self-check needs --state, --train-opts, --stateful, --finetune, --sampled, --residual or --noise (or --guarded)")
    # --guarded --self-check is the guard's own self-check; the reference stays what it is
    args.guard_self_check = args.self_check and args.guarded
    if args.guard_self_check:
        args.self_check = False
    return args


def run_old(case, d, args, worst):
    """the four modes of the first version: net(x), the plain trainer step, one cell, the preproc"""
    it, tag, dtype = case["it"], case["tag"], case["dtype"]
    L, hidden, ks, C, out, B, T, H, W = (case[k] for k in ("L", "hidden", "ks", "C", "out", "B", "T", "H", "W"))
    if args.mode == "dataset":
        from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
        from nasa_niswan_amd.engine import LayerCfg, SeqEngine
        from oracle import preproc_oracle as PO
        levels, gh, gw, py, px, mode, seq = (case[k] for k in ("levels", "gh", "gw", "py", "px", "pad_mode", "seq"))
        Cin = 3 * levels + 2
        ds = SyntheticE33OMA_CRNN("train", padding=(gh + 2 * py, gw + 2 * px), in_channels=Cin, sequence_length=seq, levels=levels,
                                  n_steps=12 + seq, grid=(gh, gw), pad_mode=mode, device="cuda", seed=it)
        assert len(ds) == case["nwin"], (tag, len(ds), case["nwin"])
        idx = case["idx"]
        X, y = ds.device_batch(idx)
        torch.cuda.synchronize()
        for b, ix in enumerate(idx):
            (u, v, w_, pr, src), yr = ds.window(ix)
            sq = (lambda a: a if levels > 1 else a[:, 0])
            ref = PO.preproc_sample(sq(u), sq(v), sq(w_), pr, src, ds.X_mean, ds.X_std, (gh + 2 * py, gw + 2 * px), mode)
            np.testing.assert_allclose(X[b].cpu().numpy(), ref, rtol=1e-6, atol=1e-6, err_msg=tag)
        # ... and straight into a model's input slab (folded or plain), then unpacked again
        k0 = case["k0"]
        eng = SeqEngine([LayerCfg(Cin, 16, k0)], dtype, "cuda")
        ws = eng.acquire(len(idx), seq, gh + 2 * py, gw + 2 * px, False, False)
        sb = ds.slab_batch(idx)[0]
        eng.pack_input(ws, sb)
        ws2 = eng.acquire(len(idx), seq, gh + 2 * py, gw + 2 * px, False, False)
        eng.pack_input(ws2, X)
        torch.cuda.synchronize()
        assert torch.equal(ws.xs, ws2.xs), (tag, "slab path differs from preproc -> pack", bool(eng.cfgs[0].xfold))
        print(f"ok   {tag} k0={k0} fold={bool(eng.cfgs[0].xfold)}", flush=True)
        return
    if args.mode == "cell":
        Ch, k, has_bias = hidden[0], ks[0], case["has_bias"]
        cell = _net(pkg.ConvLSTMCell(C, Ch, k, bias=has_bias, compute_dtype=dtype))
        Wt = d["Wt"] / np.sqrt((C + Ch) * k * k)
        bt = d["bt"] * 0.2 if has_bias else None
        with torch.no_grad():
            cell.conv.weight.copy_(Wt)
            if has_bias:
                cell.conv.bias.copy_(bt)
        x, h, c, gh, gc = d["x"], d["h"] * 0.5, d["c"], d["gh"], d["gc"]
        xd, hd, cd = (_dev(t).requires_grad_(True) for t in (x, h, c))
        h1, c1 = cell(xd, (hd, cd))
        ((h1 * _dev(gh)).sum() + (c1 * _dev(gc)).sum()).backward()
        torch.cuda.synchronize()
        xo, ho, co = (t.clone().requires_grad_(True) for t in (x, h, c))
        Wo = Wt.clone().requires_grad_(True)
        bo = bt.clone().requires_grad_(True) if has_bias else None
        pre = []
        h1o, c1o = O.cell_forward(xo, ho, co, Wo, bo, pre)
        ((h1o * gh).sum() + (c1o * gc).sum()).backward()
        res = {"h1": (h1.detach().cpu(), h1o.detach()), "c1": (c1.detach().cpu(), c1o.detach()), "dx": (xd.grad.cpu(), xo.grad),
               "dh": (hd.grad.cpu(), ho.grad), "dc": (cd.grad.cpu(), co.grad), "dW": (cell.conv.weight.grad.cpu(), Wo.grad)}
        if has_bias:
            res["db.bias"] = (cell.conv.bias.grad.cpu(), bo.grad)
        w = 0.0
        for k2, (a, b) in res.items():
            a, b = a.double(), b.double()
            assert torch.isfinite(a).all(), (tag, k2)
            if dtype == "bf16" and k2.endswith("bias"):
                eng = cell._engine(xd.device)
                (ws,) = eng.pool[(B, 1, H, W, True, True)]
                check_bias_grad(tag, k2, a, b, stored_dG(eng, ws, 0).cpu(), pre[0].grad, dtype)
                continue
            e = _err(dtype, a, b)
            if args.only >= 0:
                print(f"     {k2}: {e:.3e}", flush=True)
            assert e <= LIM[dtype], (tag, k2, e)
            w = max(w, e)
        worst[dtype] = max(worst[dtype], w)
        print(f"ok   {tag}  worst {w:.2e}", flush=True)
        return
    if args.mode == "trainer":
        from nasa_niswan_amd.trainer import FusedTrainer
        hy, hx = case["halo"]
        params = O.synth_params(C, hidden, ks, L, out_channels=out, seed=it)
        X, y = d["X"], d["y"]
        net = _net(pkg.ConvLSTM(C, hidden, ks, L, out_channels=out, compute_dtype=dtype))
        net.load_state_dict(params)
        tr = FusedTrainer(net, lr=1e-3, halo=(hy, hx))
        loss = float(tr.step(_dev(X), _dev(y)))
        torch.cuda.synchronize()
        _, _, lo, _, grads = O.train_step(params, None, X, y, lr=1e-3, halo=(hy, hx))
        assert abs(loss - lo) <= LOSS_LIM[dtype] * abs(lo), (tag, "loss", loss, lo)
        w = abs(loss - lo) / abs(lo)
        for i, (k, p) in enumerate(net.named_parameters()):
            a, b = tr.flat.grad_view(i).detach().cpu().double(), grads[k].double()
            assert torch.isfinite(a).all(), (tag, k)
            e = _err(dtype, a, b)
            if args.only >= 0:
                print(f"     {k}: {e:.3e}", flush=True)
            assert e <= LIM[dtype], (tag, k, e)
            w = max(w, e)
        worst[dtype] = max(worst[dtype], w)
        print(f"ok   {tag} halo=({hy},{hx}) trainer  worst {w:.2e}", flush=True)
        return
    params = O.synth_params(C, hidden, ks, L, out_channels=out, seed=it)
    X, wgt = d["X"], d["wgt"]
    net = _net(pkg.ConvLSTM(C, hidden, ks, L, out_channels=out, compute_dtype=dtype))
    net.load_state_dict(params)
    Xd = _dev(X).requires_grad_(True)
    pred = net(Xd)
    (pred * _dev(wgt)).sum().backward()
    torch.cuda.synchronize()
    leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    Xo = X.clone().requires_grad_(True)
    pre = {}
    po, hso, _ = O.convlstm_forward(Xo, leaf, return_states=True, preact=pre)
    (po * wgt).sum().backward()
    res = {"pred": (pred.detach().cpu(), po.detach()), "dX": (Xd.grad.cpu(), Xo.grad)}
    for k, p in net.named_parameters():
        res["grad." + k] = (p.grad.cpu(), leaf[k].grad)
    w = 0.0
    for k, (a, b) in res.items():
        a, b = a.double(), b.double()
        assert torch.isfinite(a).all(), (tag, k)
        if dtype == "f32":
            e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
            assert e <= 1e-3, (tag, k, e)
        elif k.startswith("grad.layers.") and k.endswith("bias"):
            # sums that cancel: gated on their two factors, not on the end-to-end figure (check_bias_grad)
            l = int(k.split(".")[2])
            eng = net._engine(Xd.device)
            (ws,) = eng.pool[(B, T, H, W, True, False)]
            check_bias_grad(tag, k, a, b, stored_dG(eng, ws, l).cpu(), torch.cat([pre[(l, t)].grad for t in range(T)]), dtype)
            continue
        elif k == "grad.conv.weight":
            # the head's weight gradient: a sum over pixels with random signs (check_head_wgrad)
            eng = net._engine(Xd.device)
            (ws,) = eng.pool[(B, T, H, W, True, False)]
            e = check_head_wgrad(tag, a, b, eng.h_last(ws, L - 1).cpu(), hso[-1].detach(), wgt)
            if args.only >= 0:
                print(f"     {k}: rel-L2 {e:.3e} (gated on its factors)", flush=True)
        else:
            e = float((a - b).norm() / (b.norm() + 1e-30))
            if args.only >= 0:
                print(f"     {k}: rel-L2 {e:.3e}  |ref| {float(b.norm()):.3e}", flush=True)
                if k == "grad.conv.weight":
                    print("       hip   ", a.flatten().tolist()); print("       oracle", b.flatten().tolist())
            assert e <= 3e-2 or args.only >= 0, (tag, k, e)
        w = max(w, e)
    worst[dtype] = max(worst[dtype], w)
    print(f"ok   {tag}  worst {w:.2e}", flush=True)


def run_new(case, d, args, worst, tried):
    """--state / --train-opts / --stateful; ``tried``: the self-check faults already exercised (name -> True)"""
    tag, dtype, mode = case["tag"], case["dtype"], case["mode"]
    verbose = args.only >= 0
    case["verbose"] = verbose
    params = O.synth_params(case["C"], case["hidden"], case["ks"], case["L"], out_channels=case["out"], seed=case["it"])
    if mode == "stateful":
        w, did = stateful_run(case, d, params, args.self_check and not tried.get("reset"))
        if did:
            tried["reset"] = True
    elif mode == "finetune":
        w = finetune_run(case, d, params, args.self_check, tried)
    else:
        if mode == "state":
            ref = state_oracle(case, d, params)
            res = state_device(case, d, params)
            faults = [("zero_c0", "the oracle starts the last layer from c0 = 0", case["form"] != "none",
                       lambda: state_oracle(case, d, params, corrupt=True))]
        else:
            res = train_opts_device(case, d, params, train_opts_oracle(case, d, params))
            ref = train_opts_oracle(case, d, params, dp_dev=res["_dp"])
            for j in range(case["acc"]):
                res[f"pred.{j}"] = ref[f"_pred_dev.{j}"]
                check_kink(tag, f"window {j}", ref[f"_kink.{j}"], verbose)
            faults = [("truncate", "the oracle back-propagates the last segment only", case["n"] >= 2,
                       lambda: train_opts_oracle(case, d, params, corrupt="truncate", dp_dev=res["_dp"])),
                      ("drop", "one window is left out of the oracle's sum", case["acc"] >= 2,
                       lambda: train_opts_oracle(case, d, params, corrupt="drop", dp_dev=res["_dp"]))]
        w = compare(tag, dtype, res, ref, verbose)
        if args.self_check:
            for name, what, applies, bad in faults:
                if applies and not tried.get(name):
                    expect_failure(tag, what, lambda: compare(tag, dtype, res, bad()))
                    tried[name] = True
    worst[dtype] = max(worst[dtype], w)
    print(f"ok   {tag}  worst {w:.2e}", flush=True)


def closed_loop_run(case, d, args, worst):
    """--closed-loop: one case on the device against tests/closed_loop_model.py (f64, the fed value rounded to the storage type)"""
    tdir = os.path.join(ROOT, "tests")
    if tdir not in sys.path:
        sys.path.insert(0, tdir)
    import closed_loop_model as CLM
    tag, dtype = case["tag"], case["dtype"]
    C, out, T, s, L = case["C"], case["out"], case["T"], case["fb_from"], case["L"]
    params = O.synth_params(C, case["hidden"], case["ks"], L, out_channels=out, seed=case["it"])
    net = pkg.ConvLSTM(C, case["hidden"], case["ks"], L, out_channels=out, compute_dtype=dtype, lon_cyclic=case["cyclic"],
                       feedback=True, return_sequence=True)
    net.load_state_dict(params)
    net = _net(net)
    old_fold, engine.XFOLD = engine.XFOLD, case["fold"]
    try:
        net._engine(torch.device("cuda", torch.cuda.current_device()))
    finally:
        engine.XFOLD = old_fold
    state = [(d[f"h0.{l}"], d[f"c0.{l}"]) for l in range(L)] if case["with_state"] else None
    dev_state = None if state is None else [(_dev(h), _dev(c)) for h, c in state]
    X = _dev(d["X"])
    with torch.no_grad():
        pred, seq = net(X, dev_state, free_from=s)
        pred_o, seq_o = net(X, dev_state)
        # bit contract: the open-loop pass over the input that holds the predictions of the step before in its last channels
        X2 = X.clone()
        if s < T:
            sv = seq.view(case["B"], T, out, case["H"], case["W"])
            if s == 0:
                eng = next(iter(net._engines.values()))
                with eng.window(case["B"], T, case["H"], case["W"], False, True) as ws:
                    eng.load_state(ws, eng.state_from_tensors(dev_state))
                    X2[:, 0, C - out:] = eng.head_forward(ws, net.conv.weight, net.conv.bias, slot=0)
            X2[:, max(s, 1):, C - out:] = sv[:, max(s, 1) - 1:T - 1]
        pred2, seq2 = net(X2, dev_state)
    torch.cuda.synchronize()
    assert torch.equal(seq, seq2) and torch.equal(pred, pred2), (tag, "closed loop differs from the open loop on the substituted input")
    if s >= T:
        assert torch.equal(seq, seq_o), (tag, "nothing fed back, yet not the open-loop pass")
    p64 = {k: v.double() for k, v in params.items()}
    kw = dict(h0=[h.double() for h, _ in state], c0=[c.double() for _, c in state]) if state is not None else {}
    ref = CLM.forward(d["X"].double(), p64, free_from=s, cyclic=case["cyclic"], storage=dtype, **kw)
    w = compare(tag, dtype, dict(pred=pred.cpu(), seq=seq.cpu()), dict(pred=ref["pred"], seq=ref["seq"]), args.only >= 0)
    worst[dtype] = max(worst[dtype], w)
    print(f"ok   {tag}  worst {w:.2e}", flush=True)


def rollout_run(case, d, args, worst):
    """--rollout: one case on the device against tests/rollout_model.py (f64 under CPU autograd, the fed value rounded to f32 and
    passed straight through)"""
    tdir = os.path.join(ROOT, "tests")
    if tdir not in sys.path:
        sys.path.insert(0, tdir)
    import rollout_model as RM
    tag, dtype = case["tag"], case["dtype"]
    C, out, T, F, L = case["C"], case["out"], case["T"], case["fb_from"], case["L"]
    params = O.synth_params(C, case["hidden"], case["ks"], L, out_channels=out, seed=case["it"])
    net = pkg.ConvLSTM(C, case["hidden"], case["ks"], L, out_channels=out, compute_dtype=dtype, lon_cyclic=case["cyclic"],
                       feedback=True, return_sequence=True)
    net.load_state_dict(params)
    net = _net(net)
    old_fold, engine.XFOLD = engine.XFOLD, case["fold"]
    try:
        net._engine(torch.device("cuda", torch.cuda.current_device()))
    finally:
        engine.XFOLD = old_fold
    # (the drawn cotangents get a mean: a bias gradient is the plain sum of what reaches it, and zero-mean cotangents make that
    # sum a difference of large numbers whose relative error in bf16 measures the draw)
    dseq = d["dseq"] + 0.5 if case["cot"] in ("seq", "both") else None
    dpred = d["dpred"] + 0.5 if case["cot"] in ("last", "both") else None
    X = _dev(d["X"]).requires_grad_(True)
    pred, seq = net(X, free_from=F, feedback_grad=True)
    outs, cots = zip(*[(o, _dev(c)) for o, c in ((pred, dpred), (seq, dseq)) if c is not None])
    torch.autograd.backward(list(outs), list(cots))
    torch.cuda.synchronize()
    assert not bool(X.grad[:, F:, C - out:].any()), (tag, "a gradient on the fed channels of a fed step")
    p64 = {k: v.double() for k, v in params.items()}
    ref = RM.grads(d["X"].double(), p64, F, case["cyclic"], "f32", dpred, dseq)
    res = dict(pred=pred.detach().cpu(), seq=seq.detach().cpu(), dx=X.grad.cpu())
    want = dict(pred=ref["pred"], seq=ref["seq"], dx=ref["dx"])
    for k, p in net.named_parameters():
        res["d." + k], want["d." + k] = p.grad.cpu(), ref["params"][k]
    w = compare(tag, dtype, res, want, args.only >= 0)
    worst[dtype] = max(worst[dtype], w)
    print(f"ok   {tag}  worst {w:.2e}", flush=True)


def sampled_run(case, d, args, worst, tried):
    """--sampled: one case on the device against tests/sampled_model.py.  Forward (always, under no_grad): the fed value rounded
    to the storage type, and the bit contract.  Gradients (no fed image at step 0): f64 under CPU autograd, the fed value
    rounded to f32 and passed straight through.  ``tried`` (--self-check): "full_mask" once the fault has been tried."""
    tdir = os.path.join(ROOT, "tests")
    if tdir not in sys.path:
        sys.path.insert(0, tdir)
    import sampled_model as SM
    tag, dtype = case["tag"], case["dtype"]
    C, out, B, T, L, H, W = case["C"], case["out"], case["B"], case["T"], case["L"], case["H"], case["W"]
    fed = torch.tensor(case["mask"], dtype=torch.bool)
    params = O.synth_params(C, case["hidden"], case["ks"], L, out_channels=out, seed=case["it"])
    net = pkg.ConvLSTM(C, case["hidden"], case["ks"], L, out_channels=out, compute_dtype=dtype, lon_cyclic=case["cyclic"],
                       feedback=True, return_sequence=True)
    net.load_state_dict(params)
    net = _net(net)
    old_fold, engine.XFOLD = engine.XFOLD, case["fold"]
    try:
        net._engine(torch.device("cuda", torch.cuda.current_device()))
    finally:
        engine.XFOLD = old_fold
    state = [(d[f"h0.{l}"], d[f"c0.{l}"]) for l in range(L)] if case["with_state"] else None
    dev_state = None if state is None else [(_dev(h), _dev(c)) for h, c in state]
    p64 = {k: v.double() for k, v in params.items()}
    kw = dict(h0=[h.double() for h, _ in state], c0=[c.double() for _, c in state]) if state is not None else {}
    X = _dev(d["X"])
    with torch.no_grad():
        pred, seq = net(X, dev_state, free_mask=fed)
        # bit contract: the open-loop pass over the input that holds, where the mask says, the predictions of the step before
        X2 = X.clone()
        sv = seq.view(B, T, out, H, W)
        if bool(fed[:, 0].any()):
            eng = next(iter(net._engines.values()))
            with eng.window(B, T, H, W, False, True) as ws:
                eng.load_state(ws, eng.state_from_tensors(dev_state))
                p0 = eng.head_forward(ws, net.conv.weight, net.conv.bias, slot=0)
        for b in range(B):
            for t in range(T):
                if bool(fed[b, t]):
                    X2[b, t, C - out:] = sv[b, t - 1] if t > 0 else p0[b]
        pred2, seq2 = net(X2, dev_state)
    torch.cuda.synchronize()
    assert torch.equal(seq, seq2) and torch.equal(pred, pred2), (tag, "the masked pass differs from the open loop on the substituted input")
    ref = SM.forward(d["X"].double(), p64, fed, cyclic=case["cyclic"], storage=dtype, **kw)
    w = compare(tag, dtype, dict(pred=pred.cpu(), seq=seq.cpu()), dict(pred=ref["pred"], seq=ref["seq"]), args.only >= 0)
    if not bool(fed[:, 0].any()):
        # (the drawn cotangents get a mean, as in --rollout)
        dseq = d["dseq"] + 0.5 if case["cot"] == "seq" else None
        dpred = d["dpred"] + 0.5 if case["cot"] == "last" else None
        Xg = _dev(d["X"]).requires_grad_(True)
        pred, seq = net(Xg, dev_state, free_mask=fed, feedback_grad=True)
        outs, cots = zip(*[(o, _dev(c)) for o, c in ((pred, dpred), (seq, dseq)) if c is not None])
        torch.autograd.backward(list(outs), list(cots))
        torch.cuda.synchronize()
        fedc = fed.view(B, T, 1, 1, 1).expand(B, T, out, H, W)
        assert not bool(Xg.grad.cpu()[:, :, C - out:][fedc].any()), (tag, "a gradient on the fed channels of a fed image")
        res = dict(pred=pred.detach().cpu(), seq=seq.detach().cpu(), dx=Xg.grad.cpu())
        for k, p in net.named_parameters():
            res["d." + k] = p.grad.cpu()

        def against(mask):
            r = SM.grads(d["X"].double(), p64, mask, case["cyclic"], "f32", dpred, dseq, **kw)
            want = dict(pred=r["pred"], seq=r["seq"], dx=r["dx"])
            for k in p64:
                want["d." + k] = r["params"][k]
            return compare(tag, dtype, res, want, args.only >= 0)
        w = max(w, against(fed))
        any_t = fed.any(dim=0)
        mixed = bool((any_t & ~fed.all(dim=0)).any())
        if args.self_check and mixed and not tried.get("full_mask"):
            first = int(any_t.to(torch.uint8).argmax())
            expect_failure(tag, "the reference feeds every image from the first fed step on", lambda: against(SM.suffix(B, T, first)))
            tried["full_mask"] = True
    worst[dtype] = max(worst[dtype], w)
    print(f"ok   {tag}  worst {w:.2e}", flush=True)


def residual_run(case, d, args, worst, tried):
    """--residual: one case on the device against tests/residual_model.py.  Forward (under no_grad): the fed value rounded to the
    storage type, and the bit contract.  Gradients: f64 under CPU autograd, the fed value rounded to f32 and passed straight
    through.  ``tried`` (--self-check): "no_base" once the fault has been tried."""
    tdir = os.path.join(ROOT, "tests")
    if tdir not in sys.path:
        sys.path.insert(0, tdir)
    import residual_model as RES
    import sampled_model as SM
    tag, dtype = case["tag"], case["dtype"]
    C, out, B, T, L, H, W = case["C"], case["out"], case["B"], case["T"], case["L"], case["H"], case["W"]
    fed = torch.tensor(case["mask"], dtype=torch.bool) if case["mask"] is not None else SM.suffix(B, T, case["fb_from"])
    feed = dict(free_mask=fed) if case["mask"] is not None else dict(free_from=case["fb_from"])
    params = O.synth_params(C, case["hidden"], case["ks"], L, out_channels=out, seed=case["it"])
    net = pkg.ConvLSTM(C, case["hidden"], case["ks"], L, out_channels=out, compute_dtype=dtype, lon_cyclic=case["cyclic"],
                       feedback=True, residual=True, return_sequence=True)
    net.load_state_dict(params)
    net = _net(net)
    old_fold, engine.XFOLD = engine.XFOLD, case["fold"]
    try:
        net._engine(torch.device("cuda", torch.cuda.current_device()))
    finally:
        engine.XFOLD = old_fold
    state = [(d[f"h0.{l}"], d[f"c0.{l}"]) for l in range(L)] if case["with_state"] else None
    dev_state = None if state is None else [(_dev(h), _dev(c)) for h, c in state]
    p64 = {k: v.double() for k, v in params.items()}
    kw = dict(h0=[h.double() for h, _ in state], c0=[c.double() for _, c in state]) if state is not None else {}
    X = _dev(d["X"])
    with torch.no_grad():
        pred, seq = net(X, dev_state, **feed)
        # bit contract: the residual open-loop pass over the input that holds, where fed, the predictions of the step before
        X2 = X.clone()
        sv = seq.view(B, T, out, H, W)
        for b in range(B):
            for t in range(1, T):
                if bool(fed[b, t]):
                    X2[b, t, C - out:] = sv[b, t - 1]
        pred2, seq2 = net(X2, dev_state)
    torch.cuda.synchronize()
    assert torch.equal(seq, seq2) and torch.equal(pred, pred2), (tag, "the residual closed loop differs from the open loop on the substituted input")
    ref = RES.forward(d["X"].double(), p64, fed, cyclic=case["cyclic"], storage=dtype, **kw)
    w = compare(tag, dtype, dict(pred=pred.cpu(), seq=seq.cpu()), dict(pred=ref["pred"], seq=ref["seq"]), args.only >= 0)
    # (the drawn cotangents get a mean, as in --rollout)
    dseq = d["dseq"] + 0.5 if case["cot"] in ("seq", "both") else None
    dpred = d["dpred"] + 0.5 if case["cot"] in ("last", "both") else None
    Xg = _dev(d["X"]).requires_grad_(True)
    pred, seq = net(Xg, dev_state, feedback_grad=True, **feed)
    outs, cots = zip(*[(o, _dev(c)) for o, c in ((pred, dpred), (seq, dseq)) if c is not None])
    torch.autograd.backward(list(outs), list(cots))
    torch.cuda.synchronize()
    fedc = fed.view(B, T, 1, 1, 1).expand(B, T, out, H, W)
    assert not bool(Xg.grad.cpu()[:, :, C - out:][fedc].any()), (tag, "a gradient on the fed channels of a fed image")
    res = dict(pred=pred.detach().cpu(), seq=seq.detach().cpu(), dx=Xg.grad.cpu())
    for k, p in net.named_parameters():
        res["d." + k] = p.grad.cpu()

    def against(model):
        r = model.grads(d["X"].double(), p64, fed, case["cyclic"], "f32", dpred, dseq, **kw)
        want = dict(pred=r["pred"], seq=r["seq"], dx=r["dx"])
        for k in p64:
            want["d." + k] = r["params"][k]
        return compare(tag, dtype, res, want, args.only >= 0)
    w = max(w, against(RES))
    if args.self_check and not tried.get("no_base"):
        expect_failure(tag, "the reference has no base (the non-residual model)", lambda: against(SM))
        tried["no_base"] = True
    worst[dtype] = max(worst[dtype], w)
    print(f"ok   {tag}  worst {w:.2e}", flush=True)


def noise_run(case, d, args, worst, tried):
    """--noise: one case on the device against the CPU oracle on the pre-noised input.  The reference input is built on the host
    by tests/noise_model.py (its own Philox, f64 normals rounded to f32, the float32 update, the storage rounding); the model
    then runs in f64 under CPU autograd (tests/rollout_model.py with nothing fed: the oracle's open loop).  ``tried``
    (--self-check): "clean" once the fault has been tried."""
    tdir = os.path.join(ROOT, "tests")
    if tdir not in sys.path:
        sys.path.insert(0, tdir)
    import noise_model as NM
    import rollout_model as RM
    from nasa_niswan_amd.engine import InputNoise
    tag, dtype = case["tag"], case["dtype"]
    C, out, B, T, L, H, W = case["C"], case["out"], case["B"], case["T"], case["L"], case["H"], case["W"]
    c0, n, sigma, key = case["c0"], case["n"], case["sigma"], case["key"]
    params = O.synth_params(C, case["hidden"], case["ks"], L, out_channels=out, seed=case["it"])
    net = pkg.ConvLSTM(C, case["hidden"], case["ks"], L, out_channels=out, compute_dtype=dtype, lon_cyclic=case["cyclic"],
                       return_sequence=True)
    net.load_state_dict(params)
    net = _net(net)
    old_fold, engine.XFOLD = engine.XFOLD, case["fold"]
    try:
        net._engine(torch.device("cuda", torch.cuda.current_device()))
    finally:
        engine.XFOLD = old_fold
    N = InputNoise(tuple(sigma), channels=(c0, n), **key)
    with torch.no_grad():
        X = _dev(d["X"])
        clean = net(X)
        zero = net(X, input_noise=InputNoise((0.0,) * n, channels=(c0, n), **key))
    assert all(torch.equal(a, b) for a, b in zip(clean, zero)), (tag, "an all-zero std is not the pass without noise")
    dseq, dpred = d["dseq"] + 0.5, d["dpred"] + 0.5
    Xg = _dev(d["X"]).requires_grad_(True)
    pred, seq = net(Xg, input_noise=N)
    torch.autograd.backward([pred, seq], [_dev(dpred), _dev(dseq)])
    torch.cuda.synchronize()
    res = dict(pred=pred.detach().cpu(), seq=seq.detach().cpu(), dx=Xg.grad.cpu())
    for k, p in net.named_parameters():
        res["d." + k] = p.grad.cpu()
    assert any(v != 0 for v in sigma) and not torch.equal(res["pred"], clean[0].cpu()), (tag, "the noise changed nothing")
    p64 = {k: v.double() for k, v in params.items()}
    z = NM.z_images(B, T, n, H, W, **key).astype(np.float32)
    Xn = torch.from_numpy(NM.noisy_input(d["X"].numpy(), z, c0, sigma, dtype == "bf16"))

    def against(x):
        r = RM.grads(x.double(), p64, None, case["cyclic"], "f32", dpred, dseq)
        want = dict(pred=r["pred"], seq=r["seq"], dx=r["dx"])
        for k in p64:
            want["d." + k] = r["params"][k]
        return compare(tag, dtype, res, want, args.only >= 0)
    w = against(Xn)
    if args.self_check and not tried.get("clean"):
        expect_failure(tag, "the reference saw the clean input", lambda: against(d["X"]))
        tried["clean"] = True
    worst[dtype] = max(worst[dtype], w)
    print(f"ok   {tag}  worst {w:.2e}", flush=True)


def ensemble_run(case, lib):
    """one drawn case of nint_ens_accum against tests/ensemble_model.py; returns the worst sample-row error / bound"""
    import ctypes as C
    import math
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import ensemble_model as EM
    finally:
        sys.path.pop(0)
    from oracle import small_audit as SM
    M, N, O, H, W, oy, ox, Hc, Wc = (case[k] for k in ("M", "N", "O", "H", "W", "oy", "ox", "Hc", "Wc"))
    rng = np.random.default_rng([case["it"], M, N])
    if case["integer"]:
        x = rng.integers(-8, 9, (N, M, O, Hc, Wc)).astype(np.float32)
        y = rng.integers(-8, 9, (N, O, Hc, Wc)).astype(np.float32)
        row_w = EM.dyadic_rows(Hc) if case["row_w"] else None
    else:
        x = rng.standard_normal((N, M, O, Hc, Wc)).astype(np.float32)
        y = rng.standard_normal((N, O, Hc, Wc)).astype(np.float32)
        row_w = 0.25 + rng.random(Hc) if case["row_w"] else None
    img = O * H * W
    if case["layout"] == "contiguous":
        buf = np.full((N, M, O, H, W), np.nan, np.float32)
        buf[:, :, :, oy:oy + Hc, ox:ox + Wc] = x
        off, stride = [n * M * img for n in range(N)], img
    else:                                     # sample n = (start n, lead 0) of a roll-out buffer, listed in case["order"]
        T, sp = case["T"], case["spinup"]
        buf = np.full((N * M, T, O, H, W), np.nan, np.float32)
        for n in range(N):
            buf[n * M:(n + 1) * M, sp, :, oy:oy + Hc, ox:ox + Wc] = x[n]
        order = case["order"]
        off, stride = [((n * M) * T + sp) * img for n in order], T * img
        x = x[order]
    nslots, slots = case["nslots"], case["slots"]
    pix0 = rng.integers(-4, 5, (nslots, EM.PIX, O, Hc, Wc)).astype(np.float64)
    hist0 = rng.integers(0, 9, (nslots, O, M + 2)).astype(np.int64)
    ref = EM.sums(x, y, slots, nslots, row_w, pix0, hist0)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    bd, yd, rw, pix, hist = dev(buf), dev(y), dev(row_w), dev(pix0), dev(hist0)
    nb = lib.nint_ens_scratch_bytes(N, M, O, Hc, Wc)
    sample = torch.full((N, O, EM.SAMPLE), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((N, O, Hc, Wc), float("nan"), device="cuda")
    rc = lib.nint_ens_accum(P(bd), (C.c_int64 * N)(*off), stride, M, P(yd), (C.c_int32 * N)(*slots), nslots, P(rw), P(pix), P(sample),
                            P(hist), P(mean), P(scratch), nb, N, O, H, W, oy, ox, Hc, Wc, None)
    assert rc == 0, (case["tag"], rc)
    torch.cuda.synchronize()
    SM.check_equal(pix.cpu().numpy(), ref["pix"], case["tag"] + ": pix")
    SM.check_equal(hist.cpu().numpy(), ref["rank_hist"], case["tag"] + ": rank_hist")
    SM.check_equal(mean.cpu().numpy(), ref["mean"], case["tag"] + ": mean_out")
    got = sample.cpu().numpy()
    if case["integer"]:
        SM.check_equal(got, ref["sample"], case["tag"] + ": sample")
        return 0.0
    # a row is a tree over the crop's f64 addends (the model's own terms, bit for bit the kernel's): any order of Hc * Wc terms
    st, worst = ref["sample_terms"], 0.0
    g = SM.gamma(max(Hc * Wc - 1, 0), SM.U64)
    for n in range(N):
        for o in range(O):
            for k in range(EM.SAMPLE):
                terms = st[k, n, o].reshape(-1).tolist()
                err, bound = abs(math.fsum(terms + [-float(got[n, o, k])])), g * math.fsum(abs(v) for v in terms)
                assert math.isfinite(got[n, o, k]) and err <= bound, (case["tag"], (n, o, k), got[n, o, k], err, bound)
                worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst


def ensemble_main(args):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import nasa_niswan_amd as pkg_
    lib = pkg_.load_library()
    t_start, worst = time.time(), 0.0
    for it in range(args.n):
        if args.only >= 0 and it != args.only:           # (a stream per case: the replayed case needs none of the others)
            continue
        case = draw_case(case_rng(args.seed, "ensemble", it), it, "ensemble")
        w = ensemble_run(case, lib)
        worst = max(worst, w)
        print(f"ok   {case['tag']}  rows {w:.2e} of the bound", flush=True)
    print(f"wall {time.time() - t_start:.1f} s")
    print(f"{args.n} shapes ok; worst sample-row error {worst:.2e} of the any-order bound")


def main(argv=None):
    args = parse(argv)
    new = args.mode in ALL_STREAM_MODES + SAMPLED_MODES + RESIDUAL_MODES + NOISE_MODES
    if args.list:
        for case in draw_cases(args.seed, args.n, args.mode, args.big, args.wide):
            print(json.dumps(case), flush=True)
        return
    if args.mode == "ensemble":
        return ensemble_main(args)
    _load()
    t_start = time.time()
    rng = np.random.default_rng(args.seed)
    worst = {"f32": 0.0, "bf16": 0.0}
    tried = {}
    for it in range(args.n):
        if new:
            if args.only >= 0 and it != args.only:
                continue
            rng = case_rng(args.seed, args.mode, it)
        case = draw_case(rng, it, args.mode, args.big, args.wide)
        if args.only >= 0 and not new:
            if it < args.only:                   # consume what the case would have drawn
                for _, sh in case["draws"]:
                    rng.standard_normal(sh)
                continue
            if it > args.only:
                break
        if args.only >= 0 and args.force_wave is not None:
            case["wave"] = args.force_wave
            case["tag"] = case["tag"].replace(f"wave={WAVES[it % 7]}", f"wave={args.force_wave}")
        if args.only >= 0 and args.force_dtype is not None:
            case["tag"] = case["tag"].replace(f" {case['dtype']} ", f" {args.force_dtype} ")
            case["dtype"] = args.force_dtype
        engine.FORCE_WAVE, engine.FORCE_TILE_ROWS, engine.FORCE_WIDE = case["wave"], case["rows"], case["wide"]
        try:
            d = draw_data(rng, case)
            with guarded_case(args, case, tried):
                if args.mode == "closed_loop":
                    closed_loop_run(case, d, args, worst)
                elif args.mode == "rollout":
                    rollout_run(case, d, args, worst)
                elif args.mode == "sampled":
                    sampled_run(case, d, args, worst, tried)
                elif args.mode == "residual":
                    residual_run(case, d, args, worst, tried)
                elif args.mode == "noise":
                    noise_run(case, d, args, worst, tried)
                elif new:
                    run_new(case, d, args, worst, tried)
                else:
                    run_old(case, d, args, worst)
        finally:
            engine.FORCE_WAVE, engine.FORCE_TILE_ROWS, engine.FORCE_WIDE = None, 0, 0
    if args.self_check:
        want = {"state": ["zero_c0"], "train_opts": ["truncate", "drop"], "stateful": ["reset"], "finetune": ["no_decay", "unfrozen"],
                "sampled": ["full_mask"], "residual": ["no_base"], "noise": ["clean"]}[args.mode]
        missing = [f for f in want if not tried.get(f)]
        if missing:
            raise SystemExit(f"SELF-CHECK INCOMPLETE: no drawn case to try {missing} on (raise --n or change the seed)")
    if args.guard_self_check and not tried.get("guard"):
        raise SystemExit("SELF-CHECK INCOMPLETE: no case passed, so no guard byte was flipped")
    if args.guarded:
        print(f"guarded: {tried.get('arenas', 0)} allocations checked, every guard byte intact")
    print(f"wall {time.time() - t_start:.1f} s")
    print(f"{args.n} shapes ok; worst f32 max-rel {worst['f32']:.2e}, worst bf16 rel-L2 {worst['bf16']:.2e}")


if __name__ == "__main__":
    main()
