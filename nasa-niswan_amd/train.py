#!/usr/bin/env python3
"""Fit loop with the reference's command line (reference train.py:148-227) around the fused
MI355X step.  Same flags, same artefacts (`configurations.json`, `logger.npy`,
`epoch-XXX/generator.pth.tar`, per-epoch print), same schedule (Adam betas (0.5,0.999), StepLR
stepped once per epoch before validation, checkpoint every 10 epochs); the per-batch
`loss.item()` / sklearn R2 host syncs (train.py:113-114) are replaced by device accumulators read
once per epoch.  Added flags: --dtype, --levels, --grid, --synthetic-steps, --pad-mode, --f32-inputs,
--static-channels, --sequence-loss, --test-skill, --lat-weighted-loss, --loss-weights, --clip-grad-norm,
--skip-nonfinite-steps, --stateful, --bptt-segments, --accumulate-steps, --loss-mix, --huber-delta, --output-weights,
--spinup-steps, --rollout-from, --sampling-prob, --sampling-ramp-epochs, --sampling-seed, --residual-head,
--tracer-noise, --noise-seed, --train-ensemble, --train-feedback-noise, --crps-alpha, --test-spectrum.

The data path is on the device too: by default every batch is written by ONE launch of the
fuse / z-score / halo-pad kernel straight into the model's bf16 input slab (dataset.slab_batch);
--f32-inputs materialises the reference's (B,T,C,Hp,Wp) f32 tensor first (dataset.device_batch).

    python nasa-niswan_amd/train.py --model LSTM-demo --in-channels 5 --sequence-length 12 \
        --input-size 100 154 --batch-size 8 --num-epochs 2 --snapshot-dir /tmp/snap
    python -m torch.distributed.run --nproc-per-node 8 nasa-niswan_amd/train.py ...   # batch-sharded DDP
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_arguments(argv=None, MODEL='LSTM-00', SPECIES='bcb', LEARNING_RATE=1.0E-04, DATASET='E33OMA90D', IN_CHANNELS=5,
                  HIDDEN_CHANNELS=(64, 32, 16), KERNEL_SIZE=(5, 3, 3), NUM_LAYERS=3, SEQUENCE_LENGTH=48, TRANSFORM=False,
                  NUM_EPOCHS=50, INPUT_SIZE=(100, 154), BATCH_SIZE=4, NUM_WORKERS=1, SCHEDULER_CONFIG=(10, 0.9),
                  BETAS=(0.5, 0.999), USE_CHECKPOINT=False, SNAPSHOT_DIR='./', RESTORE_FROM='./'):
    """Flag names, types and defaults follow reference train.py:148-208 (INPUT_SIZE defaults to the
    LSTM launcher value instead of the UNet 256x256, and MODEL to an LSTM name: only the LSTM
    family is in scope)."""
    parser = argparse.ArgumentParser(description=f"Training {MODEL} on E33OMA.")
    parser.add_argument("--model", type=str, default=MODEL)
    parser.add_argument("--species", type=str, default=SPECIES)
    parser.add_argument("--learning-rate", type=float, default=LEARNING_RATE)
    parser.add_argument("--dataset", type=str, default=DATASET)
    parser.add_argument("--in-channels", type=int, default=IN_CHANNELS)
    parser.add_argument("--hidden-channels", nargs='+', type=int, default=HIDDEN_CHANNELS)
    parser.add_argument("--kernel-size", nargs='+', type=int, default=KERNEL_SIZE)
    parser.add_argument("--num-layers", type=int, default=NUM_LAYERS)
    parser.add_argument("--sequence-length", type=int, default=SEQUENCE_LENGTH)
    parser.add_argument("--transform", action="store_true", default=TRANSFORM)     # parsed, never read here: the reference passes it to the UNet datasets only (train.py:52-57), its CRNN datasets take no transform (train.py:59-64)
    parser.add_argument("--num-epochs", type=int, default=NUM_EPOCHS)
    parser.add_argument("--input-size", nargs=2, type=int, default=INPUT_SIZE)
    parser.add_argument("--batch-size", type=int, default=BATCH_SIZE)
    parser.add_argument("--num-workers", type=int, default=NUM_WORKERS)     # parsed, unused -- as in the reference (train.py:67)
    parser.add_argument("--scheduler-config", nargs=2, type=float, default=SCHEDULER_CONFIG)
    parser.add_argument("--betas", nargs=2, type=float, default=BETAS)
    parser.add_argument("--use-checkpoint", action="store_true", default=USE_CHECKPOINT)
    parser.add_argument("--snapshot-dir", type=str, default=SNAPSHOT_DIR)
    parser.add_argument("--restore-from", type=str, default=RESTORE_FROM)
    # extensions
    parser.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "f32"])
    parser.add_argument("--levels", type=int, default=1, help="vertical levels fused as channels (C = 3L+2)")
    parser.add_argument("--static-channels", type=int, default=0,
                        help="time-invariant static-attribute channels appended after the dynamic ones (reference "
                             "dataset.py:100-122; C = 3L+2+S, so the reference launcher's --in-channels 8 is S = 3); 0: none, "
                             "and an --in-channels other than 3L+2 means that many generic fields")
    parser.add_argument("--synthetic-steps", type=int, default=480, help="length of the synthetic record")
    parser.add_argument("--pad-mode", type=str, default="reference", choices=["reference", "reflect"])
    parser.add_argument("--grid", nargs=2, type=int, default=(90, 144),
                        help="un-padded lat x lon grid of the synthetic record; the loss crop is (input-size - grid)/2 "
                             "(the reference hard-codes 90x144 and halo 5, train.py:102)")
    parser.add_argument("--f32-inputs", action="store_true",
                        help="materialise X as the reference's f32 (B,T,C,Hp,Wp) tensor instead of writing the input slab directly")
    parser.add_argument("--sequence-loss", action="store_true",
                        help="sequence-to-sequence supervision: the target is the tracer at every step of the window and the loss "
                             "(training and validation) runs over the head's output at every step, not the last one alone")
    parser.add_argument("--test-skill", action="store_true",
                        help="after the last epoch rank 0 evaluates the 'test' period on the device (inference.evaluate_skill: R2 per "
                             "window and per grid cell, rmse, bias, time means, cos-latitude weighted means; test.ipynb's evaluation "
                             "cells) and writes the report's arrays to skill.npz in --snapshot-dir")
    parser.add_argument("--lat-weighted-loss", action="store_true",
                        help="weight the loss (training, and the validation R2V) by cos(latitude) of the --grid rows, the area of a "
                             "cell on the lat-lon grid -- what --test-skill's weighted means report")
    parser.add_argument("--loss-weights", type=str, default=None, metavar="FILE.npy",
                        help="a --grid shaped (H, W) map of non-negative loss weights, 0 = leave the cell out (missing data, other "
                             "regions); with --lat-weighted-loss the two are multiplied")
    parser.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                        help="clip the global L2 norm of the gradient to X before the Adam step (torch.nn.utils.clip_grad_norm_), "
                             "on the device; under DDP the norm of the all-reduced mean gradient")
    parser.add_argument("--skip-nonfinite-steps", action="store_true",
                        help="drop an optimizer step whose gradient holds a NaN or inf (weights, moments and step count untouched)")
    parser.add_argument("--stateful", action="store_true",
                        help="truncated BPTT with carried state: every batch lane walks its own contiguous part of the training "
                             "period in consecutive NON-overlapping chunks of --sequence-length steps (dataset.stateful_schedule, "
                             "no shuffle), each chunk starting from the state the lane's previous chunk ended in; the state is reset "
                             "at the start of every epoch.  A record step is then run once per epoch, not --sequence-length times")
    parser.add_argument("--bptt-segments", type=int, default=None, metavar="N",
                        help="checkpointed BPTT: run every window as N equal segments of --sequence-length / N steps through one "
                             "training workspace of that length, recomputing each segment's forward pass before its backward: the "
                             "gradient of the whole window with 1/N of the per-step slabs resident, for (N-1)/N of a forward "
                             "pass more.  N must divide --sequence-length; not with --sequence-loss")
    parser.add_argument("--accumulate-steps", type=int, default=1, metavar="K",
                        help="gradient accumulation: one optimizer step (and one all-reduce) per K batches, on their mean gradient; "
                             "a group left unfinished at the end of an epoch goes on in the next")
    parser.add_argument("--loss-mix", nargs=3, type=float, default=(1.0, 1.0, 0.0), metavar=("MSE", "L1", "HUBER"),
                        help="coefficients of the MSE, L1 and Huber terms of the loss (training and validation); a coefficient of "
                             "0 takes its term out.  The default is the reference's MSELoss + L1Loss")
    parser.add_argument("--huber-delta", type=float, default=1.0, metavar="D",
                        help="threshold of the Huber term (torch.nn.HuberLoss), in the target's z-score units")
    parser.add_argument("--output-weights", type=str, default=None, metavar="FILE.npy",
                        help="a vector of --levels non-negative loss weights, one per output; 0 = leave the output out (its "
                             "targets may be NaN)")
    parser.add_argument("--spinup-steps", type=int, default=0, metavar="K",
                        help="with --sequence-loss: the first K steps of every window (spin-up from the zero state) carry no "
                             "loss; K < --sequence-length")
    parser.add_argument("--freeze-layers", type=int, default=0, metavar="N",
                        help="fine-tuning: the first N ConvLSTM layers keep their weights; the backward pass stops above them "
                             "and pays nothing for them.  N = --num-layers trains the head alone")
    parser.add_argument("--weight-decay", type=float, default=0.0, metavar="X",
                        help="decoupled weight decay (torch.optim.AdamW) on the trained weights; biases get none")
    parser.add_argument("--layer-lr-scale", nargs='+', type=float, default=None, metavar="S",
                        help="one factor on --learning-rate per ConvLSTM layer, bottom first (smaller lower down); the head "
                             "takes the last one, or one more of its own")
    parser.add_argument("--cyclic-longitude", action="store_true",
                        help="the model treats longitude as periodic: column 0 and column W-1 of its grid are neighbours in every "
                             "convolution (ConvLSTM(lon_cyclic=True)), so the input needs no longitude halo and the loss no "
                             "longitude crop.  The width of --input-size must equal the width of --grid")
    parser.add_argument("--tracer-input", action="store_true",
                        help="the tracer of the step before joins the input as its last --levels channels (dataset tracer_input; "
                             "--in-channels counts the other channels, the model gets --in-channels + --levels): teacher-forced "
                             "training of a model that can run on its own prediction (ConvLSTM(feedback=True)).  Needs a grid "
                             "without a data halo: --input-size equal to --grid, usually with --cyclic-longitude")
    parser.add_argument("--test-rollout", type=int, default=0, metavar="HORIZON",
                        help="with --tracer-input: after the test pass rank 0 runs the model closed loop over the 'test' period "
                             "(inference.rollout_skill) and prints R2 per lead time 0 .. HORIZON-1")
    parser.add_argument("--ensemble-members", type=int, default=None, metavar="M",
                        help="with --test-rollout: also run every roll-out window as an ensemble of M members in [2, 64] "
                             "(inference.rollout_ensemble) and print RMSE of the ensemble mean, spread, their ratio, CRPS, bias "
                             "and R2 per lead time")
    parser.add_argument("--ensemble-noise", type=float, default=None, metavar="S",
                        help="with --ensemble-members: std of the members' initial-condition noise on the tracer channels of the "
                             "spin-up, z-score units (default 0.05)")
    parser.add_argument("--ensemble-feedback-noise", type=float, default=None, metavar="S",
                        help="with --ensemble-members: std of the noise added to every fed-back value (default 0)")
    parser.add_argument("--ensemble-seed", type=int, default=None, metavar="K", help="with --ensemble-members: the noise seed (default 0)")
    parser.add_argument("--test-spectrum", action="store_true",
                        help="with --test-rollout: also accumulate the zonal power spectra of the roll-out (and, with "
                             "--ensemble-members, of the ensemble) against the target's per lead time on the device "
                             "(inference.SpectrumAccumulator), print the small-scale table and write rollout_spectrum.npz")
    parser.add_argument("--rollout-spinup", type=int, default=None, metavar="K",
                        help="steps of analysis input before the free run of --test-rollout (default: --sequence-length)")
    parser.add_argument("--rollout-from", type=int, default=None, metavar="K",
                        help="with --tracer-input: ROLL-OUT TRAINING -- from step K >= 1 of every training window the model runs on "
                             "its own prediction (the tracer channels of steps >= K are the head's output of the step before) and "
                             "the loss is back-propagated through the fed-back prediction (FusedTrainer(rollout_from=K)).  "
                             "Validation stays teacher-forced.  Not with --stateful, --bptt-segments, --freeze-layers")
    parser.add_argument("--sampling-prob", type=float, default=None, metavar="P",
                        help="with --rollout-from K: SCHEDULED SAMPLING -- per training step, per sample and per window step >= K a coin "
                             "of bias P decides whether the sample sees its own last prediction or the analysis "
                             "(FusedTrainer(sampling_prob=P)).  1 is plain --rollout-from; 0 is teacher forcing")
    parser.add_argument("--sampling-ramp-epochs", type=int, default=0, metavar="E",
                        help="with --sampling-prob P: the probability rises linearly from 0 to P over the first E epochs (set once "
                             "per epoch, printed with the epoch line); 0: P from the first epoch")
    parser.add_argument("--sampling-seed", type=int, default=0, help="the coin's seed (each rank draws from seed + rank)")
    parser.add_argument("--residual-head", action="store_true",
                        help="with --tracer-input: the head predicts the tracer's TENDENCY -- every step's prediction is the tracer "
                             "the step was given (its last --levels input channels) plus the head's output "
                             "(ConvLSTM(residual=True)); stored with the snapshot's arguments.  Resuming a checkpoint that was "
                             "trained without it is refused unless --reset-optimizer asks for fine-tuning")
    parser.add_argument("--tracer-noise", type=float, default=None, metavar="STD",
                        help="with --tracer-input: every training step shows the model its tracer channels with Gaussian noise of "
                             "this standard deviation (z-score units) added, drawn on the device (FusedTrainer(input_noise=STD)); "
                             "validation and test see clean inputs.  A resumed run restarts the draw counter at 0")
    parser.add_argument("--noise-seed", type=int, default=0, help="the seed of --tracer-noise (the same on every rank)")
    parser.add_argument("--train-ensemble", type=int, default=None, metavar="M",
                        help="with --rollout-from: ENSEMBLE TRAINING -- every sample runs as M member lanes in [2, 64] that differ by "
                             "the seeded noise alone (--tracer-noise on the input, --train-feedback-noise on every fed-back value), "
                             "and the loss is the almost-fair CRPS over the members (FusedTrainer(ensemble_members=M)).  "
                             "--batch-size counts samples: a step runs batch * M lanes.  --output-weights and --spinup-steps "
                             "weight it; --loss-mix / --huber-delta are refused with it")
    parser.add_argument("--train-feedback-noise", type=float, default=None, metavar="S",
                        help="with --train-ensemble: std (z-score units) of the noise added to every fed-back value in training "
                             "(default 0.05 when --tracer-noise is not given, else 0)")
    parser.add_argument("--crps-alpha", type=float, default=None, metavar="A",
                        help="with --train-ensemble: 1 the fair CRPS, 0 the plain one, between them the almost-fair mix (default 0.95)")
    parser.add_argument("--reset-optimizer", action="store_true",
                        help="with --use-checkpoint: load the weights of --restore-from only and start the optimizer afresh "
                             "(the fine-tuning entry point; without it an optimizer state of other param groups is an error)")
    args = parser.parse_args(argv)
    if not 0 <= args.freeze_layers <= args.num_layers:
        parser.error(f"--freeze-layers must be in [0, --num-layers = {args.num_layers}]")
    if args.layer_lr_scale is not None and len(args.layer_lr_scale) not in (args.num_layers, args.num_layers + 1):
        parser.error(f"--layer-lr-scale takes {args.num_layers} factors (one per layer) or {args.num_layers + 1} (the head's last)")
    if args.cyclic_longitude and int(args.input_size[1]) != int(args.grid[1]):
        parser.error(f"--cyclic-longitude: the model wraps at the edge of its own grid, so --input-size's width "
                     f"({args.input_size[1]}) must be --grid's ({args.grid[1]}): no longitude halo")
    if args.tracer_input and tuple(int(v) for v in args.input_size) != tuple(int(v) for v in args.grid):
        parser.error(f"--tracer-input: a fed-back prediction has no value in a data halo, so --input-size {tuple(args.input_size)} "
                     f"must equal --grid {tuple(args.grid)}; pass --cyclic-longitude for periodic longitude instead of the halo")
    if args.tracer_input and args.static_channels:
        parser.error("--tracer-input and --static-channels both claim the last input channels; they are not combined")
    if args.test_rollout < 0 or (args.test_rollout > 0 and not args.tracer_input):
        parser.error("--test-rollout takes a horizon >= 1 and needs --tracer-input")
    if args.rollout_from is not None:
        if not args.tracer_input:
            parser.error("--rollout-from needs --tracer-input: the model must have feedback channels to run on its own prediction")
        if args.rollout_from < 1:
            parser.error("--rollout-from must be >= 1: step 0 has no prediction to be fed")
        if args.stateful or (args.bptt_segments or 1) > 1 or args.freeze_layers > 0:
            parser.error("--rollout-from is not combined with --stateful, --bptt-segments or --freeze-layers")
    if args.residual_head and not args.tracer_input:
        parser.error("--residual-head needs --tracer-input: the increment is added to the tracer of the step before, the model's "
                     "feedback channels")
    if args.residual_head and args.use_checkpoint and not args.reset_optimizer:
        was = checkpoint_residual_head(args.restore_from)
        if was is False:
            parser.error(f"--residual-head: the checkpoint under {args.restore_from} was trained without it (its head predicts the "
                         "state, not the increment, and its optimizer moments belong to that head); pass --reset-optimizer to "
                         "fine-tune its weights as a residual model")
    if args.tracer_noise is not None:
        if not args.tracer_input:
            parser.error("--tracer-noise needs --tracer-input: the noise is added to the tracer channels of the input")
        if not 0.0 <= args.tracer_noise < float("inf"):
            parser.error("--tracer-noise must be a finite standard deviation >= 0")
    if args.noise_seed < 0:
        parser.error("--noise-seed must be >= 0")
    if args.sampling_prob is not None:
        if args.rollout_from is None:
            parser.error("--sampling-prob needs --rollout-from: the coin is thrown for the steps from --rollout-from on")
        if not 0.0 <= args.sampling_prob <= 1.0:
            parser.error("--sampling-prob must be a probability in [0, 1]")
    if args.sampling_ramp_epochs < 0 or (args.sampling_ramp_epochs > 0 and args.sampling_prob is None):
        parser.error("--sampling-ramp-epochs takes a number of epochs >= 0 and needs --sampling-prob")
    if args.rollout_spinup is None:
        args.rollout_spinup = args.sequence_length
    if args.train_ensemble is None:
        for name, v in (("--train-feedback-noise", args.train_feedback_noise), ("--crps-alpha", args.crps_alpha)):
            if v is not None:
                parser.error(f"{name} needs --train-ensemble")
    else:
        if args.rollout_from is None:
            parser.error("--train-ensemble needs --rollout-from: the members differ through the closed loop")
        if not 2 <= args.train_ensemble <= 64:
            parser.error("--train-ensemble must be in [2, 64]")
        if args.sampling_prob is not None:
            parser.error("--train-ensemble is not combined with --sampling-prob")
        if tuple(float(v) for v in args.loss_mix) != (1.0, 1.0, 0.0):
            parser.error("--train-ensemble trains the CRPS: --loss-mix is refused with it")
        if args.train_feedback_noise is None:
            args.train_feedback_noise = 0.0 if args.tracer_noise else 0.05
        if not 0.0 <= args.train_feedback_noise < float("inf"):
            parser.error("--train-feedback-noise must be a finite standard deviation >= 0")
        if args.train_feedback_noise == 0.0 and not args.tracer_noise:
            parser.error("--train-feedback-noise and --tracer-noise are both 0: the members would be identical")
        args.crps_alpha = 0.95 if args.crps_alpha is None else args.crps_alpha
        if not 0.0 <= args.crps_alpha <= 1.0:
            parser.error("--crps-alpha must lie in [0, 1]")
    ens = {"--ensemble-members": args.ensemble_members, "--ensemble-noise": args.ensemble_noise,
           "--ensemble-feedback-noise": args.ensemble_feedback_noise, "--ensemble-seed": args.ensemble_seed}
    given = [k for k, v in ens.items() if v is not None]
    if given and not args.test_rollout:
        parser.error(f"{given[0]} needs --test-rollout: the ensemble runs the roll-out's windows")
    if given and args.ensemble_members is None:
        parser.error(f"{given[0]} needs --ensemble-members")
    if args.ensemble_members is not None:
        if not 2 <= args.ensemble_members <= 64:
            parser.error("--ensemble-members must be in [2, 64]")
        args.ensemble_noise = 0.05 if args.ensemble_noise is None else args.ensemble_noise
        args.ensemble_feedback_noise = 0.0 if args.ensemble_feedback_noise is None else args.ensemble_feedback_noise
        args.ensemble_seed = 0 if args.ensemble_seed is None else args.ensemble_seed
        for name, v in (("--ensemble-noise", args.ensemble_noise), ("--ensemble-feedback-noise", args.ensemble_feedback_noise)):
            if not 0.0 <= v < float("inf"):
                parser.error(f"{name} must be a finite standard deviation >= 0")
        if args.ensemble_noise == 0.0 and args.ensemble_feedback_noise == 0.0:
            parser.error("--ensemble-noise and --ensemble-feedback-noise are both 0: the ensemble would have no spread")
        if args.ensemble_seed < 0:
            parser.error("--ensemble-seed must be >= 0")
    if args.test_spectrum and not args.test_rollout:
        parser.error("--test-spectrum needs --test-rollout: the spectra are those of the roll-out's windows")
    if args.test_rollout > 0 and args.rollout_spinup < 1:
        parser.error("--rollout-spinup must be >= 1")
    if args.spinup_steps < 0:
        parser.error("--spinup-steps must be >= 0")
    if args.spinup_steps > 0 and not args.sequence_loss:
        parser.error("--spinup-steps needs --sequence-loss: the last-step loss has no spin-up steps to drop")
    if args.spinup_steps >= args.sequence_length:
        parser.error(f"--spinup-steps {args.spinup_steps} leaves no step of the --sequence-length {args.sequence_length} window")
    rank = int(os.environ.get("RANK", "0"))
    if rank == 0:
        os.makedirs(args.snapshot_dir, exist_ok=True)
        print('Working Directory:', args.snapshot_dir)
        with open(os.path.join(args.snapshot_dir, 'configurations.json'), "w") as f:     # train.py:221-225
            json.dump(vars(args), f, indent=4)
    return args


def checkpoint_residual_head(restore_from: str):
    """Whether the run that wrote the checkpoint directory ``restore_from`` had --residual-head, from the configurations.json
    stored with the snapshot (in the directory itself or the one above it: checkpoints lie in epoch-NNN below --snapshot-dir);
    None where no such file is found.  A run from before the flag existed was trained without it."""
    for d in (restore_from, os.path.dirname(os.path.abspath(restore_from))):
        path = os.path.join(d, 'configurations.json')
        if os.path.isfile(path):
            with open(path) as f:
                return bool(json.load(f).get('residual_head', False))
    return None


def sampling_prob_of(epoch: int, P, ramp_epochs: int):
    """the coin's bias during epoch `epoch` (0-based): linear from 0 to P over the first `ramp_epochs` epochs, P from then on
    (and from the first epoch without a ramp); None without --sampling-prob"""
    if P is None:
        return None
    return float(P) if ramp_epochs <= 0 else float(P) * min(epoch / ramp_epochs, 1.0)


def build_loss_spec(args):
    """The loss.LossSpec of the loss flags, or None when none of them changes the reference's MSE + L1 (the trainer then runs
    the entries it has always run).  Built the same way on every rank: a spec is not broadcast."""
    mix = tuple(float(v) for v in args.loss_mix)
    if mix == (1.0, 1.0, 0.0) and not args.output_weights and not args.spinup_steps and not args.train_ensemble:
        return None
    from nasa_niswan_amd.loss import EnsembleLoss, LossSpec
    ow = None
    if args.output_weights:
        ow = np.load(args.output_weights)
        if ow.shape != (args.levels,):
            raise SystemExit(f"--output-weights {args.output_weights}: shape {ow.shape}, expected one weight per output {(args.levels,)}")
    sw = None
    if args.spinup_steps:
        sw = np.ones(args.sequence_length, np.float32)
        sw[:args.spinup_steps] = 0.0
    try:
        if args.train_ensemble:          # the same weights on the CRPS (FusedTrainer(ensemble_loss=...))
            return EnsembleLoss(args.crps_alpha, output_weights=ow, step_weights=sw)
        return LossSpec(mix[0], mix[1], mix[2], args.huber_delta, output_weights=ow, step_weights=sw)
    except ValueError as e:
        raise SystemExit(f"loss flags: {e}")


def main(args):
    since = time.time()
    import torch.distributed as dist
    import torch.optim as optim
    import nasa_niswan_amd as pkg
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN, stateful_schedule
    from nasa_niswan_amd.loss import cos_latitude_weights, grid_latitudes
    from nasa_niswan_amd.trainer import FusedTrainer
    from nasa_niswan_amd.utils import load_checkpoint, save_checkpoint, seed, shard_indices

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs an MI355X: the hot path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    if rank == 0:
        print(f"{args.model} is deployed on {torch.cuda.get_device_name(local_rank)}")     # train.py:29
    seed(0)                                                                                 # train.py:32
    if args.model.split('-')[0] != 'LSTM':
        raise SystemExit("only the LSTM family (ConvLSTM) is in scope of this build")
    out_ch = args.levels
    in_ch = args.in_channels + (args.levels if args.tracer_input else 0)      # the tracer of the step before: --levels more channels
    generator = pkg.ConvLSTM(in_ch, list(args.hidden_channels), list(args.kernel_size), args.num_layers,
                             out_channels=out_ch, compute_dtype=args.dtype,
                             lon_cyclic=args.cyclic_longitude, feedback=args.tracer_input,
                             residual=args.residual_head).to(dev)                                   # train.py:48
    H, W = (int(v) for v in args.grid)
    if args.input_size[0] < H or args.input_size[1] < W:
        raise SystemExit(f"--input-size {tuple(args.input_size)} is smaller than --grid {(H, W)}: the model runs on the "
                         "grid plus its halo (launcher.sh:24)")
    halo = ((args.input_size[0] - H) // 2, (args.input_size[1] - W) // 2)                    # 5,5 in the reference (train.py:102)
    ds_kw = dict(species=args.species, padding=tuple(args.input_size), in_channels=in_ch, tracer_input=args.tracer_input,
                 sequence_length=args.sequence_length, levels=args.levels, n_steps=args.synthetic_steps,
                 grid=(H, W), pad_mode=args.pad_mode, device=dev, static_channels=args.static_channels,
                 sequence_targets=args.sequence_loss)
    train_dataset = SyntheticE33OMA_CRNN('train', **ds_kw)                                   # train.py:63-65
    val_dataset = SyntheticE33OMA_CRNN('val', **ds_kw)
    get_batch = (lambda ds, idx: ds.device_batch(idx)) if args.f32_inputs else (lambda ds, idx: ds.slab_batch(idx))

    # the loss weights, built the same way on every rank (they are not broadcast)
    loss_weights = None
    if args.lat_weighted_loss:
        loss_weights = cos_latitude_weights(grid_latitudes(H), W)
    if args.loss_weights:
        m = np.load(args.loss_weights)
        if m.shape != (H, W):
            raise SystemExit(f"--loss-weights {args.loss_weights}: shape {m.shape}, expected the --grid {(H, W)}")
        loss_weights = m if loss_weights is None else (loss_weights.astype(np.float64) * m).astype(np.float32)
    trainer = FusedTrainer(generator, lr=args.learning_rate, betas=tuple(args.betas), halo=halo,        # train.py:71
                           sequence_loss=args.sequence_loss, loss_weights=loss_weights,
                           max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite_steps, stateful=args.stateful,
                           bptt_segments=args.bptt_segments, accumulate_steps=args.accumulate_steps,
                           **(dict(ensemble_members=args.train_ensemble, feedback_noise=args.train_feedback_noise,
                                   ensemble_loss=build_loss_spec(args)) if args.train_ensemble else dict(loss=build_loss_spec(args))),
                           freeze_layers=args.freeze_layers, weight_decay=args.weight_decay, layer_lr_scale=args.layer_lr_scale,
                           rollout_from=args.rollout_from, sampling_prob=args.sampling_prob, sampling_seed=args.sampling_seed,
                           input_noise=args.tracer_noise, noise_seed=args.noise_seed)
    if args.stateful:
        # one schedule of world * batch lanes, the same every epoch; each rank takes its own columns and carries its own state
        sched, dropped = stateful_schedule(len(train_dataset), args.sequence_length, world * args.batch_size)
        sched = sched[:, rank * args.batch_size:(rank + 1) * args.batch_size]
        if rank == 0:
            print(f"Stateful schedule: {sched.shape[0]} steps of {world * args.batch_size} lanes x {args.sequence_length} record "
                  f"steps per epoch, {dropped} trailing windows dropped")
    guarded = args.clip_grad_norm is not None or args.skip_nonfinite_steps
    optimizer = trainer.optimizer
    scheduler = optim.lr_scheduler.StepLR(optimizer, step_size=int(args.scheduler_config[0]),
                                          gamma=args.scheduler_config[1])                   # train.py:72
    if args.use_checkpoint:
        load_checkpoint(f'{args.restore_from}/generator.pth.tar', generator, optimizer, args.learning_rate,
                        map_location=dev, reset_optimizer=args.reset_optimizer)             # train.py:77-78
    logger = {'MSELoss': [], 'r2_score': [], 'r2_score_val': [], 'first_step_loss': None, 'train_samples_per_s': []}
    M_ens = args.train_ensemble or 0
    if M_ens:
        logger['crps'], logger['spread_skill'] = [], []
    for epoch in range(1, args.num_epochs + 1):                                              # train.py:82
        generator.train()
        trainer.reset_stats()
        p_epoch = sampling_prob_of(epoch - 1, args.sampling_prob, args.sampling_ramp_epochs)
        if p_epoch is not None:
            trainer.set_sampling_prob(p_epoch)                                               # once per epoch
        torch.cuda.synchronize()
        t_epoch, n_epoch = time.time(), 0
        if args.stateful:
            trainer.reset_state()                                                            # every lane starts the record anew
        batches = sched if args.stateful else shard_indices(len(train_dataset), epoch, rank, world, args.batch_size)   # train.py:89
        for idx in batches:
            if M_ens:                    # every index M times: lane n*M + m; the target of a sample is taken once
                X, y = get_batch(train_dataset, np.repeat(np.asarray(idx), M_ens))
                y = y[::M_ens].contiguous()
            else:
                X, y = get_batch(train_dataset, idx)                                         # preproc on device
            loss = trainer.step(X, y)                                                        # train.py:96-110
            n_epoch += len(idx)
            if logger['first_step_loss'] is None:
                logger['first_step_loss'] = float(loss)
        loss_e, r2_e = trainer.epoch_stats()                                                 # one host read per epoch (syncs)
        gstats = trainer.grad_stats(reset=True) if guarded else None                         # (and one more with the guard on)
        estats = trainer.ensemble_stats(reset=True) if M_ens else None                       # (before evaluate() adds to the stats)
        if M_ens:
            logger['crps'].append(estats['crps'])
            logger['spread_skill'].append(estats['spread_skill'])
        logger['train_samples_per_s'].append(world * n_epoch / max(time.time() - t_epoch, 1e-9))   # data path included
        logger['MSELoss'].append(loss_e)                                                     # (MSE+L1, as in train.py:116)
        logger['r2_score'].append(r2_e)
        scheduler.step()                                                                     # train.py:120
        generator.eval()
        trainer.reset_stats()
        for idx in shard_indices(len(val_dataset), 0, rank, world, 1, shuffle=False):        # utils.py:52-75, batch 1
            trainer.evaluate(*get_batch(val_dataset, idx))
        logger['r2_score_val'].append(trainer.epoch_stats()[1])
        if rank == 0:
            print(f"Epoch: {epoch}, Loss: {logger['MSELoss'][-1]:.5f}, R2T: {logger['r2_score'][-1]:.5f}, "
                  f"R2V: {logger['r2_score_val'][-1]:.5f}"                                   # train.py:124
                  + ("" if p_epoch is None else f", sampling prob: {p_epoch:.3f}")
                  + ("" if not M_ens else f", crps: {estats['crps']:.5f}, spread/skill: {estats['spread_skill']:.3f}"))
            if guarded:
                print(f"  grad norm: mean {gstats['mean_norm']:.5f}, max {gstats['max_norm']:.5f}, "
                      f"clipped {gstats['clipped']}, skipped {gstats['skipped']} of {gstats['calls']} steps")
            print(f"  train loop incl. device preproc: {logger['train_samples_per_s'][-1]:.1f} samples/s")
            if epoch % 10 == 0:                                                              # train.py:126-136
                d = os.path.join(args.snapshot_dir, f'epoch-{epoch:003d}')
                os.makedirs(d, exist_ok=True)
                print('Learning Rate:', scheduler.get_last_lr())
                save_checkpoint(generator, optimizer, os.path.join(d, 'generator.pth.tar'), scheduler.get_last_lr(), epoch)
    if rank == 0:
        with open(os.path.join(args.snapshot_dir, "logger.npy"), mode='wb') as f:           # train.py:138-142
            np.save(f, np.array(logger['MSELoss']))
            np.save(f, np.array(logger['r2_score']))
            np.save(f, np.array(logger['r2_score_val']))
        if args.test_skill:
            # the evaluation cells of test.ipynb on the 'test' period: the last step's prediction, sums kept on the device
            from nasa_niswan_amd.inference import evaluate_skill
            test_dataset = SyntheticE33OMA_CRNN('test', **dict(ds_kw, sequence_targets=False))
            lat = grid_latitudes(H)                                                          # cell centres of the H-row global grid
            report = evaluate_skill(generator, test_dataset, batch_size=args.batch_size, halo=halo, lat=lat).report(
                test_dataset.y_mean, test_dataset.y_std)
            np.savez(os.path.join(args.snapshot_dir, "skill.npz"), **report.arrays())
            logger['skill'] = report
            print(f"Test period ({len(test_dataset)} windows): mean R2 per window {np.mean(report.r2_temporal):.5f}, "
                  f"mean R2 per grid cell {np.mean(report.r2_spatial):.5f}")
        if args.test_rollout:
            # closed loop over the 'test' period: non-overlapping windows of spin-up + horizon steps, skill by lead time
            from nasa_niswan_amd.inference import lead_time_r2, rollout_skill
            test_dataset = SyntheticE33OMA_CRNN('test', **dict(ds_kw, sequence_targets=False))
            span = args.rollout_spinup + args.test_rollout
            t_lo, t_hi = int(test_dataset.first[0]), int(test_dataset.yraw.shape[0])
            starts = list(range(t_lo, t_hi - span + 1, span))
            if not starts:
                raise SystemExit(f"--test-rollout: the test period ({t_hi - t_lo} steps) holds no window of {span} steps")
            spectra = {}
            if args.test_spectrum:
                from nasa_niswan_amd.inference import SpectrumAccumulator
                for name, members in (("rollout", 1), ("ensemble", args.ensemble_members)):
                    if members:
                        spectra[name] = SpectrumAccumulator(test_dataset.levels, H, W, M=members, nslots=args.test_rollout,
                                                            lat=grid_latitudes(H), device=dev)
            acc = rollout_skill(generator, test_dataset, starts, args.test_rollout, args.rollout_spinup, args.batch_size,
                                lat=grid_latitudes(H), spectrum=spectra.get("rollout"))
            r2_lead = [float(v) for v in lead_time_r2(acc)]
            logger['rollout_r2'] = r2_lead
            np.save(os.path.join(args.snapshot_dir, "rollout_r2.npy"), np.array(r2_lead))
            print(f"Closed-loop roll-out, {len(starts)} windows, spin-up {args.rollout_spinup}: R2 per lead time")
            print("  " + " ".join(f"{j}:{v:.4f}" for j, v in enumerate(r2_lead)))
            if args.ensemble_members:
                from nasa_niswan_amd.inference import LEAD_TIME_COLUMNS, lead_time_table, rollout_ensemble
                ens = rollout_ensemble(generator, test_dataset, starts, args.test_rollout, args.rollout_spinup, args.ensemble_members,
                                       ic_noise=args.ensemble_noise, feedback_noise=args.ensemble_feedback_noise,
                                       seed=args.ensemble_seed, batch_size=args.batch_size, lat=grid_latitudes(H),
                                       spectrum=spectra.get("ensemble"))
                table = lead_time_table(ens)
                logger['rollout_ensemble'] = table
                np.save(os.path.join(args.snapshot_dir, "rollout_ensemble_table.npy"), table)
                np.savez(os.path.join(args.snapshot_dir, "rollout_ensemble.npz"),
                         **ens.report(test_dataset.y_mean, test_dataset.y_std).arrays())
                print(f"Ensemble roll-out, {args.ensemble_members} members (z-score units): lead " + " ".join(LEAD_TIME_COLUMNS))
                for j, row in enumerate(table):
                    print(f"  {j}: " + " ".join(f"{v:.4f}" for v in row))
            if spectra:
                from nasa_niswan_amd.inference import LEAD_SPECTRUM_COLUMNS, lead_time_spectrum
                out, tables = {}, {}
                for name, sp in spectra.items():
                    spec, counts = sp.sums()
                    tables[name] = lead_time_spectrum(sp)
                    out.update({f"{name}_spec": spec, f"{name}_counts": counts, f"{name}_table": tables[name], f"{name}_members": sp.M})
                    out.update({f"{name}_{k}": v for k, v in sp.report().arrays().items()})
                    print(f"Zonal spectra of the {name}, {sp.M} member(s), k >= {sp.Wc // 8} as the small scales: lead "
                          + " ".join(LEAD_SPECTRUM_COLUMNS))
                    for j, row in enumerate(tables[name]):
                        print(f"  {j}: " + " ".join(f"{v:.4f}" for v in row))
                logger['rollout_spectrum'] = tables
                np.savez(os.path.join(args.snapshot_dir, "rollout_spectrum.npz"), columns=np.array(LEAD_SPECTRUM_COLUMNS), **out)
        time_elapsed = time.time() - since
        print(f'Training complete in {time_elapsed // 60:.0f}m {time_elapsed % 60:.0f}s')
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return logger


if __name__ == '__main__':
    main(get_arguments())
