"""A bounded run of the random-shape screen (tools/fuzz_shapes.py: layer counts 1-4, kernel sizes 1-7, ragged grids, 1-62 input
channels, B = 1-5, T = 1-4, both storage types, merged-grid launches on / off, both tile heights) against the CPU oracle:
the module / autograd path, the fused trainer path, the single cell with a given state, and the device preproc of a
resident record (as a batch tensor and straight into the model's input slab).  Seeds are fixed; the tool itself takes any seed.  (It found the
one-input-channel fold bug of round 3.)

The state / options modes (--state: the module with a state in and out; --train-opts: FusedTrainer.step with drawn segments,
accumulation, loss weights, clipping and sequence loss; --stateful: two chunks of a stateful trainer with a drawn reset) run
the same way, and once each with --self-check: the reference is corrupted on the host after the first passing case and the
comparison has to fail.  tests/test_fuzz_draw_cpu.py asserts without a GPU that these seeds and counts contain the
combinations the modes exist for."""
import os
import re
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# counts: each run takes no longer than the --trainer run above on the same machine (wall times are printed)
NEW_RUNS = [["--n", "30", "--seed", "250", "--state"], ["--n", "11", "--seed", "551", "--train-opts"],
            # (two micro-batches of an unsegmented window, T > 1, in both storage types: a run of its own, so that neither is slow)
            ["--n", "4", "--seed", "483", "--train-opts"], ["--n", "12", "--seed", "387", "--stateful"]]
SELF_CHECKS = [["--n", "2", "--seed", "38", "--state", "--self-check"], ["--n", "2", "--seed", "34", "--train-opts", "--self-check"],
               ["--n", "2", "--seed", "31", "--stateful", "--self-check"]]


@pytest.mark.parametrize("extra", [["--n", "30", "--seed", "11"], ["--n", "16", "--seed", "12", "--trainer"], ["--n", "24", "--seed", "13", "--cell"], ["--n", "24", "--seed", "14", "--dataset"]])
def test_random_shapes_against_the_oracle(extra):
    run_tool(extra)


def run_tool(extra):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_shapes.py")] + extra, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-6:])
    assert r.returncode == 0, tail
    assert "shapes ok" in r.stdout, tail
    print(f"{' '.join(extra)}: {time.time() - t0:.1f} s; {r.stdout.splitlines()[-1]}")
    return r.stdout


@pytest.mark.parametrize("extra", NEW_RUNS, ids=lambda e: f"{e[-1]}-seed{e[3]}")
def test_state_and_option_modes_against_the_oracle(extra):
    run_tool(extra)


@pytest.mark.parametrize("extra", SELF_CHECKS, ids=lambda e: e[-2])
def test_the_screen_sees_a_corrupted_reference(extra):
    out = run_tool(extra)
    assert "self-check ok" in out and "SELF-CHECK" not in out, out[-2000:]


def test_cell_on_the_other_side_of_the_l1_kink_replays():
    """seed 215 --train-opts #1 (bf16, one 1x1 layer, 15 x 8 crop, two micro-batches of a window in three segments): one cell's
    pred - y has another sign on the device than in the oracle, which without tools/fuzz_shapes.py::device_side puts 3.9e-2 on
    the layer's weight gradient and 1.9e-1 on the head's bias gradient while f32 agrees to 1.1e-6.  The oracle
    adopts the device's side at exactly that ONE of the 356 weighted cells of the two windows together, a cell whose |d| is
    within the bound the prediction's gate sets; no cell beyond the bound stands on the other side, and d loss / d pred and the
    prediction read back from it pass their gates."""
    out = run_tool(["--n", "16", "--seed", "215", "--train-opts", "--only", "1"])
    rows = re.findall(r"window (\d): (\d+) of (\d+) cells on the other side of d = 0 adopted \(largest \|d\| (\S+), bound (\S+)\), "
                      r"(\d+) beyond the bound; min \|dpred cnt / w\| (\S+)", out)
    assert [r[0] for r in rows] == ["0", "1"], out[-3000:]
    assert sum(int(r[1]) for r in rows) == 1 and all(int(r[2]) == 356 and int(r[5]) == 0 for r in rows), rows
    assert all(float(r[3].rstrip(",")) <= float(r[4].rstrip(")")) and float(r[6]) >= 1.0 - 1e-5 for r in rows), rows
    assert "dpred.0" in out and "dpred.1" in out and "pred.1" in out and "MISS" not in out, out[-3000:]


# ------------------------------------------------------------------------------ the same screen inside the guarded allocator
# One --guarded run per mode, on the seeds above (tools/fuzz_shapes.py --guarded: every device buffer of a case between guards,
# `empty` payloads poisoned, inputs and parameters in arenas of their own, every guard byte compared after each case).  Counts:
# each run takes no longer than the longest run above on the same machine (wall times are printed; with the counts of the
# unguarded runs the guarded plain and --trainer runs measured 4.5 and 4.4 s against 4.4 - 4.5 and 4.4 s: theirs are lower).
GUARDED_RUNS = [["--n", "24", "--seed", "11"], ["--n", "14", "--seed", "12", "--trainer"], ["--n", "24", "--seed", "13", "--cell"],
                ["--n", "24", "--seed", "14", "--dataset"], ["--n", "30", "--seed", "250", "--state"],
                ["--n", "11", "--seed", "551", "--train-opts"], ["--n", "12", "--seed", "387", "--stateful"],
                ["--n", "8", "--seed", "708", "--finetune"]]


@pytest.mark.parametrize("extra", GUARDED_RUNS, ids=lambda e: f"{e[-1] if e[-1].startswith('--') else '--plain'}-seed{e[3]}")
def test_random_shapes_inside_the_guarded_allocator(extra):
    out = run_tool(extra + ["--guarded"])
    assert "every guard byte intact" in out and "GUARD HIT" not in out, out[-2000:]


def test_the_guarded_screen_sees_a_flipped_guard_byte():
    out = run_tool(["--n", "2", "--seed", "11", "--guarded", "--self-check"])
    assert "self-check ok: one flipped byte in a back guard" in out and "guard damaged" in out and "SELF-CHECK" not in out, out[-2000:]
