"""A bounded run of the random-shape screen's closed-loop mode (tools/fuzz_shapes.py --closed-loop: a drawn stack, grid,
number of feedback channels, first fed step, tensor state or none, storage type, boundary condition and input layout; the
per-step predictions against tests/closed_loop_model.py and, bit for bit, against the open-loop pass over the substituted
input), beside tests/test_gpu_fuzz_finetune.py: fixed seeds.  tests/test_closed_loop_cpu.py asserts that these seeds contain the
combinations the mode exists for."""
import pytest

import test_gpu_fuzz as G

RUN = ["--n", "12", "--seed", "811", "--closed-loop"]


@pytest.mark.gpu
def test_closed_loop_mode_against_the_cpu_model():
    out = G.run_tool(RUN)
    assert out.count("ok   #") == 12, out[-2000:]
