"""A bounded run of the random-shape screen's scheduled-sampling mode (tools/fuzz_shapes.py --sampled: a drawn stack, grid,
number of feedback channels, storage type, boundary condition, input layout, state, feed mask and cotangents; the masked
forward pass bit for bit against the open-loop pass on the substituted input, and outputs, every parameter gradient and dx of
net(x, free_mask=M, feedback_grad=True) against tests/sampled_model.py under CPU autograd), beside
tests/test_gpu_fuzz_rollout.py: fixed seeds.  tests/test_sampled_cpu.py asserts that these seeds contain the combinations the
mode exists for."""
import pytest

import test_gpu_fuzz as G

RUN = ["--n", "12", "--seed", "2008", "--sampled"]


@pytest.mark.gpu
def test_sampled_mode_against_the_cpu_model():
    out = G.run_tool(RUN)
    assert out.count("ok   #") == 12, out[-2000:]
