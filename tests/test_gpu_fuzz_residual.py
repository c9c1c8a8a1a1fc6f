"""A bounded run of the random-shape screen's residual-head mode (tools/fuzz_shapes.py --residual: a drawn stack, grid, number
of feedback channels, storage type, boundary condition, input layout, state, first fed step or feed mask, and cotangents; the
residual closed loop bit for bit against the residual open loop on the substituted input, and outputs, every parameter gradient
and dx of net(x, ..., feedback_grad=True) against tests/residual_model.py under CPU autograd), beside
tests/test_gpu_fuzz_sampled.py: fixed seeds, and once with --self-check -- the reference loses the base and the comparison has
to fail.  tests/test_residual_cpu.py asserts that these seeds contain the combinations the mode exists for."""
import pytest

import test_gpu_fuzz as G

RUN = ["--n", "10", "--seed", "3100", "--residual"]
SELF_CHECK = ["--n", "1", "--seed", "3100", "--residual", "--self-check"]


@pytest.mark.gpu
def test_residual_mode_against_the_cpu_model():
    out = G.run_tool(RUN)
    assert out.count("ok   #") == 10, out[-2000:]


@pytest.mark.gpu
def test_the_screen_sees_a_reference_without_the_base():
    out = G.run_tool(SELF_CHECK)
    assert "self-check ok" in out and "SELF-CHECK" not in out, out[-2000:]
