"""A bounded run of the random-shape screen's roll-out mode (tools/fuzz_shapes.py --rollout: a drawn stack, grid, number of
feedback channels, first fed step F >= 1, storage type, boundary condition, input layout and cotangents; outputs, every
parameter gradient and dx of net(x, free_from=F, feedback_grad=True) against tests/rollout_model.py under CPU autograd),
beside tests/test_gpu_fuzz_closed_loop.py: fixed seeds.  tests/test_rollout_cpu.py asserts that these seeds contain the
combinations the mode exists for."""
import pytest

import test_gpu_fuzz as G

RUN = ["--n", "12", "--seed", "1913", "--rollout"]


@pytest.mark.gpu
def test_rollout_mode_against_the_cpu_model():
    out = G.run_tool(RUN)
    assert out.count("ok   #") == 12, out[-2000:]
