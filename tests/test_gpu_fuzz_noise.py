"""A bounded run of the random-shape screen's input-noise mode (tools/fuzz_shapes.py --noise: a drawn stack, grid, noise span, sigma
per channel, storage type, boundary condition, input layout and generator key; outputs, every parameter gradient and dx of
net(x, input_noise=N) against the CPU oracle under autograd on the pre-noised input that tests/noise_model.py builds on the host),
beside tests/test_gpu_fuzz_residual.py: fixed seeds, and once with --self-check -- the reference sees the clean input and the
comparison has to fail."""
import json
import os
import subprocess
import sys

import pytest

import test_gpu_fuzz as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--n", "10", "--seed", "3200", "--noise"]
SELF_CHECK = ["--n", "1", "--seed", "3200", "--noise", "--self-check"]


def test_the_seeds_hold_what_the_mode_exists_for():
    """(no GPU) folded and plain inputs, both boundaries and storage types, a zero sigma, a span that is neither at channel 0 nor
    at the end, a step counter that wraps inside the window -- and no earlier mode's stream moved"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_shapes.py"), *RUN, "--list"], capture_output=True, text=True,
                         check=True).stdout
    cases = [json.loads(line) for line in out.splitlines()]
    assert len(cases) == 10 and all(c["mode"] == "noise" for c in cases)
    assert {c["fold"] for c in cases} == {True, False} and {c["cyclic"] for c in cases} == {True, False}
    assert {c["dtype"] for c in cases} == {"f32", "bf16"}
    assert any(0.0 in c["sigma"] for c in cases) and any(c["c0"] > 0 and c["c0"] + c["n"] < c["C"] for c in cases)
    assert any(c["key"]["step0"] + c["T"] > 1 << 32 for c in cases)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import fuzz_shapes as FZ
    finally:
        sys.path.pop(0)
    assert FZ.NOISE_MODES == ("noise",) and FZ.RESIDUAL_MODES == ("residual",) and FZ.SAMPLED_MODES == ("sampled",)
    assert FZ.ALL_STREAM_MODES == FZ.STREAM_MODES + ("rollout",)


@pytest.mark.gpu
def test_noise_mode_against_the_cpu_oracle_on_the_pre_noised_input():
    out = G.run_tool(RUN)
    assert out.count("ok   #") == 10, out[-2000:]


@pytest.mark.gpu
def test_the_screen_sees_a_reference_on_the_clean_input():
    out = G.run_tool(SELF_CHECK)
    assert "self-check ok" in out and "SELF-CHECK" not in out, out[-2000:]
