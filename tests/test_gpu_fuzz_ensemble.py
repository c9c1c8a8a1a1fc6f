"""A bounded run of the random-shape screen's ensemble mode (tools/fuzz_shapes.py --ensemble: nint_ens_accum on drawn members,
samples, outputs, grids, crop windows, slots and member layouts against tests/ensemble_model.py), beside
tests/test_gpu_fuzz_noise.py: fixed seeds."""
import json
import os
import subprocess
import sys

import pytest

import test_gpu_fuzz as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--n", "12", "--seed", "4100", "--ensemble"]


def test_the_seeds_hold_what_the_mode_exists_for():
    """(no GPU) both layouts and kinds of data, the largest M, more samples than one launch holds, a crop of one pixel and one
    wider than a workgroup, samples left out of the maps -- and no earlier mode's stream moved"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_shapes.py"), *RUN, "--list"], capture_output=True, text=True,
                         check=True).stdout
    cases = [json.loads(line) for line in out.splitlines()]
    assert len(cases) == 12 and all(c["mode"] == "ensemble" for c in cases)
    assert {c["layout"] for c in cases} == {"contiguous", "rollout"} and {c["integer"] for c in cases} == {True, False}
    assert any(c["M"] == 64 for c in cases) and any(c["N"] > 64 for c in cases) and any(c["M"] == 2 for c in cases)
    assert any(c["Hc"] * c["Wc"] == 1 for c in cases) and any(c["Hc"] * c["Wc"] > 256 for c in cases)
    assert any(-1 in c["slots"] and max(c["slots"]) >= 0 for c in cases) and all(max(c["slots"]) < c["nslots"] - 1 for c in cases)
    assert any(c["O"] > 4 for c in cases) and any(c["row_w"] for c in cases)
    for c in cases:
        assert 0 <= c["oy"] and c["oy"] + c["Hc"] <= c["H"] and 0 <= c["ox"] and c["ox"] + c["Wc"] <= c["W"]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import fuzz_shapes as FZ
    finally:
        sys.path.pop(0)
    assert FZ.ENSEMBLE_MODES == ("ensemble",) and FZ.NOISE_MODES == ("noise",) and FZ.RESIDUAL_MODES == ("residual",)
    assert FZ.ALL_STREAM_MODES == FZ.STREAM_MODES + ("rollout",)


@pytest.mark.gpu
def test_ensemble_mode_against_the_numpy_model():
    out = G.run_tool(RUN)
    assert out.count("ok   #") == 12, out[-2000:]
