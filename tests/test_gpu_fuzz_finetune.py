"""A bounded run of the random-shape screen's fine-tuning mode (tools/fuzz_shapes.py --finetune: a drawn stack, a drawn number
of frozen layers 0 ... L, weight decay and per-layer lr scales; two steps of FusedTrainer against CPU autograd and
torch.optim.AdamW), beside tests/test_gpu_fuzz.py: fixed seeds, once with --self-check (the reference's AdamW loses its
weight decay, then trains the frozen layers too: the comparison has to fail).  The CPU test asserts that these seeds contain
the combinations the mode exists for."""
import importlib.util
import os

import pytest

import test_gpu_fuzz as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--n", "8", "--seed", "708", "--finetune"]
SELF_CHECK = ["--n", "2", "--seed", "708", "--finetune", "--self-check"]


def _tool():
    spec = importlib.util.spec_from_file_location("fuzz_shapes_ft", os.path.join(ROOT, "tools", "fuzz_shapes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_finetune_seeds_contain_what_the_mode_exists_for():
    tool = _tool()
    args = tool.parse(RUN)
    assert args.mode == "finetune"
    cases = tool.draw_cases(args.seed, args.n, args.mode)
    assert any(c["f"] == 0 for c in cases), "nothing frozen"
    assert any(0 < c["f"] < c["L"] for c in cases), "a frozen prefix"
    assert any(c["f"] == c["L"] for c in cases), "the head alone"
    assert any(c["wd"] == 0 for c in cases) and any(c["wd"] > 0 for c in cases)
    assert {c["dtype"] for c in cases if 0 < c["f"] < c["L"]} == {"f32", "bf16"}
    assert all(len(c["scales"]) == c["L"] and 0 <= c["f"] <= c["L"] for c in cases)
    sc = tool.parse(SELF_CHECK)
    assert sc.self_check and sc.mode == "finetune"
    first = tool.draw_cases(sc.seed, sc.n, sc.mode)
    assert any(c["wd"] > 0 for c in first) and any(c["f"] > 0 for c in first)           # both faults apply
    # the mode has a stream of its own, and the modes before it keep theirs
    assert tool.NEW_MODES[-1] == "finetune" and tool.NEW_MODES[:3] == ("state", "train_opts", "stateful")
    assert tool.draw_case(tool.case_rng(708, "finetune", 5), 5, "finetune") == cases[5]


@pytest.mark.gpu
def test_finetune_mode_against_the_oracle():
    G.run_tool(RUN)


@pytest.mark.gpu
def test_the_finetune_screen_sees_a_corrupted_reference():
    out = G.run_tool(SELF_CHECK)
    assert out.count("self-check ok") == 2 and "SELF-CHECK" not in out, out[-2000:]
