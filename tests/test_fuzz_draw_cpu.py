"""The draw of tools/fuzz_shapes.py without a GPU: the seeded runs of tests/test_gpu_fuzz.py really contain the combinations
the state / options modes exist for (a condition on the chosen seeds and counts: if one misses, change the seed or the
count, not the list), the draw is pure and replayable, and ``--list`` prints it without importing the package."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

import test_gpu_fuzz as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "fuzz_shapes.py")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("fuzz_shapes_draw", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.pkg is None                      # loading the tool loads neither the package nor the library
    return mod


def cases_of(tool, mode):
    """every case the seeded runs of `mode` in tests/test_gpu_fuzz.py draw"""
    out = []
    for extra in G.NEW_RUNS:
        args = tool.parse(extra)
        if args.mode == mode:
            out += tool.draw_cases(args.seed, args.n, args.mode)
    assert out, mode
    return out


def require(cases, **conds):
    missing = [name for name, f in conds.items() if not any(f(c) for c in cases)]
    assert not missing, f"no drawn case with: {missing}"


def test_state_runs_contain_the_combinations(tool):
    cases = cases_of(tool, "state")
    given = [c for c in cases if c["form"] != "none"]            # a state goes in: a has_init workspace
    require(given,
            L1=lambda c: c["L"] == 1, L3=lambda c: c["L"] == 3, L4=lambda c: c["L"] == 4,
            k1=lambda c: 1 in c["ks"], k7=lambda c: 7 in c["ks"],
            hidden64=lambda c: max(c["hidden"]) >= 64,
            folded_thin_input=lambda c: c["C"] <= 3 and c["ks"][0] >= 5,
            B1=lambda c: c["B"] == 1, T1=lambda c: c["T"] == 1,
            **{f"wave_{w}": (lambda c, w=w: c["wave"] == w) for w in tool.WAVES},
            **{f"rows_{r}": (lambda c, r=r: c["rows"] == r) for r in (0, 4, 8)},
            f32=lambda c: c["dtype"] == "f32", bf16=lambda c: c["dtype"] == "bf16",
            sequence=lambda c: c["return_sequence"], no_sequence=lambda c: not c["return_sequence"],
            lanes=lambda c: c["form"] == "lanes", full=lambda c: c["form"] == "full",
            chained=lambda c: c["chain"], one_call=lambda c: not c["chain"],
            # the combinations the issue names: four layers with a state, T = 1 at B = 1 on a ragged grid
            ragged=lambda c: c["H"] % 8 and c["W"] % 16)
    require(cases, no_state=lambda c: c["form"] == "none")


def test_train_opts_runs_contain_the_combinations(tool):
    cases = cases_of(tool, "train_opts")
    require(cases,
            n2=lambda c: c["n"] == 2, n3=lambda c: c["n"] == 3, n4=lambda c: c["n"] == 4,
            S1_segments=lambda c: c["S"] == 1 and c["n"] >= 2,
            accumulate_with_segments=lambda c: c["acc"] == 2 and c["n"] >= 2,
            accumulate_without_segments=lambda c: c["acc"] == 2 and c["n"] == 1,
            # two micro-batches of a whole window of more than one step, in both storage types (bf16: each window's share of the
            # bucket is gated on its own stored factors), plain and with the sequence loss
            f32_accumulate_without_segments=lambda c: c["dtype"] == "f32" and c["acc"] == 2 and c["n"] == 1 and c["T"] > 1,
            bf16_accumulate_without_segments=lambda c: (c["dtype"] == "bf16" and c["acc"] == 2 and c["n"] == 1 and c["T"] > 1
                                                        and not c["sequence_loss"]),
            bf16_accumulate_sequence_loss=lambda c: c["dtype"] == "bf16" and c["acc"] == 2 and c["sequence_loss"] and c["T"] > 1,
            # f32 sees what bf16 with segments cannot gate on a slab: the accumulating fold of the reductions
            f32_segments=lambda c: c["dtype"] == "f32" and c["n"] >= 2 and c["acc"] == 1,
            f32_accumulate_with_segments=lambda c: c["dtype"] == "f32" and c["n"] >= 2 and c["acc"] == 2,
            no_weights=lambda c: c["wform"] == "none", row_weights=lambda c: c["wform"] == "row",
            map_weights=lambda c: c["wform"] == "map",
            clipped=lambda c: c["clip"] == 0.5, norm_below_the_limit=lambda c: c["clip"] == 2.0,
            sequence_loss=lambda c: c["sequence_loss"],
            out5=lambda c: c["out"] >= 5,
            tile_rows_with_segments=lambda c: c["rows"] in (4, 8) and c["n"] >= 2,
            **{f"wave_{w}_accumulate": (lambda c, w=w: c["wave"] == w and (c["acc"] == 2 or c["n"] >= 2)) for w in (0, 1, 2)})
    for c in cases:
        assert c["T"] == c["n"] * c["S"] and c["B"] >= 2 and c["out"] >= 2
        assert not (c["sequence_loss"] and c["n"] > 1)


def test_stateful_runs_contain_the_combinations(tool):
    cases = cases_of(tool, "stateful")
    require(cases,
            partial_reset=lambda c: c["reset_kind"] == "partial", full_reset=lambda c: c["reset_kind"] == "full",
            no_reset=lambda c: c["reset_kind"] == "none",
            n1=lambda c: c["n"] == 1, segments=lambda c: c["n"] >= 2,
            f32=lambda c: c["dtype"] == "f32", bf16=lambda c: c["dtype"] == "bf16")
    for c in cases:
        if c["reset_kind"] == "partial":
            assert any(c["reset"]) and not all(c["reset"]), c["reset"]


def test_self_check_runs_meet_their_faults(tool):
    """every --self-check run draws a case each of its faults applies to (the tool fails the run otherwise)"""
    for extra in G.SELF_CHECKS:
        args = tool.parse(extra)
        assert args.self_check
        cases = tool.draw_cases(args.seed, args.n, args.mode)
        if args.mode == "state":
            require(cases, given_state=lambda c: c["form"] != "none")
        elif args.mode == "train_opts":
            require(cases, segments=lambda c: c["n"] >= 2, accumulation=lambda c: c["acc"] == 2)
        else:
            require(cases, reset=lambda c: c["reset_kind"] != "none")
    assert sorted(tool.parse(e).mode for e in G.SELF_CHECKS) == ["state", "stateful", "train_opts"]


def test_draw_is_pure_and_each_new_case_replays_alone(tool):
    for mode in tool.NEW_MODES:
        a, b = tool.draw_cases(5, 6, mode), tool.draw_cases(5, 6, mode)
        assert a == b
        assert tool.draw_case(tool.case_rng(5, mode, 4), 4, mode) == a[4]          # no replay of cases 0..3 needed
        assert tool.draw_cases(6, 6, mode) != a
        for c in a:
            assert c["hidden"] and max(c["hidden"]) <= 64 and 5 <= c["H"] <= 30 and 9 <= c["W"] <= 50 and c["out"] in (1, 2, 5, 20)
            assert c["wave"] == tool.WAVES[c["it"] % 7] and c["rows"] == tool.TILE_ROWS[c["it"] % 4]
            assert c["dtype"] == ("f32" if c["it"] % 2 == 0 else "bf16")
    # the state modes draw from streams of their own: the plain stream's cases are not theirs
    assert tool.draw_cases(5, 6, "plain")[0]["tag"] != tool.draw_cases(5, 6, "state")[0]["tag"]


def test_old_mode_streams_are_those_of_the_first_version(tool):
    """the first and the LAST tag of each of the four seeded runs of the first version of the tool, as it printed them (the
    last one stands only if every draw before it, data included, took what it took then), and the last case's values that
    the tag does not carry"""
    runs = {("plain", 11, 30): ("#0 C=16 hidden=[8] k=[5] out=20 B=4 T=3 6x38 f32 wave=None rows=0 wide=0",
                                "#29 C=126 hidden=[4, 24] k=[3, 3] out=1 B=1 T=3 22x63 bf16 wave=0 rows=0 wide=0", {}),
            ("trainer", 12, 16): ("#0 C=3 hidden=[16, 128, 128] k=[1, 3, 3] out=20 B=2 T=2 13x67 f32 wave=None rows=0 wide=0",
                                  "#15 C=7 hidden=[16, 48] k=[5, 7] out=200 B=5 T=3 5x21 bf16 wave=0 rows=8 wide=0", {"halo": [1, 1]}),
            ("cell", 13, 24): ("#0 cell Cx=1 Ch=64 k=5 B=5 26x57 f32 bias=False rows=0",
                               "#23 cell Cx=126 Ch=16 k=1 B=4 21x60 bf16 bias=True rows=8", {}),
            ("dataset", 14, 24): ("#0 dataset levels=3 grid=7x29 pad=(0,4) reference T=1 f32",
                                  "#23 dataset levels=2 grid=23x7 pad=(1,3) reflect T=2 bf16", {"idx": [9], "k0": 3})}
    old = [tool.parse(e) for e in G.test_random_shapes_against_the_oracle.pytestmark[0].args[1]]
    assert sorted((a.mode, a.seed, a.n) for a in old) == sorted(runs)         # the four runs of tests/test_gpu_fuzz.py
    for (mode, seed, n), (first, last, more) in runs.items():
        cases = tool.draw_cases(seed, n, mode)
        assert (cases[0]["tag"], cases[-1]["tag"]) == (first, last)
        assert {k: cases[-1][k] for k in more} == more


def test_list_prints_the_draw_without_importing_the_package(tool):
    code = ("import runpy, sys; sys.argv = ['fuzz_shapes.py', '--list', '--n', '3', '--seed', '7', '--stateful']; "
            f"runpy.run_path({TOOL!r}, run_name='__main__'); "
            "assert not any(m.startswith('nasa_niswan_amd') or m.startswith('oracle') for m in sys.modules), 'package imported'")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [json.loads(line) for line in r.stdout.splitlines()]
    want = json.loads(json.dumps(tool.draw_cases(7, 3, "stateful")))
    assert got == want
