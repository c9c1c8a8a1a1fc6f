"""The whole-sequence pass (csrc/seq.hip: its check, its planners, the halo wrap pass) held against records of itself, without a
GPU.

The three nint_debug_seq_plan* entries return the refusal of a call or every conv / pointwise problem of its plan.
tests/golden/seq_plan.npy.xz holds those rows over the sweep of oracle/seq_plan.py as the library gave them BEFORE the open,
closed-loop and roll-out windows shared one pass description, one check and one funnel: the one check (its order decides the
code of a doubly wrong call) and the one planner must reproduce them row for row, refusals included.
"""
import os

import numpy as np
import pytest

from oracle import seq_plan as SP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_plan.npy.xz")
OK, E_ARG, E_SHAPE, E_ALIGN = 0, -1, -2, -4


@pytest.fixture(scope="module")
def tables():
    from nasa_niswan_amd import _lib
    want_cases, want = SP.load(GOLDEN)
    cases, got = SP.table(_lib.load())
    assert np.array_equal(cases, want_cases), "the sweep of oracle/seq_plan.py is not the fixture's"
    return cases, got, want


def test_the_fixture_is_not_hollow():
    cases, want = SP.load(GOLDEN)
    assert len(cases) > 5000 and want.shape[1] == len(SP.FIELDS)
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f))
                                          for f in os.listdir(os.path.dirname(GOLDEN)) if f != os.path.basename(GOLDEN))
    col = lambda name: cases[:, SP.CASE.index(name)]
    vals = lambda name: set(col(name).tolist())
    T, rc = SP.T, want[:, 0]
    assert vals("entry") == {0, 1, 2} and vals("bwd") == {0, 1} and vals("bf16") == {0, 1} and vals("cyclic") == {0, 1}
    stacks = [SP.STACKS[i] for i in vals("stack")]
    assert {len(h) for _, h, _ in stacks} == {1, 2, 3, 4} and {c for c, _, _ in stacks} >= {5, 64}     # folded and plain inputs
    assert vals("wave") == {0, 1, 2, 3, 4, 5, 7} and vals("shape") == {0, 1, 2}
    assert vals("fuse") == set(range(len(SP.FUSE))) and sum(f & SP.EXPLICIT != 0 for f in SP.FUSE) >= 2
    assert vals("has_init") == {0, 1} and vals("need_dx") == {0, 1} and vals("parts") == {0, 1, 2} and vals("accumulate") == {0, 1}
    assert vals("train_from") == {0, 1, 2, 3, 4} and vals("dh_seq") == {0, 1, 2}
    for L in (1, 2, 3, 4):      # train_from runs over 0 .. L of every depth
        sel = np.array([len(SP.STACKS[i][1]) == L for i in col("stack")])
        assert set(col("train_from")[sel].tolist()) == set(range(L + 1))
    assert vals("fb") == {0, 1, 2} and vals("O_kind") == {0, 1, 2, 3} and vals("from") >= {-1, 0, 1, T - 1, T, T + 1}
    assert SP.WIDE_HEAD in vals("stack")
    # what was recorded: every code of the checks and of the planner, accepted and refused rows of each entry
    assert set(rc[rc <= 0].tolist()) == {OK, E_ARG, E_SHAPE, E_ALIGN}
    for e in (0, 1, 2):
        assert (rc[col("entry") == e] > 0).sum() > 200 and (rc[col("entry") == e] < 0).sum() > 50
    fed = (col("fb") > 0) & (col("O_kind") > 0) & (col("from") < T)
    assert (rc[fed & (col("entry") == 2)] > 0).sum() > 500 and (rc[fed & (col("entry") == 1) & (col("bwd") == 0)] > 0).sum() > 500
    recs = want[:, 1:].reshape(len(want), SP.CAP, len(SP.REC))
    live = np.arange(SP.CAP)[None, :] < np.maximum(rc, 0)[:, None]
    assert set(recs[live][:, SP.REC.index("kernel")].tolist()) == set(range(9))         # NINT_K_*
    assert set(recs[live][:, SP.REC.index("op")].tolist()) == {0, 1, 2, 3}               # NINT_OP_*
    assert not recs[~live].any()


def test_the_pass_reproduces_the_recorded_plans(tables):
    cases, got, want = tables
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        r = int(bad[0])
        f = [(SP.FIELDS[c], int(got[r, c]), int(want[r, c])) for c in np.nonzero(got[r] != want[r])[0][:12]]
        pytest.fail(f"{len(bad)} of {len(cases)} cases differ; first: {dict(zip(SP.CASE, cases[r].tolist()))}: (field, got, want) {f}")
