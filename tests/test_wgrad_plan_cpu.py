"""The weight-gradient planner (csrc/wgrad.hip) held against records of itself, without a GPU.

nint_debug_wgrad_plan runs wg_plan and nint_internal_wgrad_plan on the host and returns every launch (instance, grid, block,
LDS bytes, the sources with their slab offsets) and the fold.  tests/golden/wgrad_plan.npy.xz holds those records over the
sweep of oracle/wgrad_plan.py as the planner gave them BEFORE the instance table replaced dispatch_wgrad and the three copies
of the split rule: the table, wg_splits and the plan-time refusal must reproduce them row for row, refusals included.

The second half ties the exact-reduction GPU test to the table: its KEYS cases name the instance they mean to run, and together
they must run every instance that a layer padded by nint_kc can reach.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import wgrad_plan as WP

import test_gpu_exact_reductions as ER

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan.npy.xz")


@pytest.fixture(scope="module")
def lib():
    from nasa_niswan_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def tables(lib):
    want_cases, want = WP.load(GOLDEN)
    cases, got = WP.table(lib)
    assert np.array_equal(cases, want_cases), "the sweep of oracle/wgrad_plan.py is not the fixture's"
    return cases, got, want


def _first_difference(cases, got, want, cols):
    bad = np.nonzero((got[:, cols] != want[:, cols]).any(axis=1))[0]
    if not len(bad):
        return None
    r = int(bad[0])
    f = [(WP.FIELDS[c], int(got[r, c]), int(want[r, c])) for c in cols if got[r, c] != want[r, c]]
    return f"{len(bad)} of {len(cases)} cases differ; first: {dict(zip(WP.CASE, cases[r].tolist()))}: (field, got, want) {f}"


def test_the_planner_reproduces_the_recorded_plans(tables):
    cases, got, want = tables
    assert len(WP.FIELDS) == want.shape[1] and len(cases) > 50000
    # the fixture is worth something: refusals, both families, merged and separate launches, short h sources
    F = {f: i for i, f in enumerate(WP.FIELDS)}
    assert set(want[:, F["rc"]].tolist()) == {0, -2}
    assert set(want[:, F["launch0.family"]].tolist()) == {0, 4, 8} and set(want[:, F["n_launch"]].tolist()) == {0, 1, 2}
    assert set(want[:, F["launch0.nparts"]].tolist()) == {0, 1, 2}
    cols = [c for c in range(len(WP.FIELDS)) if WP.FIELDS[c] != "workspace_bytes"]
    assert _first_difference(cases, got, want, cols) is None, _first_difference(cases, got, want, cols)


def test_the_workspace_query_reproduces_the_recorded_sizes(tables):
    cases, got, want = tables
    c = WP.FIELDS.index("workspace_bytes")
    assert _first_difference(cases, got, want, [c]) is None, _first_difference(cases, got, want, [c])
    # a refused layer is refused by the query too (0 bytes: SeqEngine.untrainable_layers), and only then
    assert np.array_equal(want[:, c] == 0, want[:, 0] != 0)


# ------------------------------------------------------------------------------ the KEYS of the exact-reduction GPU test
def _instances(lib, bf16, Cx, Ch, k, xfold, wide):
    """the instances the launches of one layer run: (dtype, family, KS, NTC, JW, KX) per launch"""
    from nasa_niswan_amd._lib import NintGeom, NintWgradPlanRec
    ly = WP.layer_of(Cx, Ch, k, bf16, xfold, wide)
    g = NintGeom()
    assert lib.nint_geom_make(C.byref(g), 37, 50, max(k // 2, 1)) == 0
    out = NintWgradPlanRec()
    rc = lib.nint_debug_wgrad_plan(C.byref(ly), C.byref(g), bf16, 7, 0, 256, C.byref(out))
    if rc != 0:
        return rc, set()
    return 0, {("bf16" if bf16 else "f32", l.family, l.KS, l.NTC, l.JW, l.KX) for l in out.launch[:out.n_launch]}


def _named(name):
    """the instance a KEYS case names: 'bf16 folded (5,2,5,1) 5->64' or 'bf16 8-wave <3,4> 64->64'"""
    dt = name.split()[0]
    m = re.search(r"\((\d),(\d),(\d),(\d)\)", name)
    if m:
        k, ntc, jw, kx = (int(v) for v in m.groups())
        return (dt, 4, k, ntc, jw, kx)
    m = re.search(r"8-wave <(\d),(\d)>", name)
    return (dt, 8, int(m.group(1)), int(m.group(2)), 0, int(m.group(1)))


def test_exact_reduction_cases_run_every_reachable_instance(lib):
    """Every layer shape the engine can build (channels padded by nint_kc, any odd k, plain or folded x source, either family):
    the instances its launches reach.  Each must be named by a KEYS case, and each case must reach the instance it names."""
    reach = set()
    for bf16 in (1, 0):
        kc = lib.nint_kc(bf16)
        seen = set()
        for Cx in range(1, 129):
            for Ch in range(4, 129, 4):
                for k in (1, 3, 5, 7):
                    for xfold in (0, 1):
                        shape = (WP.rup(k * Cx if xfold else Cx, kc), WP.rup(Ch, 16), WP.rup(Ch, kc), k, xfold)
                        if shape in seen:
                            continue                    # (the planner reads the padded counts only)
                        seen.add(shape)
                        for wide in (0, 1, 2):
                            rc, ins = _instances(lib, bf16, Cx, Ch, k, xfold, wide)
                            assert rc == 0, (bf16, Cx, Ch, k, xfold, wide, rc)
                            reach |= ins
    assert len(reach) == 22 and sum(i[1] == 8 for i in reach) == 3, sorted(reach)
    # bf16 pads channels to 32: a 4-wave instance with one channel tile per block and five columns per wave wants 16 mod 32
    assert not [i for i in reach if i[0] == "bf16" and i[1] == 4 and i[3] == 1 and i[4] == 5]
    named = {}
    for name, (dtype, xfold, wide, Cx, Ch, k) in ER.KEYS.items():
        rc, ins = _instances(lib, int(dtype == "bf16"), Cx, Ch, k, int(xfold), wide)
        assert rc == 0 and _named(name) in ins, (name, _named(name), sorted(ins))
        named[_named(name)] = name
    assert set(named) == reach, ("reachable, but no KEYS case names it", sorted(reach - set(named)), "named, never reached",
                                 sorted(set(named) - reach))
