"""CPU-only checks of the carried-state feature: the data order of truncated BPTT (dataset.stateful_schedule) and the
presence of the state hand-off entry in the header and the binding.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_windows,T,B", [(11, 4, 1), (11, 4, 3), (100, 7, 4), (37, 5, 2), (48, 48, 1), (1, 3, 1), (97, 1, 8),
                                           (433, 48, 2)])
def test_stateful_schedule(n_windows, T, B):
    from nasa_niswan_amd.dataset import stateful_schedule
    sched, dropped = stateful_schedule(n_windows, T, B)
    K = sched.shape[0]
    assert sched.shape == (K, B) and K >= 1 and np.issubdtype(sched.dtype, np.integer)
    assert sched.min() == 0 and sched.max() < n_windows                     # dataset indices
    # every lane's consecutive chunks start T steps apart: the carried state of row k - 1 is the state before row k
    assert (np.diff(sched, axis=0) == T).all()
    # the lanes' record steps [i, i + T) are disjoint, and lane b + 1 starts where lane b ends (contiguous segments)
    steps = np.concatenate([np.arange(i, i + T) for i in sched.T.reshape(-1)])
    assert len(np.unique(steps)) == len(steps) == K * B * T
    assert (steps == np.arange(K * B * T)).all()
    # as many whole rows as the non-overlapping chunks of the n_windows + T - 1 record steps give
    chunks = (n_windows + T - 1) // T
    assert K == chunks // B
    # the tail: the record steps no chunk covers = the windows that start behind the last chunk start
    assert dropped == (n_windows + T - 1) - K * B * T == n_windows - 1 - sched.max() and dropped >= 0


def test_stateful_schedule_refuses_more_lanes_than_chunks():
    from nasa_niswan_amd.dataset import stateful_schedule
    with pytest.raises(ValueError, match="lanes"):
        stateful_schedule(11, 4, 4)             # 14 steps hold 3 chunks of 4
    with pytest.raises(ValueError):
        stateful_schedule(0, 4, 1)
    assert stateful_schedule(11, 4, 3)[0].shape == (1, 3)


def test_state_copy_is_declared_and_bound():
    from nasa_niswan_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nint.h")).read(), flags=re.S)
    for name in ("nint_state_copy", "nint_pack_compact_add"):
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    res, args = _lib.SIGNATURES["nint_state_copy"]
    assert len(args) == 12
    assert "#define NINT_VERSION 113" in src and _lib.NINT_VERSION == 113       # (113: nint_debug_wgrad_plan was added)


def test_state_copy_rejects_bad_arguments_without_a_gpu():
    """argument errors come before any HIP call (the boundary's convention, tests/test_abi.py)"""
    import ctypes as C
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 9, 17, 2) == 0
    V, I = C.c_void_p * 2, C.c_int32 * 2
    a, b = V(1 << 20, 2 << 20), V(3 << 20, 4 << 20)
    c, d = V(5 << 20, 6 << 20), V(7 << 20, 8 << 20)
    chp = I(32, 32)
    E_ARG, E_ALIGN = -1, -4
    assert lib.nint_state_copy(None, b, c, d, chp, 2, 2, 2, None, C.byref(g), 1, None) == E_ARG
    assert lib.nint_state_copy(a, b, c, d, None, 2, 2, 2, None, C.byref(g), 1, None) == E_ARG
    assert lib.nint_state_copy(a, b, c, d, chp, 0, 2, 2, None, C.byref(g), 1, None) == E_ARG
    assert lib.nint_state_copy(a, b, c, d, chp, 9, 2, 2, None, C.byref(g), 1, None) == E_ARG
    assert lib.nint_state_copy(a, b, c, d, chp, 2, 3, 2, None, C.byref(g), 1, None) == E_ARG           # identity needs B_dst == B_src
    assert lib.nint_state_copy(a, b, c, d, chp, 2, 2, 2, I(0, 2), C.byref(g), 1, None) == E_ARG        # lane >= B_src
    assert lib.nint_state_copy(a, b, c, d, chp, 2, 2, 2, I(-2, 0), C.byref(g), 1, None) == E_ARG
    assert lib.nint_state_copy(a, b, a, d, chp, 2, 2, 2, None, C.byref(g), 1, None) == E_ARG           # h source = h destination
    assert lib.nint_state_copy(a, b, c, d, I(32, 16), 2, 2, 2, None, C.byref(g), 1, None) == E_ARG     # 16 channels: no bf16 padding
    assert lib.nint_state_copy(V((1 << 20) + 8, 2 << 20), b, c, d, chp, 2, 2, 2, None, C.byref(g), 1, None) == E_ALIGN
    assert lib.nint_state_copy(a, b, c, V(7 << 20, (8 << 20) + 4), chp, 2, 2, 2, None, C.byref(g), 1, None) == E_ALIGN
