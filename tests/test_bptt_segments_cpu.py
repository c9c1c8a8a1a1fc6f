"""CPU-only checks of checkpointed BPTT and gradient accumulation: the segment plan, the place of
`nint_seq.accumulate` in the structure, the planner's refusal of a value that is no mode, the new head entries in the header
and the binding, and the two command-line flags.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_plan():
    from nasa_niswan_amd.trainer import segment_plan
    assert segment_plan(6, 1) == [(0, 6)]
    assert segment_plan(6, 2) == [(0, 3), (3, 3)]
    assert segment_plan(6, 3) == [(0, 2), (2, 2), (4, 2)]
    assert segment_plan(6, 6) == [(t, 1) for t in range(6)]
    assert segment_plan(48, 4) == [(0, 12), (12, 12), (24, 12), (36, 12)]
    assert segment_plan(1, 1) == [(0, 1)]
    for T, n in [(6, 4), (6, 5), (6, 7), (48, 5), (1, 2)]:
        with pytest.raises(ValueError, match="divide"):
            segment_plan(T, n)
    for n in (0, -1, -6):
        with pytest.raises(ValueError, match=">= 1"):
            segment_plan(6, n)


def test_accumulate_field_sits_where_the_header_puts_it_and_moves_nothing(tmp_path):
    """offsetof / sizeof through gcc, as tests/test_abi.py compares the rest of the structure.  The field takes the four
    bytes that were padding behind bwd_parts, in front of the 8-byte aligned dh_seq: every other offset and the size of the
    structure are what they were (tests/test_seq_train_cpu.py pins dh_seq as the last field)."""
    from nasa_niswan_amd import _lib
    prog = tmp_path / "acc.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nint.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                    'offsetof(nint_seq,accumulate),offsetof(nint_seq,dh_seq),offsetof(nint_seq,bwd_parts),sizeof(nint_seq),'
                    'sizeof(((nint_seq*)0)->accumulate),offsetof(nint_seq,wave));return 0;}\n')
    exe = tmp_path / "acc"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.NintSeq
    assert got == [S.accumulate.offset, S.dh_seq.offset, S.bwd_parts.offset, C.sizeof(S), 4, S.wave.offset]
    assert S.accumulate.offset == S.bwd_parts.offset + 4 and S.dh_seq.offset == S.accumulate.offset + 4
    assert S.dh_seq.offset % 8 == 0 and S.dh_seq.offset + 8 == C.sizeof(S)       # the padding it took: nothing moved
    assert _lib.NintSeq().accumulate == 0                      # a zero-filled structure means "stored"


def test_planner_refuses_an_accumulate_that_is_no_mode():
    """nint_seq_bwd checks its arguments before it plans or enqueues anything, so the return code can be read on a machine
    without a GPU (tests/test_abi.py).  The structure passes every other argument check and ends at the LAST one, the
    alignment of dh_seq: both modes give E_ALIGN there, so E_ARG can only come from the accumulate check."""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    E_ARG, E_ALIGN = -1, -4
    seq = _lib.NintSeq()
    seq.L, seq.B, seq.T, seq.dtype, seq.xs, seq.h[0], seq.c[0] = 1, 1, 1, 1, 16, 16, 16
    seq.layer[0].k = 1
    seq.gates[0] = seq.dG[0] = seq.dh[0] = seq.dc[0] = seq.dW[0] = seq.db[0] = 16
    seq.wg_partial, seq.wg_partial_bytes = 16, 1 << 20
    seq.dh_seq = 24                                             # not 16-byte aligned
    for ok in (0, 1):
        seq.accumulate = ok
        assert lib.nint_seq_bwd(C.byref(seq), None) == E_ALIGN, ok
        assert lib.nint_debug_seq_plan(C.byref(seq), 1, None, 0) == E_ALIGN, ok
    for bad in (2, -1, 3, 1 << 20):
        seq.accumulate = bad
        assert lib.nint_seq_bwd(C.byref(seq), None) == E_ARG, bad
        assert lib.nint_debug_seq_plan(C.byref(seq), 1, None, 0) == E_ARG, bad
        for parts in (1, 2):
            seq.bwd_parts = parts
            assert lib.nint_seq_bwd(C.byref(seq), None) == E_ARG, (bad, parts)
        seq.bwd_parts = 0
    # the forward driver does not read the field
    seq.xs = 24
    assert lib.nint_seq_fwd(C.byref(seq), None) == E_ALIGN


def test_head_entries_are_declared_bound_and_check_their_switch():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nint.h")).read(), flags=re.S)
    for name, nargs in (("nint_head_bwd_acc", 17), ("nint_head_bwd_seq_acc", 18), ("nint_head_bwd", 16), ("nint_head_bwd_seq", 17)):
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name      # the old entries keep their signatures
        assert hasattr(lib, name)
    assert "#define NINT_VERSION 113" in src and _lib.NINT_VERSION == 113       # (113: nint_debug_wgrad_plan was added)
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 9, 17, 2) == 0
    E_ARG, E_ALIGN = -1, -4
    for bad in (2, -1):
        assert lib.nint_head_bwd_acc(16, 0, 2, 8, 32, 1, 16, 16, None, 16, 16, bad, C.byref(g), 1, None, 0, None) == E_ARG
        assert lib.nint_head_bwd_seq_acc(16, 2, 2, 8, 32, 1, 16, 16, None, 16, 16, 16, bad, C.byref(g), 1, None, 0, None) == E_ARG
    # ... and with a mode the sequence entry goes on to its next check, the alignment of the h slab
    for ok in (0, 1):
        assert lib.nint_head_bwd_seq_acc(24, 2, 2, 8, 32, 1, 16, 16, None, 16, 16, 16, ok, C.byref(g), 1, None, 0, None) == E_ALIGN


def test_train_py_parses_both_flags(tmp_path, monkeypatch):
    from nasa_niswan_amd import train as T
    monkeypatch.delenv("RANK", raising=False)
    a = T.get_arguments(["--snapshot-dir", str(tmp_path / "a")])
    assert a.bptt_segments is None and a.accumulate_steps == 1
    a = T.get_arguments(["--snapshot-dir", str(tmp_path / "b"), "--bptt-segments", "4", "--accumulate-steps", "3",
                         "--sequence-length", "48"])
    assert a.bptt_segments == 4 and a.accumulate_steps == 3 and a.sequence_length == 48
    with pytest.raises(SystemExit):
        T.get_arguments(["--snapshot-dir", str(tmp_path / "c"), "--bptt-segments", "two"])
