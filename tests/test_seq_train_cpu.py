"""CPU-only checks of the differentiable return_sequence path (training on the per-step head outputs): the new nint_seq field
and the three sequence head / loss entries at the boundary, the BPTT launch plan with a per-step top-layer gradient
(nint_seq.dh_seq) against the plan without it, and the datasets' sequence targets.  Nothing here touches a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_launch_plan_cpu as TLP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


def test_dh_seq_field_layout_matches_header(tmp_path):
    """offsetof(nint_seq, dh_seq) and sizeof(nint_seq) from gcc equal the ctypes values; the field is the last one."""
    from nasa_niswan_amd import _lib
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nint.h"\nint main(){printf("%zu %zu %zu\\n",'
                    'offsetof(nint_seq,dh_seq),sizeof(nint_seq),offsetof(nint_seq,bwd_parts));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [_lib.NintSeq.dh_seq.offset, C.sizeof(_lib.NintSeq), _lib.NintSeq.bwd_parts.offset]
    assert _lib.NintSeq._fields_[-1][0] == "dh_seq" and _lib.NintSeq.dh_seq.offset > _lib.NintSeq.bwd_parts.offset
    assert _lib.NintSeq.dh_seq.offset + C.sizeof(C.c_void_p) == C.sizeof(_lib.NintSeq)


def test_sequence_entries_exist_and_reject_bad_arguments_without_a_gpu():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    for name in ("nint_head_fwd_seq", "nint_head_bwd_seq", "nint_head_loss_seq_fused"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.nint_version() == 113
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), 12, 20, 1) == 0
    gp = C.byref(g)
    A = 4096                                    # a made-up aligned address: every call below is refused before it is read
    B, T, Ch, Chp, O = 2, 4, 8, 16, 3
    # forward: NULL slab / weights / output, sizes, dtype, a padding that is not the storage type's
    f = lib.nint_head_fwd_seq
    assert f(None, B, T, Ch, Chp, O, A, A, A, gp, 0, None) == E_ARG
    assert f(A, B, T, Ch, Chp, O, None, A, A, gp, 0, None) == E_ARG
    assert f(A, B, T, Ch, Chp, O, A, A, None, gp, 0, None) == E_ARG
    assert f(A, B, T, Ch, Chp, O, A, A, A, None, 0, None) == E_ARG
    assert f(A, 0, T, Ch, Chp, O, A, A, A, gp, 0, None) == E_ARG
    assert f(A, B, 0, Ch, Chp, O, A, A, A, gp, 0, None) == E_ARG
    assert f(A, B, T, Ch, Chp, 0, A, A, A, gp, 0, None) == E_ARG
    assert f(A, B, T, Ch, Chp, O, A, A, A, gp, 7, None) == E_ARG
    assert f(A, B, T, Ch, 16, O, A, A, A, gp, 1, None) == E_ARG          # bf16 slabs are padded to 32 channels
    assert f(A, B, T, 24, 16, O, A, A, A, gp, 0, None) == E_ARG          # Chp < Ch
    assert f(A + 8, B, T, Ch, Chp, O, A, A, A, gp, 0, None) == E_ALIGN
    # backward: at least one cotangent; dw and db together; something to produce
    b = lib.nint_head_bwd_seq
    assert b(A, B, T, Ch, Chp, O, A, None, None, A, A, A, gp, 0, None, 0, None) == E_ARG
    assert b(None, B, T, Ch, Chp, O, A, A, A, A, A, A, gp, 0, None, 0, None) == E_ARG
    assert b(A, B, T, Ch, Chp, O, None, A, A, A, A, A, gp, 0, None, 0, None) == E_ARG
    assert b(A, B, T, Ch, Chp, O, A, A, None, A, A, None, gp, 0, None, 0, None) == E_ARG
    assert b(A, B, T, Ch, Chp, O, A, A, None, None, None, None, gp, 0, None, 0, None) == E_ARG
    assert b(A, B, T, Ch, Chp, O, A, None, A, A, A, A, gp, 3, None, 0, None) == E_ARG
    assert b(A, B, T, Ch, Chp, O, A, A, None, A + 4, A, A, gp, 0, None, 0, None) == E_ALIGN
    # fused head + loss: every pointer, the crop inside the grid, the width limit, alignment
    h = lib.nint_head_loss_seq_fused
    ok = [A, B, T, Ch, Chp, O, A, A, A, A, A, A, A, gp, 1, 2, 10, 16, 0, None]
    for i in (0, 6, 8, 9, 10, 11, 13):
        bad = list(ok)
        bad[i] = None
        assert h(*bad) == E_ARG, i
    for i, v in ((1, 0), (2, -1), (5, 0), (18, 2), (14, 3), (15, 5), (16, 0)):   # B, T, O, dtype, crop rows / columns beyond the grid, empty crop
        bad = list(ok)
        bad[i] = v
        assert h(*bad) == E_ARG, (i, v)
    wide = list(ok)
    wide[3], wide[4] = 136, 144
    assert h(*wide) == E_SHAPE                                           # beyond the fused kernel: the three separate entries
    mis = list(ok)
    mis[11] = A + 4                                                      # loss_out: 8-byte aligned
    assert h(*mis) == E_ALIGN
    mis = list(ok)
    mis[10] = A + 8                                                      # dh_seq: 16-byte aligned
    assert h(*mis) == E_ALIGN


S1 = dict(C=4, hidden=[8], ks=[3], B=2, T=4, H=12, W=20)
S3 = dict(C=5, hidden=[64, 32, 16], ks=[5, 3, 3], B=2, T=4, H=12, W=20)
BENCH = dict(TLP.BENCH, B=8)


def _bwd_plan(s):
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    cap = 4 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    n = lib.nint_debug_seq_plan(C.byref(s), 1, recs, cap)
    if n < 0:
        return n
    assert n <= cap
    return [tuple(getattr(r, f) for f, _ in _lib.NintLaunchRec._fields_) for r in recs[:n]]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fuse", [0, 1, 2])
@pytest.mark.parametrize("wave", [0, 1, 4, 5])
@pytest.mark.parametrize("shape", ["S1", "S3", "bench"])
def test_plan_with_a_per_step_gradient_is_the_plan_without(shape, wave, fuse, dtype):
    """Both addends enter through runtime pointers of bodies that exist, so the BPTT plan with an aligned dh_seq is record for
    record the one with NULL: the same kernels, bodies, grids and merged grids in the same order (not only the same
    (op, layer, t) sequence).  A misaligned dh_seq is refused with NINT_E_ALIGN before anything is planned."""
    case = dict(S1=S1, S3=S3, bench=BENCH)[shape]
    kw = dict(case, dtype=dtype, wave=wave, fuse=fuse, need_dx=False)
    kw["C_"] = kw.pop("C")
    for need_dx in (False, True):
        kw["need_dx"] = need_dx
        s = TLP._seq_of(**kw)
        base = _bwd_plan(s)
        assert isinstance(base, list) and len(base) >= case["T"]
        s.dh_seq = 1 << 31
        with_seq = _bwd_plan(s)
        assert isinstance(with_seq, list) and len(with_seq) == len(base)
        assert [r[2:5] for r in with_seq] == [r[2:5] for r in base]         # (op, layer, t)
        assert with_seq == base
        for off in (1, 4, 8):
            s.dh_seq = (1 << 31) + off
            assert _bwd_plan(s) == E_ALIGN, off
        # ... and in either half of a two-part backward (part 2 plans no BPTT launch at all)
        s.dh_seq = 1 << 31
        s.bwd_parts = 1
        assert _bwd_plan(s) == base
        s.bwd_parts = 2
        assert _bwd_plan(s) == []


def test_window_with_sequence_targets_returns_every_step():
    from nasa_niswan_amd.dataset import E33OMA90D_CRNN, SyntheticE33OMA_CRNN
    kw = dict(padding=(14, 22), in_channels=5, sequence_length=4, n_steps=40, grid=(10, 16), device="cpu", seed=5)
    last = SyntheticE33OMA_CRNN("train", **kw)
    every = SyntheticE33OMA_CRNN("train", sequence_targets=True, **kw)
    assert not last.sequence_targets and every.sequence_targets and len(last) == len(every)
    assert every.y_mean == last.y_mean and every.y_std == last.y_std
    for i in (0, 3, len(every) - 1):
        t0 = int(every.first[i])
        xs, y = every.window(i)
        xs0, y0 = last.window(i)
        assert y.shape == (4, 1, 10, 16) and np.array_equal(y, every.yraw[t0:t0 + 4])
        assert np.array_equal(y[-1], y0) and np.array_equal(y0, last.yraw[t0 + 3])
        assert all(np.array_equal(a, b) for a, b in zip(xs, xs0))
    rng = np.random.default_rng(0)
    n, H, W = 30, 6, 8
    u, v, om, conc = (rng.standard_normal((n, 2, H, W)).astype(np.float32) for _ in range(4))
    prec, src = (rng.standard_normal((n, H, W)).astype(np.float32) for _ in range(2))
    ds = E33OMA90D_CRNN.from_arrays(u, v, om, prec, src, conc, period="train", padding=(8, 10), sequence_length=3,
                                    device="cpu", pinned=False, sequence_targets=True)
    _, y = ds.window(2)
    assert y.shape == (3, 2, H, W) and np.array_equal(y, conc[2:5])
    ds0 = E33OMA90D_CRNN.from_arrays(u, v, om, prec, src, conc, period="train", padding=(8, 10), sequence_length=3,
                                     device="cpu", pinned=False)
    assert np.array_equal(ds0.window(2)[1], conc[4])
