"""oracle/launch_plan.py (the launch ledger) pinned on rows derived by hand from csrc/conv_igemm.hip (cell_fwd, launch_conv,
launch_cfg, nint_internal_conv_dgrad, nint_internal_multi_plan) and csrc/seq.hip (nint_seq_fwd, nint_seq_bwd); the sweep of
every layer shape the engine accepts, with a reason for each instantiated body it never selects; and the coverage of the GPU
audit: the cases of tests/test_gpu_stored_audit.py and tests/test_gpu_launch_audit.py (their module-level tables, read without
a GPU) together run every reachable body, every 8-row body also with the merged leftover strip, and every host kernel.

The schedule half of the ledger (plan_fwd, plan_bwd, bwd_facts, multi_kernel and everything they call) is also checked against
the library itself: nint_debug_seq_plan runs the drivers' own planner without a GPU, and its records must equal the ledger's,
launch for launch, for every audit case and for the bench stack."""
import ctypes as C
import time

import pytest

from oracle import launch_plan as LP

import test_gpu_launch_audit as LA
import test_gpu_stored_audit as SAT

BENCH = dict(C=62, hidden=[64, 32, 16], ks=[5, 3, 3], T=3, H=100, W=154)


def _rows(launches, pass_, op, layer):
    """(kernel, body, strip, nt_begin) of the launches of one kind and layer; BPTT launches of time u >= 1 only (at u = 0 from
    the zero state there is no d/dh_{-1}: fewer n-tiles)"""
    return {(x.kernel, x.body, x.strip, x.nt_begin) for x in launches
            if (x.pass_, x.op, x.layer) == (pass_, op, layer) and (pass_ == "fwd" or x.t >= 1)}


def test_bench_layers():
    # bf16 (kc 32): 62 * 5 = 310 -> cdiv 10 K-steps folded against cdiv(62, 32) * 5 = 10 plain: no fold, Cxp 64; Ch16 = Chp = 64
    # / 32 / 16 (Chp 32: rounded to kc); f32 (kc 16): 20 against 20, no fold either
    assert LP.layers_of(62, [64, 32, 16], [5, 3, 3], "bf16") == [
        LP.Layer(62, 64, 5, False, 64, 64, 64), LP.Layer(64, 32, 3, False, 64, 32, 32), LP.Layer(32, 16, 3, False, 32, 16, 32)]
    assert LP.layers_of(62, [64, 32, 16], [5, 3, 3], "f32")[2] == LP.Layer(32, 16, 3, False, 32, 16, 16)
    # thin inputs fold: 5 * 5 = 25 channels -> 1 K-step against 5
    assert LP.layers_of(5, [64], [5], "bf16")[0].xfold
    # _set_wave: tiles8 = B * 10 * 13; 5 while 2 * tiles8 < 1.5 * 256 = 384
    assert [LP.default_wave(B, 100, 154, 3) for B in (8, 2, 1)] == [4, 4, 5]


@pytest.mark.parametrize("need_dx", [False, True])
def test_bench_b8_bf16(need_dx):
    ls = LP.plan(**BENCH, B=8, dt="bf16", need_dx=need_dx)
    f = LP.bwd_facts(LP.layers_of(62, [64, 32, 16], [5, 3, 3], "bf16"), "bf16", 4, 0)
    # dgrad K-steps (4*Ch16/32) * k^2: 8*25 = 200, 4*9 = 36, 2*9 = 18: only the top layer is fused (<= 24), and lo[2] (the layer
    # below is classic); wave 4: merge_d (layers 0 and 1 classic), merge_p (the top layer fused)
    assert f.fused == (False, False, True) and f.lo == (False, False, True) and f.off == (1, 1, 1)
    assert f.merge_d and f.merge_p and not f.merge
    # forward, wave 4 = rows8: every gate launch on 8-row tiles (tile_rows pinned: no column split).  NTt = 16 / 8 / 4: cbs = 4
    # -> (4,1,4), 2 -> (2,2,4), 1 -> (1,4,4).  100 % 8 = 4 leftover rows, 10 column tiles: the merged strip; the wavefront's
    # middle steps as conv_lstm_multi8, the first (layer 0, t 0) and last (layer 2, t 2) alone
    strip = {("bf16", "LSTM", 4, 1, 4, 8), ("bf16", "LSTM", 2, 2, 4, 8), ("bf16", "LSTM", 1, 4, 4, 8)}
    gates = [x for x in ls if x.op == "gate"]
    assert {x.body for x in gates} == strip and all(x.strip for x in gates)
    # grid: 8 images * 10 column tiles * 12 full tile rows + 8 * cdiv(10, 2) strip tiles = 1000, one column group
    assert {x.grid for x in gates} == {(1000, 1)}
    assert [(x.layer, x.t, x.kernel) for x in gates if x.kernel == "conv_igemm"] == [(0, 0, "conv_igemm"), (2, 2, "conv_igemm")]
    # layer 0 dgrad: 8 * 10 * 13 = 1040 8-row tiles, 2 * 1040 >= 3 * 256: no small-batch rule; 200 K-steps > 32: 8 rows.
    #   need_dx False: nt_begin = Cxp / 16 = 4, ntiles = Chp / 16 = 4 -> (1,4,4), held back and merged with layer 1's dgrad
    #   (36 K-steps: 8 rows, ntiles 4 + 2 = 6 -> (2,2,3)): the pair (2,2,3,8) + (1,4,4,8) is conv_dgrad_multi8_kernel's.
    #   need_dx True: ntiles 4 + 4 = 8 -> (2,2,4,8), which no merged kernel holds: both launch on their own
    if not need_dx:
        assert _rows(ls, "bwd", "dgrad", 0) == {("conv_dgrad_multi8", ("bf16", "DGRAD", 1, 4, 4, 8), True, 4),
                                                ("conv_bwd_multi8", ("bf16", "DGRAD", 1, 4, 4, 8), True, 4)}
        # (layer 1 at u = 2 has no held-back layer-0 dgrad to pair with)
        assert _rows(ls, "bwd", "dgrad", 1) == {("conv_dgrad_multi8", ("bf16", "DGRAD", 2, 2, 3, 8), True, 0),
                                                ("conv_igemm", ("bf16", "DGRAD", 2, 2, 3, 8), True, 0)}
        # layer 1 at u = 0 from the zero state: x columns only, ntiles 4 -> (1,4,4,8), with layer 0's u = 1 in conv_bwd_multi8
        assert {(x.kernel, x.body) for x in ls if (x.op, x.layer, x.t) == ("dgrad", 1, 0)} == {
            ("conv_bwd_multi8", ("bf16", "DGRAD", 1, 4, 4, 8))}
    else:
        assert _rows(ls, "bwd", "dgrad", 0) == {("conv_igemm", ("bf16", "DGRAD", 2, 2, 4, 8), True, 0)}
        assert _rows(ls, "bwd", "dgrad", 1) == {("conv_igemm", ("bf16", "DGRAD", 2, 2, 3, 8), True, 0)}
    # (need_dx False: the last layer-0 dgrad -- u = 0, zero state, no dx -- launches nothing)
    # top layer fused, 18 K-steps: 4 rows; DGRAD_PW ntiles = Cxp/16 + Ch16/16 = 2 + 1 = 3 -> (1,4,3,4), the middle one with
    # layer 0's pointwise pass of the step before in conv_bwd_multi_kernel
    assert _rows(ls, "bwd", "fused", 2) == {("conv_igemm", ("bf16", "DGRAD_PW", 1, 4, 3, 4), False, 0),
                                            ("conv_bwd_multi", ("bf16", "DGRAD_PW", 1, 4, 3, 4), False, 0)}
    assert [x.kernel for x in ls if x.op == "pointwise" and x.layer == 0].count("conv_bwd_multi") == 1


@pytest.mark.parametrize("need_dx", [False, True])
def test_bench_b2_bf16(need_dx):
    ls = LP.plan(**BENCH, B=2, dt="bf16", need_dx=need_dx)
    # 2 * (2 * 10 * 13) = 520 < 768: every unpinned launch on 4-row tiles, ptiles = 2 * 10 * 25 = 500; the gates stay pinned
    # at 8 rows (wave 4)
    assert {x.body[5] for x in ls if x.op == "gate"} == {8}
    # layer 0: ntiles 4 (need_dx False) -> few(4) = 2*500*1 = 1000 >= 768: (1,4,4,4); layer 1: 6 -> (2,2,3,4); both 4-row
    # shapes of conv_bwd_multi_kernel.  need_dx True: ntiles 8 -> (2,2,4,4), not held: on its own
    if not need_dx:
        assert ("conv_bwd_multi", ("bf16", "DGRAD", 1, 4, 4, 4), False, 4) in _rows(ls, "bwd", "dgrad", 0)
        assert ("conv_bwd_multi", ("bf16", "DGRAD", 2, 2, 3, 4), False, 0) in _rows(ls, "bwd", "dgrad", 1)
    else:
        assert _rows(ls, "bwd", "dgrad", 0) == {("conv_igemm", ("bf16", "DGRAD", 2, 2, 4, 4), False, 0)}


@pytest.mark.parametrize("need_dx", [False, True])
def test_bench_b1_bf16(need_dx):
    ls = LP.plan(**BENCH, B=1, dt="bf16", need_dx=need_dx)
    # wave 5: no rows8; ptiles (4 rows) = 250.  Gate layer 0: cbs 4, few4 = 2*250*1 = 500 < 768, few2 = 1000: (2,2,4,4);
    # layer 1: cbs 2, few2 = 500: (1,4,4,4); layer 2: cbs 1: (1,4,4,4); the wavefront as conv_lstm_multi
    assert {(x.layer, x.body) for x in ls if x.op == "gate"} == {
        (0, ("bf16", "LSTM", 2, 2, 4, 4)), (1, ("bf16", "LSTM", 1, 4, 4, 4)), (2, ("bf16", "LSTM", 1, 4, 4, 4))}
    # dgrad layer 0, ntiles 4: few(4) = 500 < 768 -> next rung 2: few(2) = 1000: (1,4,2,4); layer 1, ntiles 6: few(6) = 500,
    # 6 % 4 != 0, few(3) = 1000: (1,4,3,4); the pair in conv_bwd_multi_kernel.  Layer 2 at u = 0 (zero state: x columns
    # only, ntiles 2): few(2) = 500 -> (1,4,1,4)
    assert ("conv_bwd_multi", ("bf16", "DGRAD", 1, 4, 2, 4), False, 4 if not need_dx else 0) in _rows(ls, "bwd", "dgrad", 0) \
        or need_dx
    assert ("conv_bwd_multi", ("bf16", "DGRAD", 1, 4, 3, 4), False, 0) in _rows(ls, "bwd", "dgrad", 1)
    assert {(x.kernel, x.body) for x in ls if (x.op, x.layer) == ("dgrad", 2)} == {("conv_igemm", ("bf16", "DGRAD", 1, 4, 1, 4))}
    if need_dx:   # ntiles 8: few(8) = 500, few(6): 8 % 6, few(4) = 2*250*2 = 1000: (1,4,4,4)
        assert ("conv_bwd_multi", ("bf16", "DGRAD", 1, 4, 4, 4), False, 0) in _rows(ls, "bwd", "dgrad", 0)


def test_bench_b8_f32():
    ls = LP.plan(**BENCH, B=8, dt="f32", need_dx=False)
    f = LP.bwd_facts(LP.layers_of(62, [64, 32, 16], [5, 3, 3], "f32"), "f32", 4, 0)
    # f32 K-steps (4*Ch16/16) * k^2: 16*25 = 400, 8*9 = 72, 4*9 = 36: nothing fused, so no merge_p
    assert f.fused == (False, False, False) and f.merge_d and not f.merge_p
    # layer 2 dgrad: 36 K-steps -> 8 rows; ntiles Cxp/16 + Chp/16 = 2 + 1 = 3 -> (1,4,3,8)
    assert _rows(ls, "bwd", "dgrad", 2) == {("conv_igemm", ("f32", "DGRAD", 1, 4, 3, 8), True, 0)}
    assert ("conv_dgrad_multi8", ("f32", "DGRAD", 1, 4, 4, 8), True, 4) in _rows(ls, "bwd", "dgrad", 0)


@pytest.mark.parametrize("wave", [4, 5])
def test_tiny_f32_top_layer(wave):
    # 7 -> [16, 8, 8], k [5, 3, 3]: the top layer (Cx 8, Ch 8, k 3) is stencil-shaped and dense-K-shaped in f32
    # (xg = cdiv(8*4, 16) = 2, 9*2 + 9*2 = 36 groups = 9 K-steps <= 12); layer 1 (Cx 16) needs 9*4 + 18 = 54 groups = 14 > 12
    lys = LP.layers_of(7, [16, 8, 8], [5, 3, 3], "f32")
    assert LP.tiny_shape(lys[2], "f32") and not LP.tiny_shape(lys[1], "f32") and LP.tiny_shape(lys[1], "bf16")
    ls = LP.plan(7, [16, 8, 8], [5, 3, 3], 3, 3, 37, 50, "f32", wave=wave)
    top = {x.kernel for x in ls if x.op == "gate" and x.layer == 2}
    if wave == 4:
        # rows8 pins tile_rows 8, and NINT_TINY_AUTO needs tile_rows 0: the top layer runs (1,4,4,8) inside the merged grid
        assert top == {"conv_lstm_multi8", "conv_igemm"}
    else:
        # no rows8: the dense-K kernel has no planned form, so every wavefront step with the top layer falls back to single
        # launches, and the other layers of those steps launch directly
        assert top == {"tiny"}
        assert {x.kernel for x in ls if x.op == "gate" and x.t >= 1 and x.t + 2 - x.layer <= 2 + 2} >= {"tiny", "conv_igemm"}


def test_sweep_reachable_bodies():
    t0 = time.time()
    R = LP.reachable()
    dt = time.time() - t0
    assert dt < 10, dt
    assert set(R) <= LP.INSTANTIATED and len(LP.INSTANTIATED) == 76
    # every instantiated body but the ones recorded with a reason
    assert LP.INSTANTIATED - set(R) == set(LP.UNREACHABLE), sorted(LP.INSTANTIATED - set(R))
    # and every 8-row body the sweep reaches is reached with the merged strip
    assert all(True in R[b] for b in R if b[5] == 8)


def _covered(cases):
    cov, kernels = {}, set()
    for c in cases:
        for x in LP.case_launches(**c):
            kernels.add((c["dtype"], x.kernel))
            if x.body is not None:
                cov.setdefault(x.body, set()).add(x.strip)
    return cov, kernels


def test_gpu_audit_cases_cover_every_reachable_body():
    R = LP.reachable()
    cov, kernels = _covered(SAT.ledger_cases() + LA.ledger_cases())
    missing = sorted(set(R) - set(cov))
    assert not missing, "bodies no audit case runs: " + ", ".join(LP.fmt_body(b) for b in missing)
    no_strip = sorted(b for b in cov if b[5] == 8 and True not in cov[b])
    assert not no_strip, "8-row bodies no audit case runs with the merged strip: " + ", ".join(LP.fmt_body(b) for b in no_strip)
    want = {(d, k) for d in ("bf16", "f32") for k in LP.CARRIERS}
    assert want <= kernels, sorted(want - kernels)


def test_bench_cases_reach_the_bench_kernels():
    # the B = 8 trainer cases of the launch audit run what the issue's bench launches are made of
    for d in ("bf16", "f32"):
        ls = LP.case_launches(**LA.CASES[f"bench B=8 trainer {d}"])
        assert any(x.kernel == "conv_dgrad_multi8" for x in ls)
        assert any(x.body[5] == 8 and x.strip for x in ls if x.op == "dgrad")
        assert all(x.body[5] == 8 and x.strip for x in ls if x.op == "gate")


# ------------------------------------------------------------------------------ the ledger against the library's own planner
EPIS = ("LSTM", "DGRAD", "DGRAD_PW")              # nint_launch_rec.epi
OPS = ("gate", "dgrad", "fused", "pointwise")     # NINT_OP_*


def _seq_of(C_, hidden, ks, B, T, H, W, dtype, wave=None, rows=0, fuse=None, has_init=False, zero=False, need_dx=True, train=True,
            **_):
    """nint_seq as SeqEngine fills it for one run_audit case, with made-up 4096-aligned addresses (the planner reads none)"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    lys = LP.layers_of(C_, hidden, ks, dtype)
    L = len(lys)
    s = _lib.NintSeq()
    s.dtype, s.B, s.T, s.L = (_lib.NINT_BF16 if dtype == "bf16" else _lib.NINT_F32), B, T, L
    s.need_dx, s.has_init_state, s.n_cu = int(need_dx), int(has_init), LP.N_CU
    s.zero_dstate = (1 << (2 * L)) - 1 if zero else 0
    assert lib.nint_geom_make(C.byref(s.g), H, W, max(k // 2 for k in ks)) == 0
    addr = iter(range(1 << 20, 1 << 30, 1 << 20))
    for l, ly in enumerate(lys):
        n = s.layer[l]
        n.Cx, n.Cxp, n.Ch, n.Ch16, n.Chp, n.k, n.xfold, n.tile_rows = ly.Cx, ly.Cxp, ly.Ch, ly.Ch16, ly.Chp, ly.k, int(ly.xfold), rows
        n.Wf, n.Wd, n.bias_p = next(addr), next(addr), next(addr)
        s.h[l], s.c[l] = next(addr), next(addr)
        if train:
            s.gates[l], s.dG[l], s.dh[l], s.dc[l], s.dW[l], s.db[l] = (next(addr) for _ in range(6))
    s.xs, s.dx, s.wg_partial = next(addr), next(addr), next(addr)
    s.wg_partial_bytes = 1 << 30                                    # room for the bottom layer's d/dh (merge_d)
    s.fuse_bwd = 0 if fuse is None else fuse
    wave = LP.default_wave(B, H, W, L) if wave is None else wave
    s.wave = wave if L > 1 else 0
    return s


def _library_plan(s, train):
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    dt = "bf16" if s.dtype == _lib.NINT_BF16 else "f32"
    out = []
    for bwd in ((0, 1) if train else (0,)):
        cap = 4 * (s.T + s.L + 1) * s.L
        recs = (_lib.NintLaunchRec * cap)()
        n = lib.nint_debug_seq_plan(C.byref(s), bwd, recs, cap)
        assert 0 <= n <= cap, n
        for r in recs[:n]:
            assert r.bwd == bwd and r.dtype == s.dtype
            body = (dt, EPIS[r.epi], r.wn, r.wk, r.ntw, r.mt) if r.mt else None
            out.append((r.index, LP.Launch("bwd" if bwd else "fwd", OPS[r.op], r.layer, r.t, LP.CARRIERS[r.kernel], body, bool(r.strip),
                                           (r.gx, r.gy) if body else None, r.nt_begin)))
    return out


def _conformance_cases():
    cases = [(f"launch audit: {k}", v) for k, v in LA.CASES.items()]
    cases += [(f"stored audit {i}: {sorted(c.items())}", c) for i, c in enumerate(SAT.ledger_cases())]
    cases += [(f"bench B={B} need_dx={dx} {d}", dict(BENCH, B=B, dtype=d, need_dx=dx))
              for B in (8, 2, 1) for dx in (False, True) for d in ("bf16", "f32")]
    return cases


@pytest.mark.parametrize("name,case", _conformance_cases(), ids=[n for n, _ in _conformance_cases()])
def test_ledger_equals_the_library_planner(name, case):
    kw = dict(case)
    kw["C_"] = kw.pop("C")
    s = _seq_of(**kw)
    train = case.get("train", True)
    got = _library_plan(s, train)
    want = LP.plan(case["C"], case["hidden"], case["ks"], case["B"], case["T"], case["H"], case["W"], case["dtype"],
                   wave=case.get("wave"), tile_rows=case.get("rows", 0), fuse_bwd=case.get("fuse") or 0,
                   need_dx=case.get("need_dx", True), train=train, has_init=case.get("has_init", False))
    assert len(got) == len(want), (len(got), len(want))
    for i, ((_, g), w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    # problems share an enqueue index exactly where the ledger names a merged kernel for them
    groups = {}
    for idx, g in got:
        groups.setdefault((g.pass_, idx), []).append(g)
    for (pass_, idx), ps in groups.items():
        merged = ps[0].kernel not in ("conv_igemm", "stencil", "tiny", "pointwise")
        assert (len(ps) > 1) == merged and len({p.kernel for p in ps}) == 1, (pass_, idx, ps)


def test_multi_carrier_equals_the_ledger_on_every_list():
    """Which merged kernel carries a set of launches, on EVERY list and not only on the ones a schedule produces: the library's
    rule (nint_debug_multi_carrier: the first kernel whose case list holds every launch, nint_internal_multi_plan) against the
    ledger's independent statement of it (LP.multi_kernel: rows8 / dpair / the two 4-row shapes / the rider rule).  Every
    multiset of 1-3 of the 38 bodies launch_conv instantiates (dtype aside) and every multiset of 4 of the 14 a merged kernel
    holds (a list with any other body has no carrier at any length), each with and without the pointwise rider."""
    from itertools import combinations_with_replacement as multisets
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    variants = sorted({b[1:] for b in LP.INSTANTIATED})
    assert len(variants) == 38 and len(LP.MULTI_HOLDS) == 14 and LP.MULTI_HOLDS <= set(variants)
    lists = [vs for n in (1, 2, 3) for vs in multisets(variants, n)] + list(multisets(sorted(LP.MULTI_HOLDS), 4))

    def carrier(vs, pw):
        flat = [x for (epi, wn, wk, ntw, mt) in vs for x in (EPIS.index(epi), wn, wk, ntw, mt)]
        return lib.nint_debug_multi_carrier((C.c_int32 * len(flat))(*flat), len(vs), int(pw))

    checked, seen = 0, set()
    for vs in lists:
        convs = [LP.Conv(("bf16",) + v, False, 1, 1, 0) for v in vs]
        for pw in (False, True):
            want = LP.multi_kernel(convs, pw)
            got = carrier(vs, pw)
            assert got == (_lib.NINT_E_SHAPE if want is None else LP.CARRIERS.index(want)), (vs, pw, got, want)
            checked += 1
            seen.add(want)
    assert checked == 26078
    assert seen == {None, "conv_lstm_multi", "conv_lstm_multi8", "conv_bwd_multi", "conv_bwd_multi8", "conv_dgrad_multi8"}
    one = ("LSTM", 1, 4, 4, 4)
    assert carrier((), False) == _lib.NINT_E_SHAPE and carrier((one,) * 5, False) == _lib.NINT_E_SHAPE
    assert carrier((one,) * 4, False) == LP.CARRIERS.index("conv_lstm_multi")
    assert lib.nint_debug_multi_carrier(None, 1, 0) == _lib.NINT_E_SHAPE
    # a tuple that is no body (conv_variant would alias it onto one): refused, not looked up
    assert carrier((("LSTM", 1, 4, 4, 5),), False) == carrier((("LSTM", 11, 4, 4, 4),), False) == _lib.NINT_E_SHAPE


def test_backward_plan_checks_the_weight_gradient_workspace():
    """The weight-gradient reductions are steps of the planned backward pass: a split-K workspace too small for them is refused
    by the planner (NINT_E_ARG from nint_debug_seq_plan(bwd = 1) and, before anything is enqueued, from nint_seq_bwd), the
    forward plan does not look at it, and the engine's own sizing -- nint_wgrad_workspace_bytes of every layer, each rounded
    up to 256 bytes -- plans what 1 GiB plans.  (wave = 4 also parks layer 0's d/dh there, B * H * W * Chp elements: where
    the engine's sizing has no room for it the dgrad pair falls away, so the comparison then runs at wave = 2, which reads
    no such room.)"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    s = _seq_of(C_=BENCH["C"], **{k: v for k, v in BENCH.items() if k != "C"}, B=2, dtype="bf16")
    sized = sum((lib.nint_wgrad_workspace_bytes(C.byref(s.layer[l]), s.dtype, s.n_cu) + 255) // 256 * 256 for l in range(s.L))
    assert 0 < sized < s.wg_partial_bytes
    if sized < s.B * BENCH["H"] * BENCH["W"] * s.layer[0].Chp * 2:
        s.wave = 2
    want = _library_plan(s, True)
    assert any(g.pass_ == "bwd" for _, g in want)
    s.wg_partial_bytes = sized
    assert _library_plan(s, True) == want
    s.wg_partial_bytes = 0
    recs = (_lib.NintLaunchRec * len(want))()
    assert lib.nint_debug_seq_plan(C.byref(s), 1, recs, len(want)) == _lib.NINT_E_ARG
    assert _library_plan(s, False) == [x for x in want if x[1].pass_ == "fwd"]
