"""The probe stream of a backward pass, stamp for stamp (nint_seq.probe, include/nint.h).

nint_seq_bwd plans the BPTT chain, one weight-gradient reduction per layer and their fold as ONE list of steps, and the
executor brackets each step.  With every kind in the mask the backward half of the buffer must therefore read, in order:
the calibration pair; one begin / end pair per enqueue index of nint_debug_seq_plan(bwd = 1), with the kind and tags the
schedule rules of csrc/seq.hip give that step; one NINT_PROBE_WGRAD pair per reduction, tagged with its index among the
reductions of THIS call (not the layer); one NINT_PROBE_FOLD pair; and nothing after.  bwd_parts = 1 reduces layers >= 1
behind the chain and bwd_parts = 2 only layer 0, each call with its own fold, and together they must leave the bits of a
whole pass in every dW / db.

The smallest stack that has everything: two layers (3 -> 16 -> 16, 3 x 3), B = 1, T = 2, a 9 x 40 grid."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SLOTS = 512
CAL, POINTWISE, DGRAD, FUSED, WGRAD, FOLD, BWD_PAIR, BWD_PW = 0, 2, 3, 4, 5, 6, 8, 9        # NINT_PROBE_*
OP_DGRAD, OP_FUSED, OP_POINTWISE = 1, 2, 3                                                  # NINT_OP_*


def _pairs(*tags):
    return [(k, l, t, e) for k, l, t in tags for e in (0, 1)]


def _chain_tags(lib, s):
    """(kind, tag layer, tag t) of every step of the planned BPTT chain, from its problems: a lone launch is bracketed as what
    it is; a grid of two conv launches as NINT_PROBE_BWD_PAIR with the tags of the second one (the held-back bottom dgrad is
    the first); a fused step with the bottom layer's pointwise backward as NINT_PROBE_BWD_PW with the fused step's tags"""
    from nasa_niswan_amd import _lib
    cap = 4 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    n = lib.nint_debug_seq_plan(C.byref(s), 1, recs, cap)
    assert 0 < n <= cap, n
    steps = {}
    for r in recs[:n]:
        steps.setdefault(r.index, []).append((r.op, r.layer, r.t))
    assert sorted(steps) == list(range(len(steps)))
    tags = []
    for i in range(len(steps)):
        ps = steps[i]
        if len(ps) == 1:
            tags.append(({OP_POINTWISE: POINTWISE, OP_DGRAD: DGRAD, OP_FUSED: FUSED}[ps[0][0]],) + ps[0][1:])
        elif any(op == OP_POINTWISE for op, _, _ in ps):
            tags.append((BWD_PW,) + [p for p in ps if p[0] == OP_FUSED][0][1:])
        else:
            tags.append((BWD_PAIR,) + ps[-1][1:])
    return tags


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_backward_probe_stream_and_parts(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import bench
    from nasa_niswan_amd.engine import LayerCfg, SeqEngine
    cfgs, B, T, H, W = [LayerCfg(3, 16, 3), LayerCfg(16, 16, 3)], 1, 2, 9, 40
    eng = SeqEngine(cfgs, dtype, "cuda")
    g = torch.Generator().manual_seed(7)
    eng.pack_weights([0.2 * torch.randn(4 * c.Ch, c.Cx + c.Ch, c.k, c.k, generator=g).cuda() for c in cfgs],
                     [0.1 * torch.randn(4 * c.Ch, generator=g).cuda() for c in cfgs])
    X = torch.randn(B, T, 3, H, W, generator=g).cuda()
    dstate = [(0.1 * torch.randn(B, c.Ch, H, W, generator=g).cuda(), 0.1 * torch.randn(B, c.Ch, H, W, generator=g).cuda()) for c in cfgs]
    buf = torch.zeros(2 * SLOTS, dtype=torch.int64, device="cuda")
    ws = eng.acquire(B, T, H, W, True, False)

    def run(parts, reset_state=True):
        """one nint_seq_bwd call on fresh destinations; returns (the backward half's stamps, dW, db)"""
        if reset_state:                             # (the chain consumes dh / dc in place)
            for l, (dh, dc) in enumerate(dstate):
                eng.set_state_grads(ws, l, dh, dc)
        buf.zero_()
        dW = [torch.full((4 * c.Ch, c.Cx + c.Ch, c.k, c.k), float("nan"), device="cuda") for c in cfgs]
        db = [torch.full((4 * c.Ch,), float("nan"), device="cuda") for c in cfgs]
        eng.backward(ws, False, parts=parts, dW_out=dW, db_out=db)
        torch.cuda.synchronize()
        w = buf.cpu().numpy()
        assert not w[:SLOTS].any()                  # the forward half belongs to nint_seq_fwd
        tab = bench.probe_table(w[SLOTS:])
        assert not w[SLOTS + 2 * len(tab):].any()   # nothing after the last stamp
        ticks = [r[4] for r in tab]
        assert all(b >= a for a, b in zip(ticks, ticks[1:])) and ticks[-1] > ticks[0]
        return [r[:4] for r in tab], dW, db

    try:
        eng.forward(ws, X)
        ws.seq.probe, ws.seq.probe_mask, ws.seq.probe_slots = buf.data_ptr(), 0x3fe, SLOTS
        whole, dW0, db0 = run(0)
        chain = _chain_tags(eng.lib, ws.seq)
        assert len(chain) >= T
        head = _pairs((CAL, 0, 0), *chain)
        assert whole == head + _pairs((WGRAD, 0, 0), (WGRAD, 1, 0), (FOLD, 0, 0))
        for x in dW0 + db0:
            assert not torch.isnan(x).any()
        # layers >= 1 behind the chain (ONE reduction: index 0 is layer 1's), then layer 0 by itself; each call folds its own
        first, dW1, db1 = run(1)
        assert first == head + _pairs((WGRAD, 0, 0), (FOLD, 0, 0))
        assert torch.isnan(dW1[0]).all() and torch.isnan(db1[0]).all()
        second, dW2, db2 = run(2, reset_state=False)
        assert second == _pairs((CAL, 0, 0), (WGRAD, 0, 0), (FOLD, 0, 0))
        assert torch.isnan(dW2[1]).all() and torch.isnan(db2[1]).all()
        assert torch.equal(dW2[0], dW0[0]) and torch.equal(db2[0], db0[0])
        assert torch.equal(dW1[1], dW0[1]) and torch.equal(db1[1], db0[1])
    finally:
        ws.seq.probe, ws.seq.probe_mask, ws.seq.probe_slots = None, 0, 0
        eng.release(ws)
