"""oracle/wgrad_audit.py on the CPU: the reference equals autograd of the oracle's cell, the exact-integer budget refuses what
f32 cannot hold exactly, and both checks fail for the wiring mistakes a weight-gradient reduction can make.

The exact check (integer data, bit-equal) is what sees a dropped pixel tile or a doubled split: on real data such a mistake
moves a dW element by less than the rigorous bound gamma_n sum |dG||cat| allows at the bench geometry, so the bound audit is
NOT asked to see it.  The bound audit is asked to see the mistakes that move whole sums: the h source one time step off, the
wrong skip, two swapped taps and an off-by-one fold column map."""
import math

import pytest
import torch

from oracle import convlstm_oracle as O
from oracle import stored_audit as SA
from oracle import wgrad_audit as WA

# the ragged case: B = 3, T = 3 (9 images) of 37 x 50, a folded 5 -> 16 k5 first layer (cfg1-refpinned's layer 0, narrower)
B, T, H, W, Cx, Ch, k = 3, 3, 37, 50, 5, 16, 5


def _autograd(x, h, dG, k, has_init, B):
    """dW, db of sum_t <preact_t, dG_t> through the oracle's cell (model.py:216-231) in f64"""
    N, Cx = x.shape[:2]
    Ch = h.shape[1]
    Wt = torch.zeros(4 * Ch, Cx + Ch, k, k, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(4 * Ch, dtype=torch.float64, requires_grad=True)
    loss = 0
    for t in range(N // B):
        sl = slice(t * B, (t + 1) * B)
        hp = h[sl] if (t > 0 or has_init) else torch.zeros_like(h[sl])
        pre = []
        O.cell_forward(x[sl], hp, torch.zeros_like(hp), Wt, bt, preact=pre)
        loss = loss + (pre[0] * dG[sl]).sum()
    loss.backward()
    return Wt.grad, bt.grad


@pytest.mark.parametrize("has_init", [False, True])
@pytest.mark.parametrize("xfold", [False, True])
def test_reference_equals_autograd_of_the_cell(xfold, has_init):
    g = torch.Generator().manual_seed(1 + 2 * xfold + has_init)
    Bq, Tq, Hq, Wq, Cq, Chq, kq = 2, 3, 6, 9, 3, 4, 3
    x = torch.randn(Tq * Bq, Cq, Hq, Wq, generator=g, dtype=torch.float64)
    h = torch.randn((Tq + 1) * Bq, Chq, Hq, Wq, generator=g, dtype=torch.float64)
    dG = torch.randn(Tq * Bq, 4 * Chq, Hq, Wq, generator=g, dtype=torch.float64)
    if xfold:
        # through a folded f32 slab and back: the reference is fed the unfolded values the folded slab encodes
        geo = SA.Geo.make(Bq, Tq, Hq, Wq, [(Cq, Chq, kq, True)], 4)
        xr = SA.read_xs(geo, SA.write_xs(geo, x.float())).double()
        assert torch.equal(xr, x.float().double())
        x = xr
    dW_a, db_a = _autograd(x, h, dG, kq, has_init, Bq)
    dW, db = WA.wgrad_ref(dG, x, h, kq, xfold=xfold, has_init=has_init, B=Bq)
    assert dW.shape == dW_a.shape and db.shape == db_a.shape
    assert torch.allclose(dW, dW_a, rtol=1e-12, atol=1e-12) and torch.allclose(db, db_a, rtol=1e-12, atol=1e-12)


def test_exact_budget():
    with pytest.raises(AssertionError):
        WA.exact_budget(200, 190, 298)                 # 22.6 M >= 2^24
    with pytest.raises(AssertionError):
        WA.exact_budget(96, 100, 154, dG_max=1, src_max=128)
    # every case of tests/test_gpu_exact_reductions.py
    assert WA.exact_budget(96, 100, 154) == 2956800    # bench stack / cfg4 layer 0, and the product path B = 8, T = 12
    assert WA.exact_budget(48, 190, 298) == 5435520    # the cfg3 layer
    for N, Hq, Wq in ((1, 37, 50), (7, 37, 50), (8, 100, 154), (8, 190, 298), (1, 100, 154)):
        WA.exact_budget(N, Hq, Wq)


def _tile_mask(N, Hq, Wq, PR, t0, t1):
    """pixels of the pixel tiles t0 .. t1-1 in the kernel's tile order (image, tile row of PR rows, tile column of 32)"""
    tx, ty = math.ceil(Wq / 32), math.ceil(Hq / PR)
    m = torch.zeros(N, 1, Hq, Wq, dtype=torch.float64)
    for t in range(t0, t1):
        n, r = divmod(t, tx * ty)
        y, xx = divmod(r, tx)
        m[n, :, y * PR:(y + 1) * PR, xx * 32:(xx + 1) * 32] = 1
    return m


def _swap_taps(dW, c0=0, a=(0, 0), b=(0, 1)):
    out = dW.clone()
    out[:, c0:c0 + 16, a[0], a[1]] = dW[:, c0:c0 + 16, b[0], b[1]]
    out[:, c0:c0 + 16, b[0], b[1]] = dW[:, c0:c0 + 16, a[0], a[1]]
    return out


def _xfold_off_by_one(dW, Cx, k):
    """the fold kernel's map (ky, kx*Cx + c) -> W[.][c][ky][kx] read one folded column too far"""
    out = dW.clone()
    xp = dW[:, :Cx].permute(0, 2, 3, 1).reshape(dW.shape[0], k, k * Cx)     # [o][ky][kx*Cx + c]
    sh = torch.zeros_like(xp)
    sh[..., :-1] = xp[..., 1:]
    out[:, :Cx] = sh.reshape(dW.shape[0], k, k, Cx).permute(0, 3, 1, 2)
    return out


def _mutations(dG, x, h, has_init):
    """(name, dW, db) of each simulated kernel mistake"""
    N = dG.shape[0]
    ref_W, ref_b = WA.wgrad_ref(dG, x, h, k, xfold=True, has_init=has_init, B=B)
    tile = _tile_mask(N, H, W, 4, 2 * 20 + 9, 2 * 20 + 10)        # image 2, tile row 4, the ragged tile column 1
    dW_t, db_t = WA.wgrad_ref(dG * (1 - tile), x, h, k, has_init=has_init, B=B)
    split = _tile_mask(N, H, W, 4, 13, 31)                          # a split of 18 tiles across images 0 and 1
    dW_s, db_s = WA.wgrad_ref(dG * split, x, h, k, has_init=has_init, B=B)
    dW_o, _ = WA.wgrad_ref(dG, x, h[B:], k, has_init=has_init, B=B)  # h_t instead of h_{t-1}
    dW_k, _ = WA.wgrad_ref(dG, x, h, k, has_init=not has_init, B=B)
    _, db_m = WA.wgrad_ref(dG[B:], x[B:], h[B:], k, has_init=True, B=B)
    return [("dropped tile", dW_t, db_t), ("doubled split", ref_W + dW_s, ref_b + db_s), ("swapped taps", _swap_taps(ref_W), ref_b),
            ("h offset by one step", dW_o, ref_b), ("wrong skip", dW_k, ref_b), ("db missing the first images", ref_W, db_m),
            ("xfold map off by one", _xfold_off_by_one(ref_W, Cx, k), ref_b)]


def _slabs(gen, integer):
    if integer:
        return (WA.int_values((T * B, 4 * Ch, H, W), WA.DG_MAX, gen), WA.int_values((T * B, Cx, H, W), WA.SRC_MAX, gen),
                WA.int_values(((T + 1) * B, Ch, H, W), WA.SRC_MAX, gen))
    return (0.1 * torch.randn(T * B, 4 * Ch, H, W, generator=gen), torch.randn(T * B, Cx, H, W, generator=gen),
            0.5 * torch.randn((T + 1) * B, Ch, H, W, generator=gen))


@pytest.mark.parametrize("has_init", [False, True])
def test_exact_check_fails_every_mutation(has_init):
    dG, x, h = _slabs(torch.Generator().manual_seed(7), True)
    WA.exact_budget(T * B, H, W)
    ref_W, ref_b = WA.wgrad_ref(dG, x, h, k, xfold=True, has_init=has_init, B=B)
    # a kernel output equal to the reference passes, in any f32 summation order
    f32_W, f32_b = WA._tap_sums(dG, x, h, k, has_init, B, dtype=torch.float32)
    assert torch.equal(f32_W, ref_W.float()) and torch.equal(f32_b, ref_b.float())
    for name, dW, db in _mutations(dG, x, h, has_init):
        if name == "wrong skip" and has_init:
            continue                     # (skip B where 0 is right: the same mutation seen from the other side, kept below)
        same = torch.equal(dW.float(), ref_W.float()) and torch.equal(db.float(), ref_b.float())
        assert not same, f"the exact check misses: {name}"
    if has_init:
        dW_k, _ = WA.wgrad_ref(dG, x, h, k, has_init=False, B=B)
        assert not torch.equal(dW_k.float(), ref_W.float())


@pytest.mark.parametrize("es", [2, 4])
def test_bound_audit_fails_the_wiring_mutations_and_passes_another_order(es):
    dG, x, h = _slabs(torch.Generator().manual_seed(11), False)
    has_init = False
    rW, rb = WA.wgrad_bound(dG, x, h, k, es, has_init=has_init, B=B)
    f32_W, f32_b = WA._tap_sums(dG, x, h, k, has_init, B, dtype=torch.float32)
    assert WA.bound_ratio(f32_W, rW) <= 1.0 and WA.bound_ratio(f32_b, rb) <= 1.0
    muts = {name: (dW, db) for name, dW, db in _mutations(dG, x, h, has_init)}
    worst = {}
    for name in ("h offset by one step", "wrong skip", "swapped taps", "xfold map off by one"):
        dW, db = muts[name]
        worst[name] = max(WA.bound_ratio(dW.float(), rW), WA.bound_ratio(db.float(), rb))
        assert worst[name] > 1.0, (name, worst[name])
    print("  bound audit, err/bound of the wiring mutations: " + ", ".join(f"{n} {r:.0f}" for n, r in worst.items()))
    # (a dropped tile or a doubled split is the exact check's job: no assertion on their ratio here)
