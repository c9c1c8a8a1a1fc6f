"""The comparators of oracle/small_audit.py have teeth (CPU only, no GPU).

For every operation a faithful emulation of the kernel in numpy f32 (each numpy f32 operation rounds once, like the
kernel's; the order of the sums is varied) must pass its comparator, and each plausible kernel bug below must fail it:

  Adam     beta1 used as the lerp weight; bias correction 2 dropped; eps inside the square root; grad_scale not applied
           to the g*g term; step off by one at step 1000
  loss     sign(0) = 1; crop shifted by one row / one column; inv_n from the uncropped count; the R2 constant-target
           value swapped
  head     bias added twice / not at all; channel Ch-1 dropped; outputs o and o+1 swapped; a non-zero pad channel in dh
  layout   the b0 offset of the second preproc chunk dropped; the mode-0 flip taking mean and std from channel c instead
           of C-1-c; pt and pb swapped on an odd pad; fold tap kx mirrored
  skill    a sample of slot -1 added to a map; a sample dropped from its slot; a map cell or a sample row a few ulps off;
           a partial row left out of a sample row; a slot without samples touched

The skill sums' exact model (skill_sums, skill_head_pred) is also PROVED order-free on the integer data sets of
tests/skill_exact_cases.py: evaluated again in Python integers / fractions.Fraction it gives the same numbers exactly.
"""
import fractions

import numpy as np
import pytest

import skill_exact_cases as SX
from oracle import preproc_oracle as PO
from oracle import small_audit as SM

f32 = np.float32


def fails(fn):
    with pytest.raises(SM.AuditError):
        fn()


# --------------------------------------------------------------------------- comparator plumbing
def test_ratio_sees_every_element_and_zero_bounds_mean_equality():
    ref = np.zeros((3, 4))
    got = ref.copy()
    assert SM.ratio(got, ref, np.zeros_like(ref)) == 0.0
    got[2, 3] = 1e-30
    fails(lambda: SM.ratio(got, ref, np.zeros_like(ref)))
    assert SM.ratio(got, ref, np.full_like(ref, 2e-30)) == 0.5
    got[0, 0] = np.nan
    fails(lambda: SM.ratio(got, ref, np.full_like(ref, 1.0)))
    fails(lambda: SM.check_equal(np.array([0.0], f32), np.array([-0.0], f32)))


def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.14159, 0.0], f32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, 0.0], f32)
    SM.check_equal(SM.bf16_round(x), want)
    import torch
    r = np.random.default_rng(0).standard_normal(4096).astype(f32)
    SM.check_equal(SM.bf16_round(r), torch.from_numpy(r).to(torch.bfloat16).float().numpy())
    SM.check_equal(SM.decode_bf16(torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)), SM.bf16_round(r))


def test_bf16_half_ulp_is_the_rounding_bound_and_a_flat_2_pow_minus_9_is_not():
    """one round-to-nearest to bf16 moves a value by up to half an ulp of its binade: 2^-8 |x| just above a power of two,
    2^-9 |x| only just below one.  torch's own conversion shows both ends."""
    import torch
    x = np.array([1.00388, 1.9961], f32)
    r = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    err = np.abs(r.astype(np.float64) - x)
    assert err[0] > 2.0 ** -9 * x[0] and (err <= SM.halfulp_bf16(x)).all()
    assert SM.halfulp_bf16(1.0) == 2.0 ** -8 and SM.halfulp_bf16(1.999) == 2.0 ** -8 and SM.halfulp_bf16(0.0) == 0.0
    v = np.random.default_rng(1).standard_normal(100000).astype(f32) * f32(37.0)
    assert (np.abs(SM.bf16_round(v).astype(np.float64) - v) <= SM.halfulp_bf16(v)).all()
    assert (SM.halfulp_bf16(v) <= 2.0 ** -8 * np.abs(v)).all() and (SM.halfulp_bf16(v) > 2.0 ** -9 * np.abs(v)).all()


# --------------------------------------------------------------------------- Adam
def adam_f32(p, g, m, v, lr, b1, b2, eps, step, gs, form, mut=None):
    """adam_flat_kernel in numpy f32; form 'a' = m + w (g - m), 'b' = g - (g - m)(1 - w)"""
    st = step - 1 if mut == "step_off_by_one" else step
    bc1, bc2 = 1.0 - b1 ** st, 1.0 - b2 ** st
    ss, w1, B2, w2, sb, ep = f32(lr / bc1), f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(np.sqrt(bc2)), f32(eps)
    if mut == "beta1_as_weight":
        w1 = f32(b1)
    if mut == "no_bias_correction2":
        sb = f32(1.0)
    gr = g * f32(gs)
    g2 = g if mut == "grad_scale_not_on_square" else gr
    mi = m + w1 * (gr - m) if form == "a" else gr - (gr - m) * (f32(1.0) - w1)
    vi = v * B2 + (w2 * g2) * g2
    denom = np.sqrt(vi / (sb * sb) + ep) if mut == "eps_inside_sqrt" else np.sqrt(vi) / sb + ep
    return p + (-ss * mi) / denom, mi, vi


def adam_data(seed=1, n=4000):
    rng = np.random.default_rng(seed)
    mags = np.array([0.0, 1e-12, 1e-6, 1.0, 1e4], f32)
    g = (mags[rng.integers(0, 5, n)] * rng.choice([-1.0, 1.0], n) * (0.5 + rng.random(n))).astype(f32)
    p = rng.standard_normal(n).astype(f32)
    m = (g * (0.1 + 0.05 * rng.standard_normal(n))).astype(f32)
    v = (g * g * f32(0.01)).astype(f32)
    m[:50] = 0; v[:50] = 0; g[:50] = 0                          # zero gradient on zero state
    return p, g, m, v


def adam_audit(out, p, g, m, v, lr, b1, b2, eps, step, gs):
    ref = SM.adam(p, g, m, v, lr, b1, b2, eps, step, gs)
    return max(SM.ratio(out[i], *ref[k], what=f"adam {k}") for i, k in enumerate("pmv"))


@pytest.mark.parametrize("b2", [0.999, 0.9])
@pytest.mark.parametrize("b1", [0.9, 0.6, 0.5, 0.0])
@pytest.mark.parametrize("step", [1, 3, 1000])
def test_adam_faithful_emulations_pass(b1, b2, step):
    p, g, m, v = adam_data()
    form = "a" if f32(1.0 - b1) < 0.5 else "b"
    out = adam_f32(p, g, m, v, 1e-3, b1, b2, 1e-8, step, 0.25, form)
    assert adam_audit(out, p, g, m, v, 1e-3, b1, b2, 1e-8, step, 0.25) <= 1.0
    # zero gradient on zero state: nothing moves, and the bound there is zero
    ref = SM.adam(p, g, m, v, 1e-3, b1, b2, 1e-8, step, 0.25)
    assert np.array_equal(out[0][:50], p[:50]) and float(ref["p"][1][:50].max()) == 0.0


def test_adam_reference_is_torch_adam_and_restatement_agrees():
    """the reference of SM.adam is torch.optim.Adam in f64; the numpy chain its bounds are propagated along is the same
    function (the difference is folded into the bound: it must be double rounding noise only)"""
    p, g, m, v = adam_data(2)
    lr, b1, b2, eps, step = 1e-3, 0.9, 0.999, 1e-8, 7
    ref = SM.adam(p, g, m, v, lr, b1, b2, eps, step, 0.5)
    P, G, M, V = (a.astype(np.float64) for a in (p, 0.5 * g, m, v))
    M2, V2 = M + (1 - b1) * (G - M), b2 * V + (1 - b2) * G * G
    P2 = P - lr / (1 - b1 ** step) * M2 / (np.sqrt(V2) / np.sqrt(1 - b2 ** step) + eps)
    for want, k in ((P2, "p"), (M2, "m"), (V2, "v")):
        np.testing.assert_allclose(ref[k][0], want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("mut,b1,step", [("beta1_as_weight", 0.9, 2), ("no_bias_correction2", 0.9, 1), ("eps_inside_sqrt", 0.9, 3),
                                         ("grad_scale_not_on_square", 0.9, 2), ("step_off_by_one", 0.9, 1000),
                                         ("beta1_as_weight", 0.0, 2), ("step_off_by_one", 0.5, 1000)])
def test_adam_mutations_fail(mut, b1, step):
    p, g, m, v = adam_data()
    form = "a" if f32(1.0 - b1) < 0.5 else "b"
    out = adam_f32(p, g, m, v, 1e-3, b1, 0.999, 1e-8, step, 0.25, form, mut)
    fails(lambda: adam_audit(out, p, g, m, v, 1e-3, b1, 0.999, 1e-8, step, 0.25))


# --------------------------------------------------------------------------- loss
def loss_f32(pred, y, oy, ox, mut=None, order=0):
    """loss_partial_kernel + loss_final_kernel: f32 difference, double sums (in another order than numpy's pairwise one),
    the one-pass R2.  Returns (dpred, stats increment (8), loss f32)."""
    N, O, H, W = pred.shape
    Hc, Wc = y.shape[2:]
    if mut == "crop_row":
        oy += 1
    if mut == "crop_col":
        ox -= 1
    d = (pred[:, :, oy:oy + Hc, ox:ox + Wc] - y).astype(f32)
    n = float(N * O * Hc * Wc)
    inv_n = 1.0 / (N * O * H * W) if mut == "inv_n_uncropped" else 1.0 / n
    d64, y64 = d.astype(np.float64), y.astype(np.float64)
    sg = np.sign(d64) + (d64 == 0) if mut == "sign0_is_1" else np.sign(d64)
    dp = np.zeros_like(pred)
    dp[:, :, oy:oy + Hc, ox:ox + Wc] = ((2.0 * d64 + sg) * inv_n).astype(f32)
    tot = (lambda a: float(np.cumsum(a.ravel()[::-1])[-1])) if order else (lambda a: float(np.sum(a.T)))
    s0, s1, s2, s3 = tot(d64 * d64), tot(np.abs(d64)), tot(y64), tot(y64 * y64)
    lo = s0 / n + s1 / n
    ss = s3 - s2 * s2 / n
    const = (0.0, 1.0) if mut == "r2_const_swapped" else (1.0, 0.0)
    r2 = 1.0 - s0 / ss if ss > 0 else (const[0] if s0 == 0 else const[1])
    return dp, np.array([s0, s1, s2, s3, n, lo, r2, 1.0]), f32(lo)


def loss_audit(out, pred, y, oy, ox):
    ref = SM.loss(pred, y, oy, ox)
    SM.check_equal(out[0], ref["dpred"], "dpred")
    SM.check_stats(np.zeros(8), out[1], [ref])
    SM.check_loss_scalar(out[2], ref["loss"])


def loss_data(const=None, same=False):
    rng = np.random.default_rng(3)
    N, O, H, W, oy, ox, Hc, Wc = 2, 3, 9, 11, 2, 3, 5, 6
    pred = rng.standard_normal((N, O, H, W)).astype(f32)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(f32) if const is None else np.full((N, O, Hc, Wc), const, f32)
    if same:
        pred[:, :, oy:oy + Hc, ox:ox + Wc] = y
    pred[1, 2, oy + 1, ox + 2] = y[1, 2, 1, 2]                   # one exact zero difference: sign(0) = 0
    return pred, y, oy, ox


@pytest.mark.parametrize("order", [0, 1])
def test_loss_faithful_emulation_passes(order):
    for args in (loss_data(), loss_data(const=0.5), loss_data(const=-2.0, same=True)):
        loss_audit(loss_f32(*args, order=order), *args)
    assert SM.loss(*loss_data(const=0.5))["r2"] == 0.0 and SM.loss(*loss_data(const=-2.0, same=True))["r2"] == 1.0


def test_loss_stats_accumulate_over_calls():
    args = [loss_data(), loss_data(const=0.5), loss_data()]
    before = np.array([1.0, 2.0, -3.0, 4.0, 5.0, 6.0, -7.0, 8.0])
    after = before + sum(loss_f32(*a)[1] for a in args)
    refs = [SM.loss(*a) for a in args]
    SM.check_stats(before, after, refs)
    fails(lambda: SM.check_stats(before, after - loss_f32(*args[2])[1], refs))          # the third call lost
    fails(lambda: SM.check_stats(before, after + np.eye(8)[7], refs))                  # the call counter off by one


@pytest.mark.parametrize("mut", ["sign0_is_1", "crop_row", "crop_col", "inv_n_uncropped"])
def test_loss_mutations_fail(mut):
    args = loss_data()
    fails(lambda: loss_audit(loss_f32(*args, mut=mut), *args))


def test_loss_r2_constant_target_swap_fails():
    for args in (loss_data(const=0.5), loss_data(const=-2.0, same=True)):
        fails(lambda: loss_audit(loss_f32(*args, mut="r2_const_swapped"), *args))


def test_loss_scalar_one_ulp():
    ref = SM.loss(*loss_data())["loss"]
    l32 = f32(ref)
    away, toward = (f32(9), f32(-9)) if l32 >= ref else (f32(-9), f32(9))
    SM.check_loss_scalar(l32, ref)
    SM.check_loss_scalar(np.nextafter(l32, toward), ref)          # the two f32 values that bracket the f64 loss
    fails(lambda: SM.check_loss_scalar(np.nextafter(np.nextafter(l32, away), away), ref))


# --------------------------------------------------------------------------- head
def head_data(Ch=16, O=5, bf16=False, seed=4):
    rng = np.random.default_rng(seed)
    N, H, W = 2, 5, 7
    h = rng.standard_normal((N, H, W, Ch)).astype(f32)
    if bf16:
        h = SM.bf16_round(h)
    w = (0.3 * rng.standard_normal((O, Ch))).astype(f32)
    b = rng.standard_normal(O).astype(f32)
    return h, w, b


def head_fwd_f32(h, w, b, reverse=False, mut=None):
    """head_fwd_kernel: accumulator = b, then the products one by one (in channel order, or in the opposite one)"""
    N, H, W, Ch = h.shape
    O = w.shape[0]
    acc = np.zeros((N, O, H, W), f32)
    if b is not None and mut != "no_bias":
        acc += b[None, :, None, None] * f32(2.0 if mut == "bias_twice" else 1.0)
    cs = range(Ch - 1 if mut == "drop_last_channel" else Ch)
    for c in (reversed(cs) if reverse else cs):
        acc = acc + w[None, :, None, None, c] * h[:, None, :, :, c]
    if mut == "swap_outputs":
        acc[:, [1, 2]] = acc[:, [2, 1]]
    return acc


def head_bwd_f32(w, dp, Chp, bf16, reverse=False, mut=None):
    O, Ch = w.shape
    N, _, H, W = dp.shape
    acc = np.zeros((N, H, W, Chp), f32)
    for o in (reversed(range(O)) if reverse else range(O)):
        acc[..., :Ch] = acc[..., :Ch] + w[o][None, None, None, :] * dp[:, o, :, :, None]
    if mut == "pad_nonzero":
        acc[1, 2, 3, Chp - 1] = f32(1e-30)
    if mut == "swap_outputs":
        acc[..., :Ch] += (w[2] - w[1]) * (dp[:, 1] - dp[:, 2])[..., None]
    return SM.bf16_round(acc) if bf16 else acc


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("Ch,O", [(16, 5), (100, 3), (160, 4)])
def test_head_faithful_emulations_pass_in_both_orders(Ch, O, bf16, reverse):
    h, w, b = head_data(Ch, O, bf16)
    for bias in (b, None):
        SM.ratio(head_fwd_f32(h, w, bias, reverse), *SM.head_fwd(h, w, bias), what="pred")
    dp = np.random.default_rng(5).standard_normal((2, O, 5, 7)).astype(f32)
    Chp = (Ch + 31) // 32 * 32
    SM.ratio(head_bwd_f32(w, dp, Chp, bf16, reverse), *SM.head_bwd_dh(w, dp, Chp, bf16), what="dh")


@pytest.mark.parametrize("mut", ["bias_twice", "no_bias", "drop_last_channel", "swap_outputs"])
def test_head_fwd_mutations_fail(mut):
    h, w, b = head_data()
    fails(lambda: SM.ratio(head_fwd_f32(h, w, b, mut=mut), *SM.head_fwd(h, w, b), what="pred"))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mut", ["pad_nonzero", "swap_outputs"])
def test_head_bwd_mutations_fail(mut, bf16):
    h, w, b = head_data()
    dp = np.random.default_rng(5).standard_normal((2, 5, 5, 7)).astype(f32)
    fails(lambda: SM.ratio(head_bwd_f32(w, dp, 32, bf16, mut=mut), *SM.head_bwd_dh(w, dp, 32, bf16), what="dh"))


def fused_f32(h, w, b, y, oy, ox, Chp, bf16, reverse=False, mut=None):
    pred = head_fwd_f32(h, w, b, reverse, mut if mut in ("no_bias", "drop_last_channel") else None)
    dp, st, lo = loss_f32(pred, y, oy, ox, mut if mut in ("crop_row", "sign0_is_1") else None)
    if mut == "sign_flipped_far_from_zero":
        i = np.unravel_index(np.argmax(np.abs(dp)), dp.shape)
        dp[i] = f32(dp[i] - np.sign(dp[i]) * 2.0 / y.size)
    return dp, head_bwd_f32(w, dp, Chp, bf16, reverse, mut if mut == "pad_nonzero" else None), st, lo


def fused_audit(out, h, w, b, y, oy, ox, Chp, bf16):
    ref = SM.head_loss_fused(h, w, b, y, oy, ox, Chp, bf16)
    SM.ratio(out[0], *ref["dpred"], what="fused dpred")
    SM.ratio(out[1], *ref["dh"], what="fused dh")
    SM.check_stats(np.zeros(8), out[2], [ref["loss"]], ref["sum_tol"])
    SM.check_loss_scalar(out[3], ref["loss"]["loss"], ref["loss_extra"])


def fused_data(bf16):
    h, w, b = head_data(16, 5, bf16)
    y = np.random.default_rng(6).standard_normal((2, 5, 3, 4)).astype(f32)
    # one target equal to the f32 prediction: d is zero to within the head bound, so the sign there is legitimately open
    y[0, 1, 1, 1] = head_fwd_f32(h, w, b)[0, 1, 2, 3]
    return h, w, b, y, 1, 2, 32, bf16


@pytest.mark.parametrize("bf16", [False, True])
def test_fused_faithful_emulation_passes_in_both_orders(bf16):
    args = fused_data(bf16)
    for reverse in (False, True):
        fused_audit(fused_f32(*args, reverse=reverse), *args)


@pytest.mark.parametrize("mut", ["no_bias", "drop_last_channel", "crop_row", "sign_flipped_far_from_zero", "pad_nonzero"])
def test_fused_mutations_fail(mut):
    args = fused_data(False)
    fails(lambda: fused_audit(fused_f32(*args, mut=mut), *args))


# --------------------------------------------------------------------------- pack / unpack / fold
def pack_elementwise(x, Cp, geom, kf, bf16, mut=None):
    """pack_btchw_kernel's index arithmetic, one slab element at a time"""
    B, T, C, H, W = x.shape
    _, _, P, Hh, Wh = geom
    out = np.zeros((T * B, Hh, Wh, Cp), f32)
    i = np.arange(B * T * H * W * Cp)
    co = i % Cp; r = i // Cp
    xx = r % W; r //= W
    yy = r % H; r //= H
    b = r % B; t = r // B
    kx = co // C; c = co - kx * C
    xi = xx + (kf - 1 - kx if mut == "kx_mirrored" else kx) - kf // 2
    ok = (kx < kf) & (xi >= 0) & (xi < W)
    v = np.where(ok, x[b, t, np.minimum(c, C - 1), yy, np.clip(xi, 0, W - 1)], f32(0))
    out[t * B + b, yy + P, xx + P, co] = SM.bf16_round(v) if bf16 else v
    return out


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kf", [1, 3, 5])
def test_pack_reference_equals_the_elementwise_kernel_and_mirrored_taps_fail(kf, bf16):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 3, 3, 4, 9)).astype(f32)
    geom = SM.make_geom(4, 9, 2)
    Cp = (kf * 3 + 7) // 8 * 8
    ref = SM.pack_btchw(x, Cp, geom, kf, bf16)
    SM.check_equal(pack_elementwise(x, Cp, geom, kf, bf16), ref)
    if kf > 1:
        fails(lambda: SM.check_equal(pack_elementwise(x, Cp, geom, kf, bf16, "kx_mirrored"), ref))
    # round trips of the exact layout references
    SM.check_equal(SM.unpack_halo(ref, 2, 3, 3, geom) if kf == 1 else SM.unpack_halo(ref, 2, 3, 3 * kf, geom)[:, kf // 2 * 3:kf // 2 * 3 + 3],
                   (SM.bf16_round(x) if bf16 else x).transpose(1, 0, 2, 3, 4).reshape(6, 3, 4, 9)[2:5])
    c = SM.pack_compact(x[0], 8, bf16)
    SM.check_equal(SM.unpack_compact(c, 3), SM.bf16_round(x[0]) if bf16 else x[0])
    assert float(np.abs(c[..., 3:]).max()) == 0


def test_unfold_dx_reference_is_the_adjoint_of_the_fold():
    rng = np.random.default_rng(8)
    N, C, k, H, W, Cp = 2, 3, 5, 4, 9, 16
    G = rng.standard_normal((N, H, W, Cp)).astype(f32)
    x = rng.standard_normal((1, N, C, H, W))
    ref, bound = SM.unfold_dx(G, C, k)
    fold = SM._fold(x, k)[0].transpose(0, 2, 3, 1)
    assert abs(float((fold * G[..., :k * C]).sum()) - float((x[0] * ref).sum())) <= 1e-12 * float(np.abs(fold * G[..., :k * C]).sum())
    acc = np.zeros((N, C, H, W), f32)                             # the kernel's f32 sum in tap order
    for kx in range(k):
        for xo in range(W):
            xs = xo - kx + k // 2
            if 0 <= xs < W:
                acc[:, :, :, xo] += G[:, :, xs, kx * C:(kx + 1) * C].transpose(0, 2, 1)
    SM.ratio(acc, ref, bound, "dx")
    bad = acc.copy(); bad[1, 2, 3, 0] -= G[1, 3, 2, 2 * C + 2]     # the last tap inside the row dropped at the left edge
    fails(lambda: SM.ratio(bad, ref, bound, "dx"))


# --------------------------------------------------------------------------- preproc
def pre_kernel(srcs, nstatic, mean, std, t0, T, Hp, Wp, mode, mut=None, max_b=64):
    """preproc_nchw_kernel launched per chunk of max_b samples, row by row with pre_src_row's arithmetic"""
    H, W = srcs[0].shape[2:]
    C = sum(s.shape[1] for s in srcs)
    first = np.cumsum([0] + [s.shape[1] for s in srcs])
    B = len(t0)
    pl, pt = (Wp - W) // 2, (Hp - H) // 2
    pb = Hp - H - pt
    if mut == "pt_pb_swapped":
        pt, pb = pb, pt
    out = np.zeros((B, T, C, Hp, Wp), f32)
    for b0 in range(0, B, max_b):
        for b in range(min(max_b, B - b0)):
            ob = b if mut == "b0_dropped" else b0 + b
            for t in range(T):
                for c in range(C):
                    for yp in range(Hp):
                        flip = False
                        if yp < pt:
                            ys, flip = (1 + yp, True) if mode == 0 else (pt - yp, False)
                        elif yp < pt + H:
                            ys = yp - pt
                        else:
                            j = yp - pt - H
                            ys, flip = (H - pb - 1 + j, True) if mode == 0 else (H - 2 - j, False)
                        cs = C - 1 - c if flip else c
                        s = int(np.searchsorted(first, cs, side="right") - 1)
                        step = 0 if s >= len(srcs) - nstatic else t0[b0 + b] + t
                        row = srcs[s][step, cs - first[s], ys]
                        st = c if mut == "flip_stats_from_c" else cs
                        xs = (np.arange(Wp) - pl) % W
                        out[ob, t, c, yp] = (row[xs] - mean[st]) / std[st]
    return out


def pre_data(B, H=5, W=6):
    rng = np.random.default_rng(9)
    steps, T = 6, 2
    srcs = [rng.standard_normal((steps, 2, H, W)).astype(f32), rng.standard_normal((steps, 1, H, W)).astype(f32),
            rng.standard_normal((1, 2, H, W)).astype(f32)]
    mean, std = rng.standard_normal(5).astype(f32), (0.5 + rng.random(5)).astype(f32)
    t0 = [int(v) for v in rng.integers(0, steps - T + 1, B)]
    return srcs, 1, mean, std, t0, T


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Hp,Wp", [(8, 9), (7, 8), (6, 10)])
def test_preproc_reference_equals_the_kernel_emulation_and_the_oracle(mode, Hp, Wp):
    args = pre_data(3)
    ref = SM.preproc(*args, Hp, Wp, mode)
    SM.check_equal(pre_kernel(*args, Hp, Wp, mode), ref)
    # and the literal restatement of the reference code (concatenate / fliplr), sample by sample
    srcs, nstatic, mean, std, t0, T = args
    for b, s0 in enumerate(t0):
        fused = np.concatenate([s[s0:s0 + T] if i < 2 else np.repeat(s, T, axis=0) for i, s in enumerate(srcs)], axis=1)
        want = PO.padding_data_4d(PO.zscore(fused, mean, std), (Hp, Wp), "reference" if mode == 0 else "reflect").astype(f32)
        SM.check_equal(ref[b], want)


def test_preproc_mutations_fail():
    args = pre_data(70, 3, 4)                                    # 70 samples: two chunks, the second at b0 = 64
    ref = SM.preproc(*args, 6, 5, 0)                             # Hp - H = 3: pt = 1, pb = 2
    SM.check_equal(pre_kernel(*args, 6, 5, 0), ref)
    for mut in ("b0_dropped", "flip_stats_from_c", "pt_pb_swapped"):
        fails(lambda: SM.check_equal(pre_kernel(*args, 6, 5, 0, mut), ref))
    ref1 = SM.preproc(*args, 6, 5, 1)
    fails(lambda: SM.check_equal(pre_kernel(*args, 6, 5, 1, "pt_pb_swapped"), ref1))
    # the slab entry = the NCHW result packed (and folded) into the halo slab: a mirrored fold tap fails there too
    geom = SM.make_geom(6, 5, 1)
    slab = SM.pack_btchw(ref[:2], 16, geom, 3, True)
    SM.check_equal(pack_elementwise(ref[:2], 16, geom, 3, True), slab)
    fails(lambda: SM.check_equal(pack_elementwise(ref[:2], 16, geom, 3, True, "kx_mirrored"), slab))


# --------------------------------------------------------------------------- evaluation: skill sums
def _exact_int_sums(mt, st, slots, before, scale):
    """the model's sums again, in int64 arithmetic on the terms times `scale` (every term must be an integer then)"""
    mi, si = np.rint(mt * scale).astype(np.int64), np.rint(st * scale).astype(np.int64)
    assert np.array_equal(mi.astype(np.float64), mt * scale) and np.array_equal(si.astype(np.float64), st * scale)
    named = before[:SX.NSLOTS - 1]
    pix = np.rint(named * scale).astype(np.int64)
    assert np.array_equal(pix.astype(np.float64), named * scale)
    for n, s_ in enumerate(slots):
        if s_ >= 0:
            pix[s_] += mi[:, n]
    return pix, si.sum(axis=(3, 4)).transpose(1, 2, 0)


def _assert_order_free(mt, st, slots, before, ref, scale):
    pix_i, smp_i = _exact_int_sums(mt, st, slots, before, scale)
    # every partial sum, in any order, is a multiple of 1 / scale of magnitude at most the sum of the magnitudes: below
    # 2^53 / scale each one is an f64 number, so no addition of the kernel or of the model rounds
    assert scale * float(ref["pix_abs"][:SX.NSLOTS - 1].max()) < 2.0 ** 53 and scale * float(ref["sample_abs"].max()) < 2.0 ** 53
    assert np.array_equal(ref["pix"][:SX.NSLOTS - 1] * scale, pix_i.astype(np.float64))
    assert np.array_equal(ref["sample"] * scale, smp_i.astype(np.float64))
    SM.check_equal(ref["pix"][SX.NSLOTS - 1], before[SX.NSLOTS - 1], "sentinel slot")


@pytest.mark.parametrize("name", list(SX.PLAIN_CASES))
def test_skill_model_is_exact_and_order_free_on_the_plain_integer_data(name):
    c = SX.PLAIN_CASES[name]
    pred, y, row_w, before, slots = SX.plain_data(name)
    assert np.isnan(pred).sum() == c.N * c.O * (c.H * c.W - c.Hc * c.Wc)         # NaN exactly outside the crop window
    ref = SM.skill_sums(pred, y, c.oy, c.ox, slots, SX.NSLOTS, row_w, before)
    mt, st = SM.skill_terms(pred, y, c.oy, c.ox, row_w)
    assert np.isfinite(mt).all() and np.isfinite(st).all()
    sl = [0] * c.N if slots is None else slots
    _assert_order_free(mt, st, sl, before, ref, 8)
    # the samples in reverse order, the crop summed column by column: the same bits
    pix = before.copy()
    for n in reversed(range(c.N)):
        if sl[n] >= 0:
            pix[sl[n]] = mt[:, n] + pix[sl[n]]
    SM.check_equal(pix, ref["pix"], "reversed sample order")
    SM.check_equal(np.ascontiguousarray(st.sum(axis=3).sum(axis=3).transpose(1, 2, 0)), ref["sample"], "columns first")
    assert ref["sample_n"] == c.Hc * c.Wc
    if slots is not None and c.slots == "none":
        SM.check_equal(ref["pix"], before, "every slot -1")


def test_skill_model_against_fractions():
    """one case evaluated with fractions.Fraction from the stored f32 / f64 values, nothing scaled"""
    name = "1x257-N5-O7"
    c = SX.PLAIN_CASES[name]
    pred, y, row_w, before, slots = SX.plain_data(name)
    ref = SM.skill_sums(pred, y, c.oy, c.ox, slots, SX.NSLOTS, row_w, before)
    F = fractions.Fraction
    for n in range(c.N):
        for o in range(0, c.O, 3):
            rows = [F(0)] * 8
            for cx in range(c.Wc):
                p, t, rw = F(float(pred[n, o, c.oy, c.ox + cx])), F(float(y[n, o, 0, cx])), F(float(row_w[0]))
                d = p - t
                for k, v in enumerate((d * d, abs(d), t, t * t, p, p * p, rw * t, rw * p)):
                    rows[k] += v
            assert [F(float(v)) for v in ref["sample"][n, o]] == rows
    for s_ in range(SX.NSLOTS - 1):
        want = F(float(before[s_, 4, 2, 0, 100]))
        for n in range(c.N):
            if slots[n] == s_:
                want += (F(float(pred[n, 2, c.oy, c.ox + 100])) - F(float(y[n, 2, 0, 100]))) ** 2
        assert F(float(ref["pix"][s_, 4, 2, 0, 100])) == want


@pytest.mark.parametrize("name", list(SX.FUSED_CASES))
def test_skill_head_model_is_exact_and_order_free_on_the_fused_integer_data(name):
    c = SX.FUSED_CASES[name]
    slab, h, w, b, y, row_w, before, slots, gt = SX.fused_data(name)
    Chp = SX.chp_of(c.dt, c.Ch)
    assert Chp <= 128 and Chp % 4 == 0 and ("Chp" not in name or Chp > c.Ch) and (b is None) == (not c.bias)
    SM.check_equal(SM.bf16_round(np.nan_to_num(slab)), np.nan_to_num(slab), "the slab is exact in bf16")
    # NaN wherever the kernel must not read; zeros in the crop's channel padding
    live = np.zeros(slab.shape, bool)
    live[c.n0:, c.P + c.oy:c.P + c.oy + c.Hc, c.P + c.ox:c.P + c.ox + c.Wc] = True
    assert np.isnan(slab[~live]).all() and np.isfinite(slab[live]).all()
    assert not slab[c.n0:, c.P + c.oy:c.P + c.oy + c.Hc, c.P + c.ox:c.P + c.ox + c.Wc, c.Ch:].any()
    pred = SM.skill_head_pred(h, w, b)
    # the head in f32, channel by channel from either end, rounding each product and each add: the same bits
    for order in (range(c.Ch), reversed(range(c.Ch))):
        acc = np.zeros(pred.shape, f32) if b is None else np.broadcast_to(b[None, :, None, None], pred.shape).astype(f32)
        for ch in order:
            acc = acc + (w[None, :, None, None, ch] * h[:, None, :, :, ch]).astype(f32)
        SM.check_equal(acc, pred, "f32 chain")
    assert float(np.abs(pred).max()) < 2.0 ** 11
    ref = SM.skill_sums(pred, y, 0, 0, slots, SX.NSLOTS, row_w, before)
    mt, st = SM.skill_terms(pred, y, 0, 0, row_w)
    _assert_order_free(mt, st, slots, before, ref, 32)


def test_skill_head_pred_refuses_data_that_is_not_exact():
    rng = np.random.default_rng(5)
    h, w = rng.integers(-4, 5, (1, 2, 3, 8)).astype(f32), (rng.integers(-8, 9, (2, 8)) / 4.0).astype(f32)
    SM.skill_head_pred(h, w, None)
    with pytest.raises(ValueError):
        SM.skill_head_pred(h + f32(0.1), w, None)
    with pytest.raises(ValueError):
        SM.skill_head_pred(h, w, np.array([0.3, 1.0], f32))


def test_gamma_takes_the_unit_roundoff_of_the_format():
    assert SM.gamma(3) == 3 * SM.U / (1 - 3 * SM.U) and SM.gamma(0, SM.U64) == 0.0
    assert abs(SM.gamma(12959, SM.U64) - 1.4388e-12) < 1e-16      # the product crop's sample rows


def test_skill_audit_passes_other_orders_and_has_teeth():
    rng = np.random.default_rng(9)
    N, O, H, W, oy, ox, Hc, Wc, S = 9, 2, 8, 11, 1, 2, 5, 7, 3
    pred, y = rng.standard_normal((N, O, H, W)).astype(f32), rng.standard_normal((N, O, Hc, Wc)).astype(f32)
    row_w = 0.25 + rng.random(Hc)
    slot = [0, 1, -1, 0, 0, 1, 0, -1, 0]                           # slot 2: no sample
    before = rng.standard_normal((S, 5, O, Hc, Wc))
    before[0] = 0
    ref = SM.skill_sums(pred, y, oy, ox, slot, S, row_w, before)
    args = (pred, y, oy, ox, slot, S, row_w, before)
    r = SM.skill_audit(*args, ref["pix"], ref["sample"])
    assert 0.0 <= r[0] <= 1.0 and 0.0 <= r[1] <= 1.0
    mt, st = SM.skill_terms(pred, y, oy, ox, row_w)
    # another order: samples descending, the crop as a chain from the last pixel
    pix = before.copy()
    for n in reversed(range(N)):
        if slot[n] >= 0:
            pix[slot[n]] = pix[slot[n]] + mt[:, n]
    rows = np.zeros((N, O, 8))
    for v in st.reshape(8, N, O, -1).transpose(3, 1, 2, 0)[::-1]:
        rows = rows + v
    assert not np.array_equal(rows, ref["sample"])
    SM.skill_audit(*args, pix, rows)

    def moved(a, idx, by):
        a = a.copy()
        a[idx] += by
        return a
    cell = (0, 2, 1, 2, 3)                                         # sum of t^2 over the five samples of slot 0
    assert ref["pix_n"][cell] == 5 and ref["pix_n"][(1,) + cell[1:]] == 3
    fails(lambda: SM.skill_audit(*args, moved(ref["pix"], cell, 8 * np.spacing(ref["pix"][cell])), ref["sample"]))
    fails(lambda: SM.skill_audit(*args, moved(ref["pix"], cell, mt[(2, 2) + cell[2:]]), ref["sample"]))      # the slot -1 sample
    fails(lambda: SM.skill_audit(*args, moved(ref["pix"], cell, -mt[(2, 3) + cell[2:]]), ref["sample"]))     # sample 3 dropped
    fails(lambda: SM.skill_audit(*args, moved(ref["pix"], (2,) + cell[1:], np.spacing(ref["pix"][(2,) + cell[1:]])), ref["sample"]))   # an idle slot touched
    row = (4, 1, 3)
    fails(lambda: SM.skill_audit(*args, ref["pix"], moved(ref["sample"], row, 64 * np.spacing(ref["sample"][row]))))
    fails(lambda: SM.skill_audit(*args, ref["pix"], moved(ref["sample"], row, -st[3, 4, 1, 4, 6])))          # one pixel left out
    fails(lambda: SM.skill_audit(*args, ref["pix"], moved(ref["sample"], (2, 0, 0), np.nan)))
