"""The kernels of csrc/pointwise.hip, csrc/head.hip and csrc/pack.hip around the gate GEMMs -- Adam, the loss, the 1x1 head and its fused form, the layout
packers and the preproc -- at every branch of their host dispatch, called through the C ABI and checked element by
element with the f64 references and derived bounds of oracle/small_audit.py (no tolerance here comes from a run).

Every case names the branch it is meant to reach and asserts, in Python, the dispatch condition copied from the host code
(csrc/head.hip, csrc/pack.hip): a case whose shape drifts out of its branch fails before it launches anything.  Every buffer is sized
exactly for its call."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import preproc_oracle as PO
from oracle import small_audit as SM

pytestmark = pytest.mark.gpu
f32 = np.float32
KIB = 1024


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as pkg
    return pkg.load_library()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def geom(lib, H, W, Pd):
    from nasa_niswan_amd._lib import NintGeom
    g = NintGeom()
    assert lib.nint_geom_make(C.byref(g), H, W, Pd) == 0
    assert (g.H, g.W, g.P, g.Hh, g.Wh) == SM.make_geom(H, W, Pd)
    return g, (g.H, g.W, g.P, g.Hh, g.Wh)


def et(dt):
    return torch.bfloat16 if dt else torch.float32


def to_slab(vals, dt):
    """f32 values (already representable in the storage type) -> device tensor of the storage type"""
    return dev(np.asarray(vals, f32)).to(et(dt))


def decode(t, dt):
    """device tensor of the storage type -> the stored values as f32, exactly"""
    torch.cuda.synchronize()
    if dt:
        return SM.decode_bf16(t.view(torch.int16).cpu().numpy().view(np.uint16))
    return t.cpu().numpy()


def stored(a, dt):
    a = np.asarray(a, f32)
    return SM.bf16_round(a) if dt else a


# =========================================================================== Adam
GRID1D_CAP = 8192 * 256            # grid1d(): 256 * 32 workgroups of 256 threads; above it the grid-stride loop iterates
GRAD_MAGS = np.array([0.0, 1e-12, 1e-6, 1.0, 1e4], f32)


def adam_grads(rng, n):
    return (GRAD_MAGS[rng.integers(0, 5, n)] * rng.choice([-1.0, 1.0], n) * (0.5 + rng.random(n))).astype(f32)


def adam_step_checked(lib, p, g, m, v, lr, b1, b2, eps, step, gs, what):
    """one nint_adam_flat call, audited against one torch.optim.Adam f64 step from the state the device held before it"""
    before = [host(t).copy() for t in (p, g, m, v)]
    assert lib.nint_adam_flat(P(p), P(g), P(m), P(v), p.numel(), lr, b1, b2, eps, step, gs, None) == 0
    ref = SM.adam(*before, lr, b1, b2, eps, step, gs)
    worst = {k: SM.ratio(host(t), *ref[k], what=f"{what} step {step} {k}") for k, t in (("p", p), ("m", m), ("v", v))}
    print(f"{what} step {step}: worst ratios {worst}")
    np.testing.assert_array_equal(host(g), before[1])             # the gradient is read-only
    return ref


@pytest.mark.parametrize("b2", [0.999, 0.9], ids=lambda b: f"beta2={b}")
@pytest.mark.parametrize("b1,lerp", [pytest.param(0.9, "a", id="lerp[w1<0.5:m+w(g-m)]-beta1=0.9"),
                                     pytest.param(0.6, "a", id="lerp[w1<0.5:m+w(g-m)]-beta1=0.6"),
                                     pytest.param(0.5, "b", id="lerp[w1>=0.5:g-(g-m)(1-w)]-beta1=0.5"),
                                     pytest.param(0.0, "b", id="lerp[w1>=0.5:g-(g-m)(1-w)]-beta1=0.0")])
def test_adam_both_lerp_formulas_steps_1_to_5_then_1000(lib, b1, lerp, b2):
    assert (f32(1.0 - b1) < f32(0.5)) == (lerp == "a")            # adam_flat_kernel: (w1 < 0.5f) ? ... : ...
    rng = np.random.default_rng(20)
    n, lr, eps, gs = 4096 + 3, 1e-3, 1e-8, 0.25
    p = dev(rng.standard_normal(n).astype(f32))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 6):
        g = adam_grads(rng, n)
        g[:64] = 0                                                # zero gradient on zero state at every step: denom = eps
        ref = adam_step_checked(lib, p, dev(g), m, v, lr, b1, b2, eps, step, gs, f"beta1={b1} beta2={b2}")
        assert float(ref["p"][1][:64].max()) == 0.0 and not host(m)[:64].any() and not host(v)[:64].any()
    # step 1000 from a loaded state (a checkpoint): the bias corrections near their limits
    g = adam_grads(rng, n)
    m.copy_(dev((g * (0.1 + 0.05 * rng.standard_normal(n))).astype(f32)))
    v.copy_(dev((g * g * f32(0.01)).astype(f32)))
    adam_step_checked(lib, p, dev(adam_grads(rng, n)), m, v, lr, b1, b2, eps, 1000, gs, f"beta1={b1} beta2={b2}")


def test_adam_grid_stride_loop_above_the_grid_cap(lib):
    n = GRID1D_CAP + 257
    assert n > GRID1D_CAP                                         # grid1d(): g > 256 * 32 -> capped, the loop strides
    rng = np.random.default_rng(21)
    p = dev(rng.standard_normal(n).astype(f32))
    g = adam_grads(rng, n)
    m, v = dev((g * f32(0.1)).astype(f32)), dev((g * g * f32(0.01)).astype(f32))
    adam_step_checked(lib, p, dev(g), m, v, 1e-3, 0.9, 0.999, 1e-8, 4, 0.25, "grid-stride")


def test_fused_adam_optimizer_default_betas_take_the_first_lerp_formula(lib):
    from nasa_niswan_amd.optim import FlatParams, FusedAdam
    torch.manual_seed(22)
    mod = torch.nn.Linear(37, 11).cuda()
    flat = FlatParams(mod)
    opt = FusedAdam(flat)
    b1, b2 = opt.param_groups[0]["betas"]
    assert (b1, b2) == (0.9, 0.999) and f32(1.0 - b1) < f32(0.5)
    rng = np.random.default_rng(22)
    for step in (1, 2):
        flat.grad.copy_(dev(adam_grads(rng, flat.numel)))
        before = [host(t).copy() for t in (flat.data, flat.grad, opt.exp_avg, opt.exp_avg_sq)]
        opt.step()
        ref = SM.adam(*before, 1e-3, b1, b2, 1e-8, step, 1.0)
        for k, t in (("p", flat.data), ("m", opt.exp_avg), ("v", opt.exp_avg_sq)):
            SM.ratio(host(t), *ref[k], what=f"FusedAdam step {step} {k}")
    assert mod.weight.data_ptr() == flat.data.data_ptr()          # the module's parameters are the bucket that moved


# =========================================================================== 1x1 head
def head_fused_holds(Chp, O):
    """The ONE limit of the staged head arithmetic (csrc/head.hip head_staged_holds, engine._beyond_fused_head): at most 128
    padded channels in 4-channel vectors, and the weight image [O][CHV] plus one 64-output chunk of d loss / d pred of 64
    pixels plus 8 KiB of static LDS within the 160 KiB of a CU"""
    chv = 32 if Chp <= 32 else (64 if Chp <= 64 else 128)
    return Chp <= 128 and Chp % 4 == 0 and (O * chv + min(O, 64) * 64) * 4 + 8192 <= 160 * KIB


def head_dispatch(dt, Ch, O):
    """nint_head_fwd / nint_head_bwd: which kernel runs (the condition of the host code): the staged kernels wherever the
    fused head passes hold the shape -- with the dynamic-LDS opt-in once the weight image exceeds 64 KiB -- so that fused and
    unfused entries run the same arithmetic; the wide kernels beyond"""
    kc = 32 if dt else 16
    Chp = (Ch + kc - 1) // kc * kc
    chv = 32 if Chp <= 32 else (64 if Chp <= 64 else 128)
    w_lds = O * chv * 4
    fwd = bwd = f"staged{chv}" if head_fused_holds(Chp, O) else "wide"
    return Chp, chv, w_lds, fwd, bwd


def head_inputs(lib, dt, Ch, O, N, n0, H, W, Pd, seed, bias=True):
    rng = np.random.default_rng(seed)
    g, gt = geom(lib, H, W, Pd)
    Chp = head_dispatch(dt, Ch, O)[0]
    assert Chp == (Ch + lib.nint_kc(dt) - 1) // lib.nint_kc(dt) * lib.nint_kc(dt)
    # the whole slab is random, halo ring, slack and images below n0 included: a kernel that reads a wrong place sees it.
    # The channel padding holds zeros, as every producer of an h slab leaves it.
    full = stored(rng.standard_normal((n0 + N, g.Hh, g.Wh, Chp)), dt)
    full[..., Ch:] = 0
    hsl = to_slab(full, dt)
    h = full[n0:, Pd:Pd + H, Pd:Pd + W, :Ch]
    w = (0.3 * rng.standard_normal((O, Ch))).astype(f32)
    b = rng.standard_normal(O).astype(f32) if bias else None
    return g, Chp, hsl, h, w, b, rng


HEAD_CASES = [
    # id = <kernel the case must reach>-<why>; (dt, Ch, O, kernel, bias, n0)
    pytest.param(0, 16, 20, "staged32", True, 0, id="staged32-f32-Chp16"),
    pytest.param(1, 16, 20, "staged32", True, 2, id="staged32-bf16-Chp32-n0=2"),
    pytest.param(0, 48, 3, "staged64", False, 1, id="staged64-f32-Chp48-no-bias-n0=1"),
    pytest.param(1, 64, 5, "staged64", True, 0, id="staged64-bf16-Chp64"),
    pytest.param(0, 100, 3, "staged128", True, 0, id="staged128-f32-Chp112"),
    pytest.param(1, 128, 20, "staged128", False, 1, id="staged128-bf16-Chp128-no-bias-n0=1"),
    pytest.param(0, 160, 4, "wide", True, 1, id="wide[Chp>128]-f32-Ch160-n0=1"),
    pytest.param(1, 160, 4, "wide", False, 0, id="wide[Chp>128]-bf16-Ch160-no-bias"),
    pytest.param(0, 16, 600, "staged32", True, 0, id="staged32-LDS-opt-in[weights>64KiB]-f32-O600-Ch16"),
    pytest.param(1, 128, 200, "staged128", True, 1, id="staged128-LDS-opt-in[weights>64KiB]-bf16-O200-Ch128-n0=1"),
    pytest.param(1, 16, 1088, "staged32", False, 0, id="staged32-LDS-opt-in[last O the rule admits]-bf16-O1088-Ch16-no-bias"),
    pytest.param(0, 16, 1200, "wide", True, 0, id="wide[weights beyond the LDS rule]-f32-O1200-Ch16"),
    pytest.param(1, 16, 1200, "wide", True, 1, id="wide[weights beyond the LDS rule]-bf16-O1200-Ch16-n0=1"),
]


@pytest.mark.parametrize("dt,Ch,O,kernel,bias,n0", HEAD_CASES)
def test_head_fwd_and_dh_elementwise_at_every_dispatch_branch(lib, dt, Ch, O, kernel, bias, n0):
    Chp, chv, w_lds, fwd, bwd = head_dispatch(dt, Ch, O)
    assert fwd == kernel and bwd == kernel
    assert (kernel != "wide" and w_lds > 64 * KIB) == (O in (200, 600, 1088))                  # the hipFuncSetAttribute branch
    if O == 1200:
        assert Chp <= 128 and not head_fused_holds(Chp, O)
    if O == 1088:
        assert head_fused_holds(Chp, O) and not head_fused_holds(Chp, O + 1)
    N, H, W, Pd = 2, 9, 13, 2
    g, Chp, hsl, h, w, b, rng = head_inputs(lib, dt, Ch, O, N, n0, H, W, Pd, 30 + Ch + O, bias)
    wd, bd = dev(w), (dev(b) if bias else None)
    pred = torch.full((N, O, H, W), 7.0, device="cuda")
    assert lib.nint_head_fwd(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(pred), C.byref(g), dt, None) == 0
    r = SM.ratio(host(pred), *SM.head_fwd(h, w, b), what="pred")
    dp = rng.standard_normal((N, O, H, W)).astype(f32)
    dh = torch.full((N, H, W, Chp), 7.0, device="cuda").to(et(dt))
    dpd = dev(dp)
    assert lib.nint_head_bwd(P(hsl), n0, N, Ch, Chp, O, P(wd), P(dpd), P(dh), None, None, C.byref(g), dt, None, 0, None) == 0
    got = decode(dh, dt)
    r2 = SM.ratio(got, *SM.head_bwd_dh(w, dp, Chp, bool(dt)), what="dh")
    assert not got[..., Ch:].any()                                # the channel padding: exactly zero (bound 0 above, too)
    print(f"head {kernel} dt={dt}: worst ratio pred {r:.3f}, dh {r2:.3f}")


LOSS_BLOCKS_MAX = (8194 - 2) // 8     # csrc/head.hip: what the caller's scratch holds, 4 doubles per workgroup

FUSED_CASES = [
    # (dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, CHV of the instantiation, what else the case is there for)
    pytest.param(0, 16, 20, 2, 1, 9, 13, 2, 3, 4, 5, 32, ("asym",), id="fused32-f32-asymmetric-crop-n0=1"),
    pytest.param(1, 16, 20, 2, 0, 9, 13, 0, 0, 9, 13, 32, ("full",), id="fused32-bf16-full-image-crop"),
    pytest.param(0, 48, 3, 3, 0, 7, 11, 1, 1, 5, 9, 64, ("ragged",), id="fused64-f32-npix-not-multiple-of-64"),
    pytest.param(1, 64, 70, 1, 1, 9, 13, 2, 1, 5, 11, 64, ("chunks",), id="fused64-bf16-O70-two-output-chunks-n0=1"),
    pytest.param(0, 100, 3, 2, 0, 9, 13, 3, 1, 4, 9, 128, ("asym",), id="fused128-f32-Chp112-asymmetric-crop"),
    pytest.param(1, 128, 128, 1, 0, 9, 13, 2, 2, 5, 9, 128, ("optin",), id="fused128-bf16-LDS-opt-in[lds+8KiB>64KiB]-O128"),
    pytest.param(0, 128, 128, 1, 1, 6, 11, 1, 2, 4, 7, 128, ("optin",), id="fused128-f32-LDS-opt-in[lds+8KiB>64KiB]-O128-n0=1"),
    pytest.param(0, 16, 1, 2, 0, 150, 220, 5, 4, 140, 212, 32, ("many",), id="fused32-f32-grid-stride[npix/64>LOSS_BLOCKS_MAX]"),
    pytest.param(1, 16, 2, 2, 0, 150, 220, 5, 4, 140, 212, 32, ("many",), id="fused32-bf16-grid-stride[npix/64>LOSS_BLOCKS_MAX]"),
    # "window": the weight image alone is beyond 64 KiB while the fused LDS rule still holds.  The unfused entries must run
    # their staged kernels there too (with the LDS opt-in), or "fused = the three launches bit for bit" fails
    pytest.param(1, 128, 200, 1, 0, 9, 13, 2, 2, 5, 9, 128, ("window", "optin"), id="fused128-bf16-window[weights>64KiB]-Ch128-O200"),
    pytest.param(0, 48, 300, 1, 1, 9, 13, 2, 1, 5, 11, 64, ("window", "optin"), id="fused64-f32-window[weights>64KiB]-Ch48-O300-n0=1"),
    pytest.param(0, 16, 600, 2, 0, 9, 13, 2, 3, 4, 5, 32, ("window", "optin"), id="fused32-f32-window[weights>64KiB]-Ch16-O600"),
    pytest.param(1, 16, 1088, 1, 0, 9, 13, 2, 2, 5, 9, 32, ("window", "optin"), id="fused32-bf16-window[last O the LDS rule admits]-Ch16-O1088"),
    # "tail": hidden values and weights in the last 12 STAGED channels (Ch > CHV - 12), the ones the head's dot product joins by a
    # rounded product and an add instead of a fused multiply-add (include/nint.h): with zeros there both give the same bits, and no
    # fused-vs-launches comparison sees how a body forms them.  (The bf16 64 and both 128 cases above have Ch = CHV as well.)
    pytest.param(0, 24, 5, 2, 1, 5, 70, 1, 2, 3, 60, 32, ("tail", "ragged"), id="fused32-f32-tail-channels-Ch24-n0=1"),
    pytest.param(1, 32, 5, 2, 0, 5, 70, 1, 2, 3, 60, 32, ("tail", "ragged"), id="fused32-bf16-tail-channels-Ch32"),
    pytest.param(0, 56, 5, 2, 0, 5, 70, 1, 2, 3, 60, 64, ("tail", "ragged"), id="fused64-f32-tail-channels-Ch56"),
]


@pytest.mark.parametrize("dt,Ch,O,N,n0,H,W,oy,ox,Hc,Wc,want_chv,tags", FUSED_CASES)
def test_head_loss_fused_elementwise(lib, dt, Ch, O, N, n0, H, W, oy, ox, Hc, Wc, want_chv, tags):
    Chp, chv, w_lds, fwd, bwd = head_dispatch(dt, Ch, O)
    assert Chp <= 128 and Chp % 4 == 0 and chv == want_chv      # nint_head_loss_fused: Chp > 128 -> NINT_E_SHAPE; CHV by Chp
    lds = (O * chv + min(O, 64) * 64) * 4                         # nint_head_loss_fused: weights [O][CHV] + one output chunk of dpred
    assert lds + 8192 <= 160 * KIB and head_fused_holds(Chp, O)
    assert ("window" in tags) == (w_lds > 64 * KIB)
    assert fwd == bwd == f"staged{chv}"                           # the unfused pair runs the same staged arithmetic
    if O == 1088:
        assert not head_fused_holds(Chp, O + 1)
    npix = N * H * W
    assert ("optin" in tags) == (lds + 8192 > 64 * KIB)           # hipFuncSetAttribute branch
    assert ("many" in tags) == ((npix + 63) // 64 > LOSS_BLOCKS_MAX)
    if "ragged" in tags:
        assert npix % 64 != 0
    if "tail" in tags:
        assert Ch > chv - 12 and npix > 64
    if "asym" in tags:
        assert oy != H - Hc - oy and ox != W - Wc - ox
    if "full" in tags:
        assert (oy, ox, Hc, Wc) == (0, 0, H, W)
    if "chunks" in tags:
        assert O > 64                                             # HEAD_OCH: the outputs go through LDS in chunks of 64
    g, Chp, hsl, h, w, b, rng = head_inputs(lib, dt, Ch, O, N, n0, H, W, 2, 40 + Ch + O)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(f32)
    before = np.array([1.0, 2.0, -3.0, 4.0, 5.0, 6.0, -7.0, 8.0])
    dpred = torch.full((N, O, H, W), 7.0, device="cuda")
    dh = torch.full((N, H, W, Chp), 7.0, device="cuda").to(et(dt))
    sc, st = torch.zeros(8194, device="cuda"), dev(before)
    wd, bd, yd = dev(w), dev(b), dev(y)
    assert lib.nint_head_loss_fused(P(hsl), n0, N, Ch, Chp, O, P(wd), P(bd), P(yd), P(dpred), P(dh), P(sc), P(st),
                                    C.byref(g), oy, ox, Hc, Wc, dt, None) == 0
    ref = SM.head_loss_fused(h, w, b, y, oy, ox, Chp, bool(dt))
    got_dp, got_dh = host(dpred), decode(dh, dt)
    r1 = SM.ratio(got_dp, *ref["dpred"], what="fused dpred")
    outside = np.ones((H, W), bool)
    outside[oy:oy + Hc, ox:ox + Wc] = False
    assert not got_dp[:, :, outside].any()                        # outside the crop: exactly zero
    r2 = SM.ratio(got_dh, *ref["dh"], what="fused dh")
    assert not got_dh[..., Ch:].any()
    r3 = SM.check_stats(before, host(st), [ref["loss"]], ref["sum_tol"], what="fused stats")
    r4 = SM.check_loss_scalar(host(sc)[0], ref["loss"]["loss"], ref["loss_extra"], what="fused loss")
    print(f"fused chv={chv} dt={dt}: worst ratio dpred {r1:.3f}, dh {r2:.3f}, stats {r3:.3f}, loss {r4:.3f}")


# =========================================================================== loss
def loss_call(lib, pred, y, oy, ox, st, with_dpred=True, with_stats=True):
    N, O, H, W = pred.shape
    Hc, Wc = y.shape[2:]
    dp = torch.full((N, O, H, W), 7.0, device="cuda") if with_dpred else None
    sc = torch.zeros(8194, device="cuda")
    pd, yd = dev(pred), dev(y)
    assert lib.nint_loss_mse_l1_crop(P(pd), P(yd), P(dp), P(sc), P(st) if with_stats else None, N, O, H, W, oy, ox,
                                     Hc, Wc, None) == 0
    ref = SM.loss(pred, y, oy, ox)
    if with_dpred:
        SM.check_equal(host(dp), ref["dpred"], "dpred")            # bit for bit, +0 outside the crop
    SM.check_loss_scalar(host(sc)[0], ref["loss"], what="loss")
    return ref


def loss_inputs(seed, N, O, H, W, oy, ox, Hc, Wc, const=None, same=False):
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((N, O, H, W)).astype(f32)
    y = rng.standard_normal((N, O, Hc, Wc)).astype(f32) if const is None else np.full((N, O, Hc, Wc), const, f32)
    if same:
        pred[:, :, oy:oy + Hc, ox:ox + Wc] = y
    else:
        pred[0, 0, oy, ox] = y[0, 0, 0, 0]                         # sign(0) = 0
    return pred, y, oy, ox


@pytest.mark.parametrize("const,same,r2", [pytest.param(0.5, False, 0.0, id="r2[ss_tot<=0,residual>0]=0"),
                                           pytest.param(-2.0, True, 1.0, id="r2[ss_tot<=0,residual==0]=1")])
def test_loss_constant_target_r2_conventions(lib, const, same, r2):
    args = loss_inputs(50, 2, 3, 9, 11, 2, 3, 5, 6, const, same)
    y64 = args[1].astype(np.float64)
    n = y64.size
    assert float((y64 * y64).sum()) - float(y64.sum()) ** 2 / n <= 0.0      # loss_final_kernel: ss_tot > 0.0 ? ... : (s0 == 0.0 ? 1 : 0)
    before = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0, 1.0])
    st = dev(before)
    ref = loss_call(lib, *args, st)
    assert ref["r2"] == r2 and ref["r2_tol"] == 0.0 and (ref["sums"][0] == 0.0) == same
    SM.check_stats(before, host(st), [ref])
    assert host(st)[6] == 3.0 + r2


def test_loss_three_calls_accumulate_into_one_stats(lib):
    before = np.array([1.0, 2.0, -3.0, 4.0, 5.0, 6.0, -7.0, 8.0])
    st = dev(before)
    calls = [loss_inputs(51, 2, 3, 9, 11, 2, 3, 5, 6), loss_inputs(52, 1, 1, 7, 9, 0, 0, 7, 9), loss_inputs(53, 3, 2, 12, 20, 1, 5, 8, 9)]
    refs = [loss_call(lib, *a, st) for a in calls]
    r = SM.check_stats(before, host(st), refs)
    print(f"loss stats over three calls: worst ratio {r:.3f}")


def test_loss_without_dpred_and_without_stats(lib):
    args = loss_inputs(54, 2, 3, 9, 11, 2, 3, 5, 6)
    st = dev(np.zeros(8))
    ref = loss_call(lib, *args, st, with_dpred=False)             # dpred == NULL: the sums are unchanged
    SM.check_stats(np.zeros(8), host(st), [ref])
    loss_call(lib, *args, None, with_stats=False)                 # stats == NULL: loss and dpred are unchanged


def test_loss_grid_stride_above_256x1024_elements(lib):
    N, O, H, W = 1, 3, 300, 300
    assert N * O * H * W > 256 * 1024                             # LOSS_BLOCKS workgroups of 1024 threads: the loop strides
    args = loss_inputs(55, N, O, H, W, 7, 9, 280, 275)
    st = dev(np.zeros(8))
    ref = loss_call(lib, *args, st)
    SM.check_stats(np.zeros(8), host(st), [ref])


# =========================================================================== pack / unpack
def pack_dispatch(ptr, dt, C_, W, Cp):
    """pack_btchw_impl: 'rows-vw{4,2,1}' (+ '-optin' above 64 KiB of LDS) or 'fallback'"""
    tile = C_ * (W + 1) * 4
    if tile <= 160 * KIB and Cp % (8 if dt else 4) == 0:
        vw = 4 if (ptr & 15) == 0 and W % 4 == 0 else (2 if (ptr & 7) == 0 and W % 2 == 0 else 1)
        return f"rows-vw{vw}" + ("-optin" if tile > 64 * KIB else "")
    return "fallback"


PACK_CASES = [
    # (dt, C, W, H, kf, float offset into an aligned buffer, branch)
    pytest.param(0, 5, 40, 5, 1, 0, "rows-vw4", id="rows-vw4-f32-W40"),
    pytest.param(1, 5, 40, 5, 1, 0, "rows-vw4", id="rows-vw4-bf16-W40"),
    pytest.param(1, 3, 40, 5, 5, 0, "rows-vw4", id="rows-vw4-bf16-W40-folded-k5"),
    pytest.param(0, 5, 38, 5, 1, 0, "rows-vw2", id="rows-vw2[W%4!=0]-f32-W38"),
    pytest.param(1, 5, 40, 5, 1, 2, "rows-vw2", id="rows-vw2[src 8-byte aligned: buf[2:]]-bf16-W40"),
    pytest.param(0, 5, 37, 5, 1, 0, "rows-vw1", id="rows-vw1[W odd]-f32-W37"),
    pytest.param(0, 5, 40, 5, 1, 1, "rows-vw1", id="rows-vw1[src 4-byte aligned: buf[1:]]-f32-W40"),
    pytest.param(1, 5, 38, 5, 3, 1, "rows-vw1", id="rows-vw1[src 4-byte aligned: buf[1:]]-bf16-W38-folded-k3"),
    pytest.param(1, 70, 240, 3, 1, 0, "rows-vw4-optin", id="rows-LDS-opt-in[tile>64KiB]-bf16-C70-W240"),
    pytest.param(0, 70, 238, 3, 1, 0, "rows-vw2-optin", id="rows-LDS-opt-in[tile>64KiB]-f32-C70-W238-vw2"),
    pytest.param(0, 172, 240, 2, 1, 0, "fallback", id="fallback[tile>160KiB]-f32-C172-W240-plain"),
    pytest.param(1, 172, 240, 2, 3, 0, "fallback", id="fallback[tile>160KiB]-bf16-C172-W240-folded-k3"),
]


@pytest.mark.parametrize("dt,Cc,W,H,kf,off,branch", PACK_CASES)
def test_pack_btchw_every_row_width_opt_in_and_fallback(lib, dt, Cc, W, H, kf, off, branch):
    B, T, Pd = 2, 2, 2
    g, gt = geom(lib, H, W, Pd)
    kc = lib.nint_kc(dt)
    Cp = (kf * Cc + kc - 1) // kc * kc
    rng = np.random.default_rng(60 + Cc + W + off)
    x = rng.standard_normal((B, T, Cc, H, W)).astype(f32)
    buf = torch.zeros(x.size + off, device="cuda")
    assert buf.data_ptr() % 16 == 0
    xd = buf[off:]
    xd.copy_(dev(x).reshape(-1))
    assert pack_dispatch(xd.data_ptr(), dt, Cc, W, Cp) == branch
    if "optin" in branch:
        assert Cc * (W + 1) * 4 > 64 * KIB
    if branch == "fallback":
        assert Cc * (W + 1) * 4 > 160 * KIB
    slab = torch.zeros(T * B, g.Hh, g.Wh, Cp, device="cuda", dtype=et(dt))
    if kf == 1:
        assert lib.nint_pack_btchw(P(xd), P(slab), B, T, Cc, Cp, C.byref(g), dt, None) == 0
    else:
        assert lib.nint_pack_btchw_xfold(P(xd), P(slab), B, T, Cc, kf, Cp, C.byref(g), dt, None) == 0
    got = decode(slab, dt)
    SM.check_equal(got, SM.pack_btchw(x, Cp, gt, kf, bool(dt)), f"pack {branch}")     # interior, halo, slack and channel padding
    # and back out of the slab, the second half of the images only (n0 > 0)
    n0, N = B, T * B - B
    out = torch.full((N, kf * Cc, H, W), 7.0, device="cuda")
    assert lib.nint_unpack_halo(P(slab), P(out), n0, N, kf * Cc, Cp, C.byref(g), dt, None) == 0
    SM.check_equal(host(out), SM.unpack_halo(got, n0, N, kf * Cc, gt), "unpack_halo n0 > 0")
    if kf == 1:
        SM.check_equal(host(out), stored(x, dt).transpose(1, 0, 2, 3, 4).reshape(T * B, Cc, H, W)[n0:], "round trip")


@pytest.mark.parametrize("dt", [pytest.param(0, id="f32"), pytest.param(1, id="bf16")])
def test_pack_and_unpack_compact_both_dtypes(lib, dt):
    N, Cc, H, W = 3, 5, 7, 11
    Cp = lib.nint_kc(dt)
    x = np.random.default_rng(61).standard_normal((N, Cc, H, W)).astype(f32)
    slab = torch.full((N, H, W, Cp), 7.0, device="cuda").to(et(dt))
    xd = dev(x)
    assert lib.nint_pack_compact(P(xd), P(slab), N, Cc, Cp, H, W, dt, None) == 0
    got = decode(slab, dt)
    SM.check_equal(got, SM.pack_compact(x, Cp, bool(dt)), "pack_compact")            # the channel padding is written as zeros
    out = torch.full((N, Cc, H, W), 7.0, device="cuda")
    assert lib.nint_unpack_compact(P(slab), P(out), N, Cc, Cp, H, W, dt, None) == 0
    SM.check_equal(host(out), SM.unpack_compact(got, Cc), "unpack_compact")
    SM.check_equal(host(out), stored(x, dt), "round trip")


@pytest.mark.parametrize("dt", [pytest.param(0, id="f32"), pytest.param(1, id="bf16")])
@pytest.mark.parametrize("Cc,k,W", [(3, 5, 9), (1, 3, 4), (5, 5, 37)])
def test_unfold_dx_elementwise(lib, dt, Cc, k, W):
    N, H = 3, 5
    kc = lib.nint_kc(dt)
    Cp = (k * Cc + kc - 1) // kc * kc
    G = stored(np.random.default_rng(62).standard_normal((N, H, W, Cp)), dt)
    dx = torch.full((N, Cc, H, W), 7.0, device="cuda")
    Gd = to_slab(G, dt)
    assert lib.nint_unfold_dx(P(Gd), P(dx), N, Cc, k, Cp, H, W, dt, None) == 0
    r = SM.ratio(host(dx), *SM.unfold_dx(G, Cc, k), what="unfold_dx")
    print(f"unfold_dx dt={dt}: worst ratio {r:.3f}")


# =========================================================================== preproc
PRE_MAX_B = 64                         # include/nint.h NINT_PRE_MAX_B


def pre_sources(rng, levs, nstatic, steps, H, W, offs=None):
    """records on the device, each in its own aligned buffer at a float offset offs[i]; returns (numpy records, device
    views, the buffers that own them)"""
    recs, views, bufs = [], [], []
    for i, lv in enumerate(levs):
        st = 1 if i >= len(levs) - nstatic else steps
        a = rng.standard_normal((st, lv, H, W)).astype(f32)
        off = offs[i] if offs else 0
        buf = torch.zeros(a.size + off, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[off:]
        v.copy_(dev(a).reshape(-1))
        recs.append(a); views.append(v); bufs.append(buf)
    return recs, views, bufs


def pre_vw(views, W):
    """nint_preproc_fuse_pad_static_slab: the widest row vector every source pointer allows"""
    vw = 4 if W % 4 == 0 else (2 if W % 2 == 0 else 1)
    for v in views:
        while vw > 1 and (v.data_ptr() & (4 * vw - 1)):
            vw >>= 1
    return vw


def pre_slab_run(lib, recs, views, nstatic, mean, std, t0, T, H, W, Hp, Wp, mode, dt, Cxp, kf, Pd=2):
    g, gt = geom(lib, Hp, Wp, Pd)
    B, nsrc = len(t0), len(recs)
    ptrs = (C.c_void_p * nsrc)(*[v.data_ptr() for v in views])
    lev = (C.c_int * nsrc)(*[r.shape[1] for r in recs])
    slab = torch.zeros(T * B, g.Hh, g.Wh, Cxp, device="cuda", dtype=et(dt))
    assert slab.data_ptr() % 16 == 0
    t0a = (C.c_int * B)(*t0)
    md, sd = dev(mean), dev(std)
    if nstatic:
        rc = lib.nint_preproc_fuse_pad_static_slab(ptrs, lev, nsrc, nstatic, P(md), P(sd), t0a, B, P(slab), Cxp,
                                                   kf if kf > 1 else 0, T, H, W, C.byref(g), mode, dt, None)
    else:
        rc = lib.nint_preproc_fuse_pad_slab(ptrs, lev, nsrc, P(md), P(sd), t0a, B, P(slab), Cxp, kf if kf > 1 else 0,
                                            T, H, W, C.byref(g), mode, dt, None)
    assert rc == 0
    want = SM.pack_btchw(SM.preproc(recs, nstatic, mean, std, t0, T, Hp, Wp, mode), Cxp, gt, kf, bool(dt))
    SM.check_equal(decode(slab, dt), want, "preproc slab")        # interior, halo, slack, channel padding


def pre_stats(rng, Cc):
    return rng.standard_normal(Cc).astype(f32), (0.5 + rng.random(Cc)).astype(f32)


@pytest.mark.parametrize("mode", [pytest.param(0, id="mode0-channel-flip"), pytest.param(1, id="mode1-reflect")])
@pytest.mark.parametrize("nstatic", [pytest.param(0, id="dynamic"), pytest.param(1, id="static")])
def test_preproc_two_chunks_B70_odd_pads_repeated_t0(lib, mode, nstatic):
    """B = 70 > NINT_PRE_MAX_B through the NCHW entries (second launch: output offset of chunk 1) and the slab entries
    (b0 = 64 image offset); Hp - H = 3 and Wp - W = 3 are odd, so pt != pb and pl != pr; t0 is non-zero and repeats."""
    B, T, H, W, Hp, Wp, steps = 70, 2, 6, 8, 9, 11, 7
    assert B > PRE_MAX_B and (Hp - H) % 2 == 1 and (Wp - W) % 2 == 1 and (Hp - H) // 2 != Hp - H - (Hp - H) // 2
    rng = np.random.default_rng(70 + mode)
    levs = [2, 1, 2]
    recs, views, _bufs = pre_sources(rng, levs, nstatic, steps, H, W)
    Cc = sum(levs)
    mean, std = pre_stats(rng, Cc)
    t0 = [int(v) for v in rng.integers(1, steps - T + 1, B)]
    t0[1] = t0[0]; t0[65] = t0[64] = t0[3]                        # repeated windows, across the chunk boundary too
    assert min(t0) > 0 and len(set(t0)) < B
    nsrc = len(levs)
    ptrs = (C.c_void_p * nsrc)(*[v.data_ptr() for v in views])
    lev = (C.c_int * nsrc)(*levs)
    out = torch.full((B, T, Cc, Hp, Wp), 7.0, device="cuda")
    md, sd = dev(mean), dev(std)
    t0a = (C.c_int * B)(*t0)
    if nstatic:
        assert lib.nint_preproc_fuse_pad_static_batch(ptrs, lev, nsrc, nstatic, P(md), P(sd), t0a, B, P(out), T, H, W, Hp, Wp, mode, None) == 0
    else:
        assert lib.nint_preproc_fuse_pad_batch(ptrs, lev, nsrc, P(md), P(sd), t0a, B, P(out), T, H, W, Hp, Wp, mode, None) == 0
    got = host(out)
    ref = SM.preproc(recs, nstatic, mean, std, t0, T, Hp, Wp, mode)
    SM.check_equal(got, ref, "preproc NCHW, two chunks")
    # the per-sample entry, its source pointers moved to the window's first step, gives the same bytes (one sample of each chunk)
    one = torch.full((T, Cc, Hp, Wp), 7.0, device="cuda")
    for b in (0, 1, 63, 64, 65, 69):
        p1 = (C.c_void_p * nsrc)(*[v.data_ptr() + (0 if i >= nsrc - nstatic else 4 * t0[b] * levs[i] * H * W) for i, v in enumerate(views)])
        if nstatic:
            assert lib.nint_preproc_fuse_pad_static(p1, lev, nsrc, nstatic, P(md), P(sd), P(one), T, H, W, Hp, Wp, mode, None) == 0
        else:
            assert lib.nint_preproc_fuse_pad(p1, lev, nsrc, P(md), P(sd), P(one), T, H, W, Hp, Wp, mode, None) == 0
        SM.check_equal(host(one), got[b], f"per-sample entry, sample {b}")
        # and the literal restatement of the reference code (concatenate / fliplr)
        fused = np.concatenate([np.repeat(r, T, axis=0) if i >= nsrc - nstatic else r[t0[b]:t0[b] + T] for i, r in enumerate(recs)], axis=1)
        want = PO.padding_data_4d(PO.zscore(fused, mean, std), (Hp, Wp), "reference" if mode == 0 else "reflect").astype(f32)
        SM.check_equal(got[b], want, f"reference restatement, sample {b}")
    # the slab entries: image t*B + b0 + b
    for dt, kf in ((1, 1), (0, 3)):
        Cxp = (kf * Cc + 7) // 8 * 8
        assert pre_vw(views, W) == 4
        pre_slab_run(lib, recs, views, nstatic, mean, std, t0, T, H, W, Hp, Wp, mode, dt, Cxp, kf)


@pytest.mark.parametrize("dt", [pytest.param(0, id="f32"), pytest.param(1, id="bf16")])
def test_preproc_slab_lds_opt_in_40_levels(lib, dt):
    levels, T, H, W, Hp, Wp, steps = 40, 1, 4, 144, 7, 149, 3
    levs = [levels, levels, levels, 1, 1]
    Cc = sum(levs)
    tile_bytes = (Cc * 24 + 15) // 16 * 16 + Cc * (W + 1) * 4     # sizeof(RowDesc) = 24: pointer, two floats, an int, padded
    assert Cc == 122 and tile_bytes > 64 * KIB and tile_bytes <= 160 * KIB
    rng = np.random.default_rng(71)
    recs, views, _bufs = pre_sources(rng, levs, 0, steps, H, W)
    mean, std = pre_stats(rng, Cc)
    assert pre_vw(views, W) == 4
    pre_slab_run(lib, recs, views, 0, mean, std, [2, 0], T, H, W, Hp, Wp, 0, dt, 128, 1)


@pytest.mark.parametrize("offs,vw", [pytest.param([0, 1, 0], 1, id="vw1[one source 4-byte aligned]"),
                                     pytest.param([0, 2, 0], 2, id="vw2[one source 8-byte aligned]"),
                                     pytest.param([0, 0, 0], 4, id="vw4[all sources 16-byte aligned]")])
@pytest.mark.parametrize("mode", [0, 1])
def test_preproc_slab_source_alignment_narrows_the_row_vector(lib, offs, vw, mode):
    T, H, W, Hp, Wp, steps = 2, 5, 8, 8, 13, 4                    # Hp - H = 3, Wp - W = 5: both odd
    levs = [2, 3, 1]
    rng = np.random.default_rng(72)
    recs, views, _bufs = pre_sources(rng, levs, 1, steps, H, W, offs)
    assert pre_vw(views, W) == vw
    mean, std = pre_stats(rng, sum(levs))
    pre_slab_run(lib, recs, views, 1, mean, std, [2, 2, 1], T, H, W, Hp, Wp, mode, 1, 8, 1)
    pre_slab_run(lib, recs, views, 1, mean, std, [1, 0, 2], T, H, W, Hp, Wp, mode, 0, 20, 3)


@pytest.mark.parametrize("W,vw", [pytest.param(6, 2, id="W6-vw2"), pytest.param(7, 1, id="W7-vw1")])
def test_preproc_16_sources_nchw_and_slab(lib, W, vw):
    nsrc, T, H, Hp, Wp, steps = 16, 2, 5, 8, W + 3, 4
    levs = [1] * nsrc
    rng = np.random.default_rng(73)
    recs, views, _bufs = pre_sources(rng, levs, 3, steps, H, W)
    assert nsrc == 16 and pre_vw(views, W) == vw                  # PRE_MAX_SRC
    mean, std = pre_stats(rng, nsrc)
    t0 = [2, 2, 1]
    md, sd = dev(mean), dev(std)
    for mode in (0, 1):
        ptrs = (C.c_void_p * nsrc)(*[v.data_ptr() for v in views])
        lev = (C.c_int * nsrc)(*levs)
        out = torch.full((len(t0), T, nsrc, Hp, Wp), 7.0, device="cuda")
        assert lib.nint_preproc_fuse_pad_static_batch(ptrs, lev, nsrc, 3, P(md), P(sd), (C.c_int * 3)(*t0), 3, P(out), T, H, W,
                                                      Hp, Wp, mode, None) == 0
        SM.check_equal(host(out), SM.preproc(recs, 3, mean, std, t0, T, Hp, Wp, mode), "16 sources NCHW")
        pre_slab_run(lib, recs, views, 3, mean, std, t0, T, H, W, Hp, Wp, mode, 1, 16, 1)
