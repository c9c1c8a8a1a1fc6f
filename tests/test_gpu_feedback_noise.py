"""GPU: noise on the fed-back value -- ``net(x, free_from=s | free_mask=M, feedback_noise=InputNoise(...))``,
nint_seq_fwd_stochastic, nint_head_feedback_noise: a fed step t stores round_ET( p + sigma[o] * z ), p the f32 prediction of the
step before (a residual head: base included), z nint_noise_normal's number for (pixel, o, step0 + t, lane0 + b), the product and
the sum two f32 operations.

The contract is the closed loop's: the stochastic pass equals, bit for bit, the open-loop pass over an input that already
holds the stored values.  That input is built on the CPU from the pass's own per-step predictions and from z.  Shapes:
closed_loop_model.CASES (B = 2, T = 4, 13 x 37), both storage types."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_model as CLM
import test_gpu_closed_loop as CL
import test_gpu_memory_contract as MC

pytestmark = pytest.mark.gpu
BOTH = ("f32", "bf16")
SEED, DRAW, STEP0, LANE0 = 7, 1, 3, 5


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


def sigmas(c, zero=None):
    sig = [0.05 * (1 + o) for o in range(c["O"])]
    if zero is not None:
        sig[zero] = 0.0
    return tuple(sig)


def noise_of(pkg, sig, seed=SEED, lane0=LANE0):
    from nasa_niswan_amd.engine import InputNoise
    return InputNoise(sig, seed=seed, draw=DRAW, step0=STEP0, lane0=lane0)


def normals(pkg, c, B, seed=SEED, lane0=LANE0):
    """z (T, B, O, H, W) f32 on the CPU, from nint_noise_normal"""
    from nasa_niswan_amd import _lib
    lib = pkg.load_library()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), c["H"], c["W"], 2) == 0
    out = torch.empty(c["T"] * B, c["O"], c["H"], c["W"], device="cuda")
    assert lib.nint_noise_normal(C.c_void_p(out.data_ptr()), B, c["T"], c["O"], seed, DRAW, STEP0, lane0, C.byref(g), None) == 0
    torch.cuda.synchronize()
    return out.cpu().view(c["T"], B, c["O"], c["H"], c["W"])


def run(net, eng, X, feed, fnoise=None, residual=False):
    """one forward pass through the engine: the input slab's bytes, the per-step head and the last prediction"""
    B, T, _, H, W = X.shape
    ws = eng.acquire(B, T, H, W, False, False)
    try:
        net._pack_weights(eng)
        fb = None if feed is None else (net.conv.weight, net.conv.bias, feed)
        eng.forward(ws, X, feedback=fb, residual=net.conv.weight.shape[0] if residual else False, feedback_noise=fnoise)
        res = dict(xs=ws.xs.clone(), seq=eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).clone(),
                   pred=eng.head_forward(ws, net.conv.weight, net.conv.bias).clone(), stochastic=ws.feedback.noise is not None)
        for l in range(len(eng.cfgs)):
            res[f"h{l}"] = ws.h[l].clone()
    finally:
        eng.release(ws)
    torch.cuda.synchronize()
    return res


def stored_input(c, X, seq, fed_bt, sig, z):
    """X (CPU) with the feedback channels of every fed (b, t) replaced by f32(p_{t-1}) + f32(sigma * z_t): two f32 operations, and
    p alone where sigma is 0"""
    B, T, O_ = X.shape[0], X.shape[1], c["O"]
    p = seq.cpu().view(B, T, O_, c["H"], c["W"])
    sg = torch.tensor(sig, dtype=torch.float32).view(1, O_, 1, 1)
    X2 = X.clone()
    for t in range(1, T):
        add = sg * z[t]                                                     # (B, O, H, W), one f32 product
        v = torch.where(sg != 0, p[:, t - 1] + add, p[:, t - 1])            # one f32 sum
        for b in range(B):
            if fed_bt[b][t]:
                X2[b, t, c["C"] - O_:] = v[b]
    return X2


def from_step(c, s, B=None):
    return [[t >= s for t in range(c["T"])] for _ in range(c["B"] if B is None else B)]


def same(a, b, what):
    for k in a:
        if k != "stochastic":
            assert torch.equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------ the bit contract
@pytest.mark.parametrize("cyclic", [False, True], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(CLM.CASES))
def test_stochastic_closed_loop_is_the_open_loop_on_the_stored_input(pkg, case, dtype, cyclic):
    c = CLM.CASES[case]
    net, eng = CL.make_net(pkg, case, dtype, cyclic)
    X = CL.data_of(c)["X"]
    sig = sigmas(c)
    z = normals(pkg, c, c["B"])
    with torch.no_grad():
        for s in (1, 2):
            a = run(net, eng, X.cuda(), s, noise_of(pkg, sig))
            assert a["stochastic"]
            b = run(net, eng, stored_input(c, X, a["seq"], from_step(c, s), sig, z).cuda(), None)
            same(a, b, (case, dtype, cyclic, s))
            quiet = run(net, eng, X.cuda(), s)
            assert not torch.equal(a["seq"], quiet["seq"]) and not quiet["stochastic"]            # the noise is in fact there
            assert torch.equal(a["seq"][:, :s * c["O"]], quiet["seq"][:, :s * c["O"]])            # ... from the first fed step on
        # the module takes the same route
        pred = net(X.cuda(), free_from=1, feedback_noise=noise_of(pkg, sig))
        assert torch.equal(pred, run(net, eng, X.cuda(), 1, noise_of(pkg, sig))["pred"])


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", ["thin", "wide"])
def test_with_a_residual_head(pkg, case, dtype):
    c = CLM.CASES[case]
    net, eng = CL.make_net(pkg, case, dtype, True, residual=True)
    X = CL.data_of(c)["X"]
    sig, z = sigmas(c), normals(pkg, c, c["B"])
    with torch.no_grad():
        a = run(net, eng, X.cuda(), 1, noise_of(pkg, sig), residual=True)         # seq: p_t with its base
        b = run(net, eng, stored_input(c, X, a["seq"], from_step(c, 1), sig, z).cuda(), None, residual=True)
        same(a, b, (case, dtype))
        assert not torch.equal(a["seq"], run(net, eng, X.cuda(), 1, residual=True)["seq"])


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", ["thin", "wide"])
def test_under_a_mask_only_fed_images_draw_and_unfed_bytes_stay(pkg, case, dtype):
    c = CLM.CASES[case]
    net, eng = CL.make_net(pkg, case, dtype, False)
    X = CL.data_of(c)["X"]
    sig, z = sigmas(c), normals(pkg, c, c["B"])
    fed = [[0, 1, 0, 1], [0, 0, 1, 1]]                                         # step 1 and 2: one image fed, the other not
    with torch.no_grad():
        a = run(net, eng, X.cuda(), torch.tensor(fed, dtype=torch.uint8), noise_of(pkg, sig))
        b = run(net, eng, stored_input(c, X, a["seq"], fed, sig, z).cuda(), None)
        same(a, b, (case, dtype))                                              # xs too: an unfed image keeps the caller's bytes


@pytest.mark.parametrize("dtype", BOTH)
def test_a_zero_sigma_channel_stores_what_the_noiseless_launch_stores(pkg, dtype):
    c = CLM.CASES["wide"]                                                      # a plain slab: channel c0 + o of the pixel
    net, eng = CL.make_net(pkg, "wide", dtype, False)
    X = CL.data_of(c)["X"]
    sig, z = sigmas(c, zero=1), normals(pkg, c, c["B"])
    B, T, H, W, s = c["B"], c["T"], c["H"], c["W"], 2
    with torch.no_grad():
        a = run(net, eng, X.cuda(), s, noise_of(pkg, sig))
        same(a, run(net, eng, stored_input(c, X, a["seq"], from_step(c, s), sig, z).cuda(), None), dtype)
        quiet = run(net, eng, X.cuda(), s)
        ws = eng.acquire(B, T, H, W, False, False)
        P, Hh, Wh, Cxp = ws.g.P, ws.g.Hh, ws.g.Wh, ws.Cxp0
        eng.release(ws)
    et = torch.float32 if dtype == "f32" else torch.bfloat16
    view = lambda r: r["xs"].view(et).view(T * B, Hh, Wh, Cxp)[s * B:(s + 1) * B, P:P + H, P:P + W, c["C"] - c["O"]:c["C"]]
    va, vq = view(a), view(quiet)                                             # the first fed step: both saw the same h
    assert torch.equal(va[..., 1], vq[..., 1])
    assert not torch.equal(va[..., 0], vq[..., 0]) and not torch.equal(va[..., 2], vq[..., 2])


# ------------------------------------------------------------------ determinism and composition
@pytest.mark.parametrize("dtype", BOTH)
def test_seeds_repeat_and_lanes_compose(pkg, dtype):
    c = CLM.CASES["thin"]
    net, eng = CL.make_net(pkg, "thin", dtype, True)
    X = CL.data_of(c)["X"].cuda()
    sig = sigmas(c)
    with torch.no_grad():
        a = run(net, eng, X, 1, noise_of(pkg, sig, seed=3))
        again = run(net, eng, X, 1, noise_of(pkg, sig, seed=3))
        other = run(net, eng, X, 1, noise_of(pkg, sig, seed=4))
        same(a, again, "the same seed")
        assert not torch.equal(a["seq"], other["seq"])
        # lane0 = 1 on the second image alone is lane 1 of the B = 2 run from lane0 = 0
        two = run(net, eng, X, 1, noise_of(pkg, sig, lane0=0))
        one = run(net, eng, X[1:2].contiguous(), 1, noise_of(pkg, sig, lane0=1))
        assert torch.equal(one["seq"][0], two["seq"][1]) and torch.equal(one["pred"][0], two["pred"][1])


# ------------------------------------------------------------------ unchanged paths
@pytest.mark.parametrize("dtype", BOTH)
def test_none_and_zero_std_are_the_call_without_it(pkg, dtype):
    from nasa_niswan_amd import _lib
    from nasa_niswan_amd.engine import InputNoise
    lib = pkg.load_library()
    c = CLM.CASES["thin"]
    net, eng = CL.make_net(pkg, "thin", dtype, False)
    X = CL.data_of(c)["X"].cuda()
    with torch.no_grad():
        quiet = run(net, eng, X, 1)
        for fn in (None, InputNoise(0.0, seed=9), InputNoise((0.0,) * c["O"])):
            r = run(net, eng, X, 1, fn)
            assert not r["stochastic"]                       # the engine names the entry it named before: no noise structure
            same(r, quiet, fn)
        assert torch.equal(net(X, free_from=1, feedback_noise=InputNoise(0.0)), net(X, free_from=1))
        # a call that feeds nothing has nothing to put the noise on: the call without the argument, and no workspace is kept
        live = noise_of(pkg, sigmas(c))
        plain = net(X)
        assert torch.equal(net(X, feedback_noise=live), plain)
        assert torch.equal(net(X, free_mask=torch.zeros(c["B"], c["T"], dtype=torch.uint8), feedback_noise=live), plain)
        assert torch.equal(net(X, free_from=c["T"], feedback_noise=live), plain)
        assert not any(w.in_use for pool in eng.pool.values() for w in pool)
        assert not run(net, eng, X, None, live)["stochastic"]


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("dtype", BOTH)
def test_the_pass_entry_without_a_noise_structure_is_the_entry_it_extends(pkg, dtype, residual):
    """nint_seq_fwd_stochastic with fn = NULL, and with a structure whose sigma is NULL, against nint_seq_fwd_sampled /
    nint_seq_fwd_residual on the same workspace: every byte of the input slab and of every h and c slab"""
    from nasa_niswan_amd import _lib
    lib = pkg.load_library()
    c = CLM.CASES["wide"]
    net, eng = CL.make_net(pkg, "wide", dtype, True, residual=residual)
    X = CL.data_of(c)["X"].cuda()
    fed = torch.tensor([[0, 1, 0, 1], [0, 0, 1, 1]], dtype=torch.uint8)
    with torch.no_grad():
        ws = eng.acquire(c["B"], c["T"], c["H"], c["W"], False, False)
        try:
            net._pack_weights(eng)
            for feed in (1, fed):
                eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, feed), residual=c["O"] if residual else False)
                want = [ws.xs.clone()] + [t.clone() for t in list(ws.h) + list(ws.c)]
                for fn in (None, C.byref(_lib.NintFeedbackNoise())):
                    for t in [ws.xs] + list(ws.h) + list(ws.c):
                        t.zero_()
                    eng.pack_input(ws, X)
                    fb, fm = ws.feedback.fb, ws.feedback.fm
                    assert lib.nint_seq_fwd_stochastic(C.byref(ws.seq), C.byref(fb), C.byref(fm), int(residual), fn, _lib.stream_ptr()) == 0
                    torch.cuda.synchronize()
                    got = [ws.xs] + list(ws.h) + list(ws.c)
                    assert all(torch.equal(u, v) for u, v in zip(got, want)), (dtype, residual, fn is None)
        finally:
            eng.release(ws)


def test_the_launch_entry_alone(pkg):
    """nint_head_feedback_noise with fn = NULL is nint_head_feedback_res: the same bytes; with fn it writes what the pass's
    launch of that step writes"""
    from nasa_niswan_amd import _lib
    lib = pkg.load_library()
    c = CLM.CASES["wide"]
    net, eng = CL.make_net(pkg, "wide", "bf16", False)
    X = CL.data_of(c)["X"].cuda()
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    sig = sigmas(c)
    with torch.no_grad():
        whole = run(net, eng, X, 1, noise_of(pkg, sig))["xs"].view(T * B, -1)
        ws = eng.acquire(B, T, H, W, False, False)
        try:
            net._pack_weights(eng)
            eng.forward(ws, X)
            top, cfg = eng.layers[-1], eng.cfgs[0]
            w, b = net.conv.weight.reshape(c["O"], -1).contiguous(), net.conv.bias
            outs = []
            for name, tail in (("nint_head_feedback_res", ()), ("nint_head_feedback_noise", (None, 0))):
                before = ws.xs.clone()
                rc = getattr(lib, name)(C.c_void_p(ws.h[-1].data_ptr()), B, B, eng.cfgs[-1].Ch, top.Chp, c["O"], C.c_void_p(w.data_ptr()),
                                        C.c_void_p(b.data_ptr()), C.c_void_p(ws.xs.data_ptr()), B, cfg.Cx, ws.Cxp0, cfg.Cx - c["O"], 0, 0, -1,
                                        None, C.byref(ws.g), eng.dt, None, *tail)
                assert rc == 0, (name, rc)
                torch.cuda.synchronize()
                outs.append(ws.xs.clone())
                assert not torch.equal(outs[-1], before)
                ws.xs.copy_(before)
            assert torch.equal(outs[0], outs[1])
            sd = torch.tensor(sig, dtype=torch.float32, device="cuda")
            fn = _lib.NintFeedbackNoise()
            fn.sigma, fn.seed, fn.draw, fn.step0, fn.lane0 = sd.data_ptr(), SEED, DRAW, 0, LANE0
            rc = lib.nint_head_feedback_noise(C.c_void_p(ws.h[-1].data_ptr()), B, B, eng.cfgs[-1].Ch, top.Chp, c["O"], C.c_void_p(w.data_ptr()),
                                              C.c_void_p(b.data_ptr()), C.c_void_p(ws.xs.data_ptr()), B, cfg.Cx, ws.Cxp0, cfg.Cx - c["O"], 0, 0,
                                              -1, None, C.byref(ws.g), eng.dt, None, C.byref(fn), STEP0 + 1)
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert torch.equal(ws.xs.view(T * B, -1)[B:2 * B], whole[B:2 * B])        # step 1 of the pass: the same h, the same draw
        finally:
            eng.release(ws)
