"""Carried state on the device: `ConvLSTM.forward(x, state, return_state=...)`, `ConvLSTMState`, the state
hand-off kernel `nint_state_copy`, `FusedTrainer(stateful=True)` and `inference.predict_stream`.

Two routes that launch the same kernels on the same bytes are compared bit for bit (torch.equal); numbers are compared with
the CPU oracle in f64 under the bounds of tests/test_gpu_shapes.py::check (f32: max abs error <= 1e-3 max|ref| + 1e-5; bf16:
relative L2 <= 2e-2)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
# two layers: the merged-grid modes are live; one layer under k = 5: the folded-input shape of the contract tests
SHAPES = {
    "two": dict(C=5, hidden=[16, 8], ks=[3, 3], out=2, B=2, H=9, W=17),
    "one": dict(C=3, hidden=[8], ks=[5], out=1, B=2, H=8, W=20),
}


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


def params_of(shape, seed=0):
    from oracle import convlstm_oracle as O
    s = SHAPES[shape]
    return O.synth_params(s["C"], s["hidden"], s["ks"], len(s["hidden"]), out_channels=s["out"], seed=seed)


def make_net(pkg, shape, dtype, seq=True, seed=0):
    s = SHAPES[shape]
    net = pkg.ConvLSTM(s["C"], s["hidden"], s["ks"], len(s["hidden"]), out_channels=s["out"], return_sequence=seq,
                       compute_dtype=dtype).cuda()
    net.load_state_dict(params_of(shape, seed))
    return net


def data(shape, T, seed):
    """X, cotangents for pred and seq, an initial state (h scaled 0.5: inside tanh's range) and cotangents for the final one"""
    s = SHAPES[shape]
    rng = np.random.default_rng(seed)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    B, H, W = s["B"], s["H"], s["W"]
    d = dict(X=f(B, T, s["C"], H, W), R=f(B, s["out"], H, W), RS=f(B, T * s["out"], H, W))
    d["h0"] = [0.5 * f(B, ch, H, W) for ch in s["hidden"]]
    d["c0"] = [f(B, ch, H, W) for ch in s["hidden"]]
    d["Rh"] = [f(B, ch, H, W) for ch in s["hidden"]]
    d["Rc"] = [f(B, ch, H, W) for ch in s["hidden"]]
    return d


def check(res, ref, dtype, keys=None):
    """tests/test_gpu_shapes.py::check"""
    for k in (keys or ref):
        a, b = res[k].detach().double().cpu().numpy(), ref[k].detach().double().cpu().numpy()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if dtype == "f32":
            err, top = np.abs(a - b).max(), np.abs(b).max()
            print(f"  {k}: max abs err {err:.2e} (ref max {top:.2e})")
            assert err <= 1e-3 * top + 1e-5, (k, err, top)
        else:
            r = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
            print(f"  {k}: rel-L2 {r:.2e}")
            assert r <= 2e-2, (k, r)


# ------------------------------------------------------------------ 1. nint_state_copy
SENT, FILL, GUARD = 0xA5, 0x5A, 256


class Blocks:
    """per region (h and c of every layer) one buffer [guard | B images | guard]"""

    def __init__(self, nbytes, B, fill, seed=None):
        self.B, self.nbytes, self.buf = B, nbytes, []
        for i, n in enumerate(nbytes):
            t = torch.full((2 * GUARD + B * n,), SENT, dtype=torch.uint8, device="cuda")
            if seed is None:
                t[GUARD:GUARD + B * n] = fill
            else:
                gen = torch.Generator().manual_seed(seed + i)
                t[GUARD:GUARD + B * n] = torch.randint(0, 256, (B * n,), dtype=torch.uint8, generator=gen).cuda()
            self.buf.append(t)

    def ptrs(self, which, off=0):
        L = len(self.buf) // 2
        return (C.c_void_p * L)(*[self.buf[2 * l + which].data_ptr() + GUARD + off for l in range(L)])

    def image(self, r, b):
        n = self.nbytes[r]
        return self.buf[r][GUARD + b * n:GUARD + (b + 1) * n]

    def guards_intact(self):
        return all(bool((t[:GUARD] == SENT).all()) and bool((t[-GUARD:] == SENT).all()) for t in self.buf)

    def snapshot(self):
        return [t.clone() for t in self.buf]


def geometry(H, W, P, Chp, dt):
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    g = _lib.NintGeom()
    assert lib.nint_geom_make(C.byref(g), H, W, P) == 0
    es = 2 if dt == 1 else 4
    nbytes = []
    for c in Chp:
        nbytes += [g.Hh * g.Wh * c * es, H * W * c * 4]
    assert all(n % 64 == 0 for n in nbytes)
    return lib, g, nbytes


def state_copy(lib, g, dt, Chp, dst, src, lane, L=None, dst_ptrs=None, src_ptrs=None):
    L = len(Chp) if L is None else L
    chp = (C.c_int32 * len(Chp))(*Chp)
    ln = None if lane is None else (C.c_int32 * len(lane))(*lane)
    hd, cd = dst_ptrs or (dst.ptrs(0), dst.ptrs(1))
    hs, cs = src_ptrs or (src.ptrs(0), src.ptrs(1))
    rc = lib.nint_state_copy(hd, cd, hs, cs, chp, L, dst.B, src.B, ln, C.byref(g), dt, None)
    torch.cuda.synchronize()
    return rc


def assert_mapped(dst, src, lane):
    for r in range(len(dst.buf)):
        for b, s in enumerate(lane):
            got = dst.image(r, b)
            if s < 0:
                assert not bool(got.any()), (r, b)             # all zero bits
            else:
                assert torch.equal(got, src.image(r, s)), (r, b, s)
    assert dst.guards_intact() and src.guards_intact()


@pytest.mark.parametrize("dt,Chp", [(0, (32, 16)), (1, (32, 32))])
def test_state_copy_is_exact(pkg, dt, Chp):
    lib, g, nbytes = geometry(9, 17, 2, Chp, dt)
    src = Blocks(nbytes, 2, None, seed=11)
    before = src.snapshot()
    dst = Blocks(nbytes, 3, FILL)
    lane = [1, -1, 0]
    assert state_copy(lib, g, dt, Chp, dst, src, lane) == 0
    assert_mapped(dst, src, lane)
    assert all(torch.equal(a, b) for a, b in zip(before, src.buf))              # the source is read only
    # identity: a bit copy
    dst2 = Blocks(nbytes, 2, FILL)
    assert state_copy(lib, g, dt, Chp, dst2, src, None) == 0
    assert_mapped(dst2, src, [0, 1])


@pytest.mark.parametrize("dt,Chp", [(0, (32, 16)), (1, (32, 32))])
def test_state_copy_splits_large_batches(pkg, dt, Chp):
    """B_dst = 65 > NINT_PRE_MAX_B: the second launch's destination offset and lane slice"""
    lib, g, nbytes = geometry(3, 5, 2, Chp, dt)
    src = Blocks(nbytes, 3, None, seed=5)
    dst = Blocks(nbytes, 65, FILL)
    lane = [-1 if b % 4 == 3 else b % 3 for b in range(65)]
    lane[64] = 2
    assert state_copy(lib, g, dt, Chp, dst, src, lane) == 0
    assert_mapped(dst, src, lane)
    src65 = Blocks(nbytes, 65, None, seed=6)
    assert state_copy(lib, g, dt, Chp, dst, src65, None) == 0
    assert_mapped(dst, src65, list(range(65)))


def test_state_copy_argument_errors_leave_the_destination_untouched(pkg):
    dt, Chp = 1, (32, 32)
    lib, g, nbytes = geometry(9, 17, 2, Chp, dt)
    src = Blocks(nbytes, 2, None, seed=3)
    dst = Blocks(nbytes, 3, FILL)
    before = dst.snapshot()
    E_ARG, E_ALIGN = -1, -4
    ok = [1, -1, 0]
    hd, cd, hs, cs = dst.ptrs(0), dst.ptrs(1), src.ptrs(0), src.ptrs(1)
    cases = [
        ("NULL h_dst", dict(dst_ptrs=(None, cd)), ok, None, E_ARG),
        ("NULL c_src", dict(src_ptrs=(hs, None)), ok, None, E_ARG),
        ("L = 0", {}, ok, 0, E_ARG),
        ("L = 9", {}, ok, 9, E_ARG),
        ("lane = B_src", {}, [1, 2, 0], None, E_ARG),
        ("lane = -2", {}, [1, -2, 0], None, E_ARG),
        ("identity with B_dst != B_src", {}, None, None, E_ARG),
        ("overlap: h source inside the h destination", dict(src_ptrs=(dst.ptrs(0, nbytes[0]), cs)), [0, 0, 0], None, E_ARG),
        ("overlap: c destination = c source", dict(dst_ptrs=(hd, src.ptrs(1))), ok, None, E_ARG),
        ("misaligned h_dst", dict(dst_ptrs=(dst.ptrs(0, 8), cd)), ok, None, E_ALIGN),
        ("misaligned c_src", dict(src_ptrs=(hs, src.ptrs(1, 4))), ok, None, E_ALIGN),
    ]
    for name, kw, lane, L, want in cases:
        assert state_copy(lib, g, dt, Chp, dst, src, lane, L=L, **kw) == want, name
        assert all(torch.equal(a, b) for a, b in zip(before, dst.buf)), name
    null_chp = lib.nint_state_copy(hd, cd, hs, cs, None, 2, 3, 2, (C.c_int32 * 3)(*ok), C.byref(g), dt, None)
    assert null_chp == E_ARG
    assert state_copy(lib, g, dt, Chp, dst, src, ok) == 0                        # ... and the good call still works
    assert_mapped(dst, src, ok)


def test_state_object_select_reset_clone_tensors(pkg):
    """ConvLSTMState through the lane map, against its own tensor form"""
    net = make_net(pkg, "two", "bf16")
    eng = net._engine(torch.device("cuda", torch.cuda.current_device()))
    d = data("two", 1, 21)
    # bf16-representable values: the tensor form must come back exactly
    pairs = [(h.bfloat16().float().cuda(), c.cuda()) for h, c in zip(d["h0"], d["c0"])]
    st = eng.state_from_tensors(pairs)
    for (h, c), (h2, c2) in zip(pairs, st.tensors()):
        assert torch.equal(h, h2) and torch.equal(c, c2)
    sel = st.select([1, -1, 0, 1])
    assert sel.B == 4
    for (h, c), (h2, c2) in zip(pairs, sel.tensors()):
        assert torch.equal(h2[0], h[1]) and torch.equal(h2[2], h[0]) and torch.equal(h2[3], h[1]) and not h2[1].any()
        assert torch.equal(c2[0], c[1]) and torch.equal(c2[2], c[0]) and not c2[1].any()
    cl = st.clone()
    assert cl.h[0].data_ptr() != st.h[0].data_ptr() and all(torch.equal(a, b) for a, b in zip(cl.h + cl.c, st.h + st.c))
    cl.reset([False, True])
    for (h, c), (h2, c2) in zip(pairs, cl.tensors()):
        assert torch.equal(h2[0], h[0]) and not h2[1].any() and torch.equal(c2[0], c[0]) and not c2[1].any()
    cl.reset()
    assert not any(bool(t.any()) for t in cl.h + cl.c)
    z = eng.new_state(2, 9, 17)
    assert not any(bool(t.any()) for t in z.h + z.c)
    with pytest.raises(ValueError):
        st.select([2])


# ------------------------------------------------------------------ 2. a split window = the whole window
def as_dict(pred, seq, states):
    res = {"pred": pred, "seq": seq}
    for l, (h, c) in enumerate(states):
        res[f"h.{l}"], res[f"c.{l}"] = h, c
    return res


@pytest.mark.parametrize("form", ["tensors", "device"])
@pytest.mark.parametrize("a", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["two", "one"])
def test_split_window_equals_whole_window_bit_for_bit(pkg, shape, dtype, a, form):
    """The same kernels read the same bytes: the merged-grid modes do not depend on T, a later chunk's first step is a
    step with a given h like any step t > 0 of the whole window, and h survives the f32 round trip exactly."""
    net = make_net(pkg, shape, dtype)
    X = data(shape, 4, 31)["X"].cuda()
    with torch.no_grad():
        pred, seq = net(X)
        pred_s, seq_s, states = net(X, return_state=True)
        assert torch.equal(pred, pred_s) and torch.equal(seq, seq_s)            # asking for the state changes no bit
        whole = as_dict(pred, seq, states)
        if form == "tensors":
            _, s1, st = net(X[:, :a], return_state=True)
            p2, s2, st2 = net(X[:, a:], st, return_state=True)
        else:
            _, s1, st = net(X[:, :a], return_state="device")
            assert isinstance(st, pkg.ConvLSTMState)
            p2, s2, st2 = net(X[:, a:], st, return_state="device")
            st2 = st2.tensors()
    split = as_dict(p2, torch.cat([s1, s2], dim=1), st2)
    for k in whole:
        assert torch.equal(split[k], whole[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["two", "one"])
def test_explicit_zero_state_against_none(pkg, shape, dtype):
    """The zero-state step skips the h half of K, which may change the order of the K-slice partials: bounds, not bits."""
    net = make_net(pkg, shape, dtype)
    s = SHAPES[shape]
    X = data(shape, 3, 32)["X"].cuda()
    zeros = [(torch.zeros(s["B"], ch, s["H"], s["W"], device="cuda"),) * 2 for ch in s["hidden"]]
    eng = net._engine(X.device)
    with torch.no_grad():
        ref = as_dict(*net(X, return_state=True))
        a = as_dict(*net(X, zeros, return_state=True))
        p, q, st = net(X, eng.new_state(s["B"], s["H"], s["W"]), return_state="device")
        b = as_dict(p, q, st.tensors())
    check(a, ref, dtype)
    check(b, ref, dtype)
    for k in a:
        assert torch.equal(a[k], b[k]), k                                      # the two forms of the same state: the same bytes


# ------------------------------------------------------------------ 3. against the oracle in f64
_ORACLE = {}


def oracle_stateful(T, variant, none_layer):
    """convlstm_forward(..., h0, c0) in f64 under autograd with the variant's cotangents; computed once per key"""
    key = (T, variant, none_layer)
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import convlstm_oracle as O
    d = data("two", T, 41)
    leaf = {k: v.double().requires_grad_(True) for k, v in params_of("two").items()}
    Xo = d["X"].double().requires_grad_(True)
    h0 = [t.double().requires_grad_(True) for t in d["h0"]]
    c0 = [t.double().requires_grad_(True) for t in d["c0"]]
    pred, seq = O.convlstm_forward(Xo, leaf, return_sequence=True, h0=h0, c0=c0)
    _, hs, cs = O.convlstm_forward(Xo, leaf, return_states=True, h0=h0, c0=c0)
    loss_of(variant, none_layer, d, pred, seq, list(zip(hs, cs))).backward()
    res = as_dict(pred.detach(), seq.detach(), [(h.detach(), c.detach()) for h, c in zip(hs, cs)])
    res["dX"] = Xo.grad
    for l in range(2):
        res[f"dh0.{l}"], res[f"dc0.{l}"] = h0[l].grad, c0[l].grad
    for k, v in leaf.items():
        res["grad." + k] = torch.zeros_like(v) if v.grad is None else v.grad
    _ORACLE[key] = res
    return res


def loss_of(variant, none_layer, d, pred, seq, states):
    """all: pred, seq and every state; states: the states only (no head gradient); pred: pred only (today's path plus
    dh0 / dc0); noseq: pred and the states of a module without return_sequence; `none_layer`: that layer's state unused"""
    to = lambda t: t.to(pred)
    loss = 0
    if variant in ("all", "pred", "noseq"):
        loss = loss + (pred * to(d["R"])).sum()
    if variant == "all":
        loss = loss + (seq * to(d["RS"])).sum()
    if variant in ("all", "states", "noseq"):
        for l, (h, c) in enumerate(states):
            if l != none_layer:
                loss = loss + (h * to(d["Rh"][l])).sum() + (c * to(d["Rc"][l])).sum()
    return loss


@pytest.mark.parametrize("variant,none_layer", [("all", None), ("states", None), ("pred", None), ("noseq", None), ("all", 0), ("all", 1),
                                                ("noseq", 1), ("states", 0)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stateful_forward_backward_vs_oracle(pkg, dtype, variant, none_layer):
    T = 3
    ref = oracle_stateful(T, variant, none_layer)
    d = data("two", T, 41)
    net = make_net(pkg, "two", dtype, seq=variant != "noseq")
    X = d["X"].cuda().requires_grad_(True)
    h0 = [t.cuda().requires_grad_(True) for t in d["h0"]]
    c0 = [t.cuda().requires_grad_(True) for t in d["c0"]]
    out = net(X, list(zip(h0, c0)), return_state=True)
    pred, seq, states = (out[0], None, out[1]) if variant == "noseq" else out
    loss_of(variant, none_layer, d, pred, seq, states).backward()
    res = as_dict(pred, seq, states)
    res["dX"] = X.grad
    for l in range(2):
        res[f"dh0.{l}"], res[f"dc0.{l}"] = h0[l].grad, c0[l].grad
    for k, p in net.named_parameters():
        res["grad." + k] = torch.zeros_like(p) if p.grad is None else p.grad
    keys = [k for k in ref if not (k == "seq" and seq is None)]
    check(res, ref, dtype, keys)


# ------------------------------------------------------------------ 4. chained autograd
@pytest.mark.parametrize("dtype", DTYPES)
def test_chained_calls_through_tensor_states_are_full_bptt(pkg, dtype):
    """T = 4 as 2 + 2 with ONE backward against net(x) on the whole window.  Not bit-equal: each weight gradient is the sum
    of two calls' reductions."""
    d = data("two", 4, 51)
    O = SHAPES["two"]["out"]
    R, RS = d["R"].cuda(), d["RS"].cuda()
    net = make_net(pkg, "two", dtype)
    X = d["X"].cuda().requires_grad_(True)
    pred, seq = net(X)
    ((pred * R).sum() + (seq * RS).sum()).backward()
    ref = {"pred": pred.detach(), "seq": seq.detach(), "dX": X.grad}
    ref.update({"grad." + k: p.grad.clone() for k, p in net.named_parameters()})
    net.zero_grad(set_to_none=True)
    X2 = d["X"].cuda().requires_grad_(True)
    p1, s1, st = net(X2[:, :2], return_state=True)
    p2, s2 = net(X2[:, 2:], st)
    ((p2 * R).sum() + (torch.cat([s1, s2], dim=1) * RS).sum()).backward()
    res = {"pred": p2, "seq": torch.cat([s1, s2], dim=1), "dX": X2.grad}
    res.update({"grad." + k: p.grad for k, p in net.named_parameters()})
    check(res, ref, dtype)
    assert torch.equal(res["pred"], ref["pred"]) and torch.equal(res["seq"], ref["seq"])     # (the forward pass is: test 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_state_truncates_bptt(pkg, dtype):
    """Through return_state="device" the first chunk gets no gradient from the second: its dX is that of the first chunk
    trained alone, bit for bit."""
    d = data("two", 4, 52)
    O = SHAPES["two"]["out"]
    R, RS = d["R"].cuda(), d["RS"].cuda()
    net = make_net(pkg, "two", dtype)
    Xa = d["X"][:, :2].cuda().requires_grad_(True)
    Xb = d["X"][:, 2:].cuda().requires_grad_(True)
    _, s1, st = net(Xa, return_state="device")
    p2, s2 = net(Xb, st)
    ((s1 * RS[:, :2 * O]).sum() + (p2 * R).sum() + (s2 * RS[:, 2 * O:]).sum()).backward()
    assert Xb.grad is not None and bool(Xb.grad.abs().sum() > 0)
    Xc = d["X"][:, :2].cuda().requires_grad_(True)
    _, s1c = net(Xc)
    (s1c * RS[:, :2 * O]).sum().backward()
    assert torch.equal(Xa.grad, Xc.grad)


# ------------------------------------------------------------------ 5. contract edges
def test_mismatched_states_are_refused(pkg):
    s = SHAPES["two"]
    net = make_net(pkg, "two", "f32")
    d = data("two", 2, 61)
    X = d["X"].cuda()
    eng = net._engine(X.device)
    B, H, W = s["B"], s["H"], s["W"]
    good = [(h.cuda(), c.cuda()) for h, c in zip(d["h0"], d["c0"])]
    with torch.no_grad():
        net(X, good)
        with pytest.raises(ValueError, match="B = 3"):
            net(X, eng.new_state(3, H, W))
        with pytest.raises(ValueError, match="grid"):
            net(X, eng.new_state(B, H + 1, W))
        other = make_net(pkg, "two", "bf16")
        with pytest.raises(ValueError, match="dtype"):
            net(X, other._engine(X.device).new_state(B, H, W))
        one = pkg.ConvLSTM(5, [16], [3], 1, compute_dtype="f32").cuda()
        with pytest.raises(ValueError, match="layers"):
            net(X, one._engine(X.device).new_state(B, H, W))
        with pytest.raises(ValueError, match="1 .* pairs"):
            net(X, good[:1])
        with pytest.raises(ValueError, match="shape"):
            net(X, [(h[:1], c[:1]) for h, c in good])
        with pytest.raises(ValueError, match="shape"):
            net(X, [(h[..., :-1], c[..., :-1]) for h, c in good])
        with pytest.raises(ValueError, match="shape"):
            net(X, [good[1], good[0]])
        with pytest.raises(ValueError, match="return_state"):
            net(X, good, return_state="host")


def test_double_backward_through_a_state_gradient_is_refused(pkg):
    d = data("two", 2, 62)
    net = make_net(pkg, "two", "f32")
    X = d["X"].cuda()
    h0 = [t.cuda().requires_grad_(True) for t in d["h0"]]
    c0 = [t.cuda().requires_grad_(True) for t in d["c0"]]
    pred, seq, states = net(X, list(zip(h0, c0)), return_state=True)
    (g,) = torch.autograd.grad(pred.sum() + states[0][1].sum(), h0[0], create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        g.sum().backward()


def test_retained_graph_reused_after_another_forward_is_refused(pkg):
    d = data("two", 2, 63)
    net = make_net(pkg, "two", "f32")
    X = d["X"].cuda().requires_grad_(True)
    st = [(h.cuda(), c.cuda()) for h, c in zip(d["h0"], d["c0"])]
    pred, seq, states = net(X, st, return_state=True)
    loss = pred.sum() + states[1][0].sum()
    loss.backward(retain_graph=True)
    out2 = net(X, st, return_state=True)            # the same shape: takes the workspace the first backward released
    with pytest.raises(RuntimeError, match="retained"):
        loss.backward()
    del out2


def test_default_call_after_stateful_calls_is_unchanged(pkg):
    d = data("two", 3, 64)
    X = d["X"].cuda()
    net = make_net(pkg, "two", "bf16")
    st = [(h.cuda(), c.cuda()) for h, c in zip(d["h0"], d["c0"])]
    with torch.no_grad():
        _, _, dev = net(X, st, return_state="device")
        net(X, dev, return_state=True)
    Xg = d["X"].cuda().requires_grad_(True)
    out = net(Xg, st, return_state=True)
    (out[0].sum() + out[2][0][0].sum()).backward()
    fresh = make_net(pkg, "two", "bf16")
    with torch.no_grad():
        a, b = net(X), fresh(X)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and its gradients: the default training path after the stateful one
    net.zero_grad(set_to_none=True)
    R = d["R"].cuda()
    Xa, Xb = d["X"].cuda().requires_grad_(True), d["X"].cuda().requires_grad_(True)
    (net(Xa)[0] * R).sum().backward()
    (fresh(Xb)[0] * R).sum().backward()
    assert torch.equal(Xa.grad, Xb.grad)
    for (k, p), (_, q) in zip(net.named_parameters(), fresh.named_parameters()):
        assert torch.equal(p.grad, q.grad), k


# ------------------------------------------------------------------ 6. FusedTrainer(stateful=True)
TRAIN = dict(C=5, hidden=[16, 8], ks=[3, 3], out=1, B=2, T=2, grid=(8, 12), pad=(12, 16), halo=(2, 2))


def oracle_stateful_steps(params, Xs, ys, resets, lr, betas, seq_loss):
    """three steps of truncated BPTT composed from the oracle: convlstm_forward from the detached carried (h0, c0), crop,
    loss_mse_l1, autograd, adam_step_numpy"""
    from oracle import convlstm_oracle as O
    t = TRAIN
    hs = cs = None
    m = {k: np.zeros_like(v.numpy()) for k, v in params.items()}
    v2 = {k: np.zeros_like(v.numpy()) for k, v in params.items()}
    p = {k: v.clone() for k, v in params.items()}
    losses = []
    for step, (X, y, reset) in enumerate(zip(Xs, ys, resets), 1):
        if hs is not None and reset is not None:
            keep = torch.tensor([0.0 if r else 1.0 for r in reset]).view(-1, 1, 1, 1)
            hs, cs = [h * keep for h in hs], [c * keep for c in cs]
        leaf = {k: w.detach().clone().requires_grad_(True) for k, w in p.items()}
        if seq_loss:
            _, seq = O.convlstm_forward(X, leaf, return_sequence=True, h0=hs, c0=cs)
            pred = O.crop_pred(seq, t["halo"], t["grid"])                     # (B, T*O, Hc, Wc) against y (B, T, Hc, Wc)
        else:
            pred = O.crop_pred(O.convlstm_forward(X, leaf, h0=hs, c0=cs), t["halo"], t["grid"])[:, 0]
        loss = O.loss_mse_l1(y, pred)
        loss.backward()
        with torch.no_grad():
            _, nh, nc = O.convlstm_forward(X, leaf, return_states=True, h0=hs, c0=cs)
        hs, cs = [h.detach() for h in nh], [c.detach() for c in nc]
        losses.append(float(loss.detach()))
        for k in p:
            a, m[k], v2[k] = O.adam_step_numpy(p[k].numpy(), leaf[k].grad.numpy(), m[k], v2[k], step, lr, betas)
            p[k] = torch.from_numpy(a)
    return p, losses


@pytest.mark.parametrize("seq_loss", [False, True])
def test_stateful_trainer_matches_oracle_truncated_bptt(pkg, seq_loss):
    """Parameters after 3 steps within the tolerance of tests/test_gpu_train.py's parameters-after-3-steps golden (same
    lr = 1e-4: max |dW| <= 6.5e-4, mean <= 2e-6); lane 1 is reset before the second step."""
    from nasa_niswan_amd.trainer import FusedTrainer
    from oracle import convlstm_oracle as O
    t = TRAIN
    lr, betas = 1e-4, (0.5, 0.999)
    params = O.synth_params(t["C"], t["hidden"], t["ks"], 2, out_channels=t["out"], seed=71)
    rng = np.random.default_rng(72)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    Xs = [f(t["B"], t["T"], t["C"], *t["pad"]) for _ in range(3)]
    ys = [f(t["B"], t["T"], *t["grid"]) if seq_loss else f(t["B"], *t["grid"]) for _ in range(3)]
    resets = [None, [False, True], None]
    want, want_losses = oracle_stateful_steps(params, Xs, ys, resets, lr, betas, seq_loss)
    net = pkg.ConvLSTM(t["C"], t["hidden"], t["ks"], 2, out_channels=t["out"]).cuda()
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=lr, betas=betas, halo=t["halo"], sequence_loss=seq_loss, stateful=True)
    for X, y, reset, wl in zip(Xs, ys, resets, want_losses):
        loss = float(tr.step(X.cuda(), y.cuda(), reset=reset))
        print(f"  loss {loss:.7f} oracle {wl:.7f}")
        # both sides are f32: gate sums of K = 189 terms carry ~sqrt(K) eps = 2e-6 relative, through 2 layers and up to 6 carried
        # steps, averaged down by the loss's mean over 192 cells -- 1e-5 relative bounds it with room
        assert abs(loss - wl) < 1e-5 * abs(wl)
    for k, v in net.state_dict().items():
        dlt = (v.cpu() - want[k]).abs()
        print(f"  {k}: max |dW| {float(dlt.max()):.2e}, mean {float(dlt.mean()):.2e}")
        assert float(dlt.max()) <= 6.5e-4 and float(dlt.mean()) <= 2e-6
    # the carried state is the oracle's after step 3 (forward with the weights BEFORE the third update)
    assert tr.state is not None and tr.state.B == t["B"]
    tr.reset_state()
    assert tr.state is None


def test_stateless_trainer_is_unchanged(pkg):
    """stateful=False on the same data: today's trainer bit for bit; reset= is refused there"""
    from nasa_niswan_amd.trainer import FusedTrainer
    from oracle import convlstm_oracle as O
    t = TRAIN
    params = O.synth_params(t["C"], t["hidden"], t["ks"], 2, out_channels=t["out"], seed=73)
    rng = np.random.default_rng(74)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32)).cuda()
    Xs, ys = [f(t["B"], t["T"], t["C"], *t["pad"]) for _ in range(3)], [f(t["B"], *t["grid"]) for _ in range(3)]
    nets = []
    for kw in ({}, dict(stateful=False)):
        net = pkg.ConvLSTM(t["C"], t["hidden"], t["ks"], 2, out_channels=t["out"]).cuda()
        net.load_state_dict(params)
        tr = FusedTrainer(net, lr=1e-3, halo=t["halo"], **kw)
        losses = [tr.step(X, y).clone() for X, y in zip(Xs, ys)]
        nets.append((net, losses, tr))
    for a, b in zip(nets[0][1], nets[1][1]):
        assert torch.equal(a, b)
    for (k, p), (_, q) in zip(nets[0][0].state_dict().items(), nets[1][0].state_dict().items()):
        assert torch.equal(p, q), k
    assert nets[1][2].state is None
    with pytest.raises(ValueError, match="stateful"):
        nets[1][2].step(Xs[0], ys[0], reset=True)
    # a stateful trainer differs from the second step on (the first starts from zeros either way)
    net = pkg.ConvLSTM(t["C"], t["hidden"], t["ks"], 2, out_channels=t["out"]).cuda()
    net.load_state_dict(params)
    tr = FusedTrainer(net, lr=1e-3, halo=t["halo"], stateful=True)
    l1, l2 = float(tr.step(Xs[0], ys[0])), float(tr.step(Xs[1], ys[1]))
    assert abs(l1 - float(nets[0][1][0])) <= 1e-5 * abs(l1) and l2 != float(nets[0][1][1])


# ------------------------------------------------------------------ 7. predict_stream
def stream_dataset():
    """a 'test' period of 11 windows of 4 steps = 14 record steps (70-step record: steps 56..69)"""
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    ds = SyntheticE33OMA_CRNN("test", padding=(12, 16), in_channels=5, sequence_length=4, n_steps=70, grid=(8, 12), device="cuda")
    assert len(ds) == 11 and int(ds.first[0]) == 56
    return ds


def test_predict_stream_equals_the_hand_written_loop(pkg):
    from nasa_niswan_amd.inference import SkillAccumulator, predict_stream, skill_from_sums
    ds = stream_dataset()
    net = pkg.ConvLSTM(5, [16, 8], [3, 3], 2, out_channels=1, return_sequence=True, compute_dtype="bf16").cuda()
    halo, (Hc, Wc), T = (2, 2), ds.grid, 4
    acc = SkillAccumulator(1, Hc, Wc, device="cuda")
    pred, steps, dropped = predict_stream(net, ds, lanes=1, halo=halo, skill=acc)
    assert dropped == 2 and pred.shape == (12, 1, Hc, Wc) and pred.dtype == torch.float32 and pred.is_cuda
    assert steps.tolist() == list(range(56, 68))
    want, state = [], None
    with torch.no_grad():
        for k in range(3):
            X, _ = ds.slab_batch([k * T])
            _, seq, state = net(X, state, return_state="device")
            want.append(seq.view(T, 1, 12, 16)[:, :, 2:2 + Hc, 2:2 + Wc])
    assert torch.equal(pred, torch.cat(want))
    # the carried state matters: chunk 1 from the zero state is another prediction
    with torch.no_grad():
        cold = net(ds.slab_batch([T])[0])[1].view(T, 1, 12, 16)[:, :, 2:2 + Hc, 2:2 + Wc]
    assert not torch.equal(cold, pred[T:2 * T])
    # skill: the same sums as update_from_pred on the returned tensor against the tracer at those steps (z-score units),
    # chunk by chunk as predict_stream folds them: the same launches on the same values
    y = torch.from_numpy((ds.yraw[56:68] - ds.y_mean) / ds.y_std).cuda()
    acc2 = SkillAccumulator(1, Hc, Wc, device="cuda")
    for k in range(3):
        acc2.update_from_pred(pred[k * T:(k + 1) * T], y[k * T:(k + 1) * T], (0, 0))
    rep, rep2 = acc.report(), skill_from_sums(*acc2.sums())
    assert rep.count == 12
    for name, a in rep.arrays().items():
        # f64 sums of the same f32 terms; the crop offset may change how a launch splits its rows, i.e. the order of the f64
        # additions: a few ulp of f64 on the sums, far below 1e-9 on every statistic of a 12-sample, O(1)-valued series
        np.testing.assert_allclose(a, rep2.arrays()[name], rtol=1e-9, atol=1e-9, err_msg=name)


def test_predict_stream_lanes(pkg):
    """lanes = 3: three contiguous segments as one batch, each from the zero state = three lanes = 1 runs of one chunk"""
    from nasa_niswan_amd.inference import predict_stream
    ds = stream_dataset()
    net = pkg.ConvLSTM(5, [16, 8], [3, 3], 2, out_channels=1, compute_dtype="f32").cuda()
    pred, steps, dropped = predict_stream(net, ds, lanes=3, halo=(2, 2))
    assert dropped == 2 and steps.tolist() == list(range(56, 68)) and pred.shape[0] == 12
    with pytest.raises(ValueError, match="lanes"):
        predict_stream(net, ds, lanes=4, halo=(2, 2))


# ------------------------------------------------------------------ train.py --stateful
@pytest.mark.parametrize("seq_loss", [False, True])
def test_train_py_stateful(pkg, tmp_path, monkeypatch, seq_loss):
    """two epochs over the schedule (no shuffle, state reset per epoch); the first step starts from zeros, so its loss is the
    stateless loop's on the same batch; with and without --sequence-loss"""
    from nasa_niswan_amd import train as T
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN, stateful_schedule
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--model", "LSTM-st", "--in-channels", "5", "--hidden-channels", "16", "8", "--kernel-size", "3", "3", "--num-layers", "2",
            "--sequence-length", "4", "--input-size", "12", "16", "--grid", "8", "12", "--batch-size", "2", "--num-epochs", "2",
            "--learning-rate", "1e-3", "--synthetic-steps", "60", "--dtype", "f32", "--snapshot-dir", str(tmp_path / "s"),
            "--stateful"] + (["--sequence-loss"] if seq_loss else [])
    logger = T.main(T.get_arguments(argv))
    assert len(logger["MSELoss"]) == 2 and np.isfinite(logger["MSELoss"]).all() and np.isfinite(logger["r2_score_val"]).all()
    assert logger["MSELoss"][1] < logger["MSELoss"][0]                      # the same batches in the same order: it learns
    ds = SyntheticE33OMA_CRNN("train", padding=(12, 16), in_channels=5, sequence_length=4, n_steps=60, grid=(8, 12), device="cuda",
                              sequence_targets=seq_loss)
    sched, dropped = stateful_schedule(len(ds), 4, 2)
    assert len(ds) == 42 and sched.shape == (5, 2) and dropped == 5         # 45 record steps: two lanes of 5 chunks of 4, 5 steps left
