"""The autograd contract of ConvLSTM / ConvLSTMCell on the device: whatever autograd allows on
the reference's nn.Modules gives the right gradient here or is refused loudly.  The kernels are audited launch by launch
elsewhere; this file is about the Python glue that decides which memory they read: the autograd Functions of model.py
(one for ConvLSTM, with or without state, one for the cell), the engine's workspace pool and the releaser -- on the
paths a training script takes and the one-forward / one-dense-backward tests do not: user-written recurrences over the
cell, several live graphs, work between forward and backward, retained graphs, in-place weight updates, double backward,
strided / expanded / f64 / bf16 inputs and cotangents, frozen parameters, dropped graphs, a side stream, a deepcopy twin.

Numbers are compared with the CPU oracle run in f64 under the bounds of tests/test_gpu_shapes.py::check; two routes that
must launch the same kernels on the same bytes are compared bit for bit (torch.equal), one of each pair also against the
oracle."""
import copy
import gc
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = ["f32", "bf16"]
SHAPES = {
    # two layers: the merged-grid modes are live.  Its 5-channel input under k = 3 is horizontally FOLDED too (15 folded channels
    # are one MFMA K-step against three): the engine's rule, asserted in test_input_forms
    "plain": dict(C=5, hidden=[16, 8], ks=[3, 3], out=2, B=2, T=3, H=9, W=17),
    # a thin input under k = 5: folded, dx through nint_unfold_dx
    "fold": dict(C=3, hidden=[8], ks=[5], out=1, B=2, T=2, H=8, W=20),
}
# ... so the channel-padded input layout and its dx path (nint_unpack_compact) get S-plain once more, built with engine.XFOLD off
SHAPES["plain-unfolded"] = SHAPES["plain"]
FOLDED = {"plain": True, "fold": True, "plain-unfolded": False}
CELL = dict(Cin=5, Ch=16, k=3, B=2, H=9, W=17)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as p
    p.load_library()
    return p


# ------------------------------------------------------------------ data, oracle, comparisons
def params_of(shape, seed=0):
    from oracle import convlstm_oracle as O
    s = SHAPES[shape]
    return O.synth_params(s["C"], s["hidden"], s["ks"], len(s["hidden"]), out_channels=s["out"], seed=seed)


def batch(shape, seed, B=None):
    """X (B,T,C,H,W), a cotangent for pred (B,out,H,W) and one for seq (B,T*out,H,W): CPU f32, seeded"""
    s = SHAPES[shape]
    B = s["B"] if B is None else B
    rng = np.random.default_rng(seed)
    X = torch.from_numpy(rng.standard_normal((B, s["T"], s["C"], s["H"], s["W"])).astype(np.float32))
    R = torch.from_numpy(rng.standard_normal((B, s["out"], s["H"], s["W"])).astype(np.float32))
    RS = torch.from_numpy(rng.standard_normal((B, s["T"] * s["out"], s["H"], s["W"])).astype(np.float32))
    return X, R, RS


def dense(R):
    return lambda pred: (pred * R.to(pred)).sum()


def dense_seq(R, RS):
    return lambda pred, seq: (pred * R.to(pred)).sum() + (seq * RS.to(seq)).sum()


_ORACLE = {}


def oracle(key, shape, X, loss, seq=False, params=None):
    """convlstm_forward in f64 on the CPU and loss(pred[, seq]).backward(): computed once per `key`, never modified."""
    if key not in _ORACLE:
        from oracle import convlstm_oracle as O
        leaf = {k: v.double().requires_grad_(True) for k, v in (params or params_of(shape)).items()}
        Xo = X.double().requires_grad_(True)
        out = O.convlstm_forward(Xo, leaf, return_sequence=seq)
        out = out if seq else (out,)
        loss(*out).backward()
        res = {"pred": out[0].detach(), "dX": Xo.grad}
        if seq:
            res["seq"] = out[1].detach()
        for k, v in leaf.items():
            res["grad." + k] = v.grad
        _ORACLE[key] = res
    return _ORACLE[key]


def check(res, ref, dtype, keys=None):
    """tests/test_gpu_shapes.py::check: f32 max abs error <= 1e-3 max|ref| + 1e-5, bf16 relative L2 <= 2e-2"""
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


def same(a, b, keys=None):
    """bit equality of two result dicts (None = no gradient, on both sides)"""
    for k in (keys or b):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def make_net(pkg, shape, dtype, seq=False, params=None):
    from nasa_niswan_amd import engine
    s = SHAPES[shape]
    net = pkg.ConvLSTM(s["C"], s["hidden"], s["ks"], len(s["hidden"]), out_channels=s["out"], return_sequence=seq,
                       compute_dtype=dtype).cuda()
    net.load_state_dict(params or params_of(shape))
    old = engine.XFOLD
    engine.XFOLD = FOLDED[shape]
    try:                                # the engine is built on first use: here, under this shape's input layout
        eng = net._engine(torch.device("cuda", torch.cuda.current_device()))
    finally:
        engine.XFOLD = old
    assert eng.cfgs[0].xfold == FOLDED[shape], "the shape no longer runs the input layout it is here for"
    return net


def zero(mod):
    for p in mod.parameters():
        p.grad = None


def grads_of(mod):
    return {"grad." + k: (None if p.grad is None else p.grad.detach().clone()) for k, p in mod.named_parameters()}


def run(net, x, loss, between=None):
    """One forward and one backward of `net` on the device tensor `x` (a leaf or a view of one: the caller reads its
    gradient); `between` runs after the forward and before the backward.  -> outputs and parameter gradients."""
    zero(net)
    out = net(x)
    out = out if isinstance(out, tuple) else (out,)
    kept = between() if between is not None else None
    loss(*out).backward()
    del kept
    res = {"pred": out[0].detach()}
    if len(out) > 1:
        res["seq"] = out[1].detach()
    res.update(grads_of(net))
    return res


def run_std(net, X, loss, between=None):
    """... on a contiguous f32 leaf made from the CPU tensor X: the twin every other route is compared with"""
    Xd = X.to(DEV).requires_grad_(True)
    res = run(net, Xd, loss, between)
    res["dX"] = Xd.grad
    return res


def spaces(mod, train=None):
    """the workspaces of a module's (one) engine"""
    (eng,) = mod._engines.values()
    return [ws for pool in eng.pool.values() for ws in pool if train is None or ws.train == train]


# ------------------------------------------------------------------ the cell
def cell_params(bias=True):
    from oracle import convlstm_oracle as O
    p = O.synth_params(CELL["Cin"], [CELL["Ch"]], [CELL["k"]], 1, seed=2)
    sd = {"conv.weight": p["layers.0.conv.weight"]}
    if bias:
        sd["conv.bias"] = p["layers.0.conv.bias"]
    return sd


def cell_data(seed, zero_state=False):
    """x, h, c and the cotangents of h', c': CPU f32, seeded"""
    B, Cin, Ch, H, W = (CELL[k] for k in ("B", "Cin", "Ch", "H", "W"))
    rng = np.random.default_rng(seed)
    x, h, c, Dh, Dc = (torch.from_numpy(rng.standard_normal((B, n, H, W)).astype(np.float32)) for n in (Cin, Ch, Ch, Ch, Ch))
    if zero_state:
        h, c = torch.zeros_like(h), torch.zeros_like(c)
    return x, 0.5 * h, c, Dh, Dc


def make_cell(pkg, dtype, bias=True):
    cell = pkg.ConvLSTMCell(CELL["Cin"], CELL["Ch"], CELL["k"], bias=bias, compute_dtype=dtype).cuda()
    cell.load_state_dict(cell_params(bias))
    return cell


def cell_loss(Dh, Dc):
    return lambda h1, c1: (h1 * Dh.to(h1)).sum() + (c1 * Dc.to(c1)).sum()


def oracle_cell(key, x, h, c, loss):
    if key not in _ORACLE:
        from oracle import convlstm_oracle as O
        sd = {k: v.double().requires_grad_(True) for k, v in cell_params().items()}
        xo, ho, co = (t.double().requires_grad_(True) for t in (x, h, c))
        h1, c1 = O.cell_forward(xo, ho, co, sd["conv.weight"], sd["conv.bias"])
        loss(h1, c1).backward()
        _ORACLE[key] = {"h1": h1.detach(), "c1": c1.detach(), "dx": xo.grad, "dh": ho.grad, "dc": co.grad,
                        "grad.conv.weight": sd["conv.weight"].grad, "grad.conv.bias": sd["conv.bias"].grad}
    return _ORACLE[key]


def run_cell(cell, x, h, c, loss):
    """x, h, c: device tensors (leaves or views of leaves); -> outputs and parameter gradients"""
    zero(cell)
    h1, c1 = cell(x, (h, c))
    loss(h1, c1).backward()
    res = {"h1": h1.detach(), "c1": c1.detach()}
    res.update(grads_of(cell))
    return res


def run_cell_std(cell, x, h, c, loss):
    xd, hd, cd = (t.to(DEV).requires_grad_(True) for t in (x, h, c))
    res = run_cell(cell, xd, hd, cd, loss)
    res.update(dx=xd.grad, dh=hd.grad, dc=cd.grad)
    return res


# ------------------------------------------------------------------ one subject for the lifetime / refusal cases
def subject(pkg, kind, dtype):
    """kind "pred" / "seq": ConvLSTM on S-plain without / with return_sequence; "cell": ConvLSTMCell.
    -> (module, graph, ref): graph(seed) records one forward and returns (loss, leaves, outputs), ref(seed) is the f64
    oracle of that graph under the keys collect() uses."""
    if kind == "cell":
        mod = make_cell(pkg, dtype)

        def graph(seed):
            x, h, c, Dh, Dc = cell_data(seed)
            leaves = {"x": x.to(DEV).requires_grad_(True), "h": h.to(DEV).requires_grad_(True), "c": c.to(DEV).requires_grad_(True)}
            h1, c1 = mod(leaves["x"], (leaves["h"], leaves["c"]))
            return cell_loss(Dh, Dc)(h1, c1), leaves, {"h1": h1.detach(), "c1": c1.detach()}

        def ref(seed):
            x, h, c, Dh, Dc = cell_data(seed)
            return oracle_cell(("cell", seed), x, h, c, cell_loss(Dh, Dc))
    else:
        seq = kind == "seq"
        mod = make_net(pkg, "plain", dtype, seq=seq)

        def graph(seed):
            X, R, RS = batch("plain", seed)
            leaves = {"X": X.to(DEV).requires_grad_(True)}
            out = mod(leaves["X"])
            if seq:
                return dense_seq(R, RS)(*out), leaves, {"pred": out[0].detach(), "seq": out[1].detach()}
            return dense(R)(out), leaves, {"pred": out.detach()}

        def ref(seed):
            X, R, RS = batch("plain", seed)
            return oracle(("plain", kind, seed), "plain", X, dense_seq(R, RS) if seq else dense(R), seq=seq)
    return mod, graph, ref


def collect(mod, leaves, outs):
    res = dict(outs)
    res.update({"d" + k: (None if v.grad is None else v.grad.detach().clone()) for k, v in leaves.items()})
    res.update(grads_of(mod))
    return res


def single(mod, graph, seed):
    """forward + backward with nothing in between"""
    zero(mod)
    loss, leaves, outs = graph(seed)
    loss.backward()
    return collect(mod, leaves, outs)


def drop_grads(mod, leaves):
    zero(mod)
    for v in leaves.values():
        v.grad = None


# ================================================================== 1. a recurrence written over ConvLSTMCell
@pytest.mark.parametrize("dtype", DTYPES)
def test_cell_recurrence_as_the_reference_builds_it(pkg, dtype):
    """reference model.py:253-271 spelled out by the user: T steps over two ConvLSTMCells from zero states, the 1x1 head as
    an einsum -- against convlstm_forward in f64; next to them a bias-free cell recurring over the same inputs, against
    cell_forward(..., bias=None).  Every step of every cell holds its own workspace while the graph lives; a second
    iteration creates none."""
    from oracle import convlstm_oracle as O
    s = SHAPES["plain"]
    B, T, H, W = s["B"], s["T"], s["H"], s["W"]
    params = params_of("plain")
    X, R, _ = batch("plain", 11)
    rng = np.random.default_rng(21)
    R3 = torch.from_numpy(rng.standard_normal((B, 8, H, W)).astype(np.float32))
    w3 = O.synth_params(s["C"], [8], [3], 1, seed=4)["layers.0.conv.weight"]
    cells = [pkg.ConvLSTMCell(5, 16, 3, compute_dtype=dtype).cuda(), pkg.ConvLSTMCell(16, 8, 3, compute_dtype=dtype).cuda()]
    for i, cell in enumerate(cells):
        cell.load_state_dict({"conv.weight": params[f"layers.{i}.conv.weight"], "conv.bias": params[f"layers.{i}.conv.bias"]})
    nb = pkg.ConvLSTMCell(5, 8, 3, bias=False, compute_dtype=dtype).cuda()
    assert nb.conv.bias is None and [k for k, _ in nb.named_parameters()] == ["conv.weight"]
    nb.load_state_dict({"conv.weight": w3})
    w = params["conv.weight"][:, :, 0, 0].to(DEV).requires_grad_(True)
    b = params["conv.bias"].to(DEV).requires_grad_(True)
    key = (B, 1, H, W, True, True)

    for it in range(2):
        for m in cells + [nb]:
            zero(m)
        w.grad = b.grad = None
        Xd = X.to(DEV).requires_grad_(True)
        hs = [torch.zeros(B, ch, H, W, device=DEV) for ch in (16, 8)]
        cs = [torch.zeros(B, ch, H, W, device=DEV) for ch in (16, 8)]
        h3, c3 = torch.zeros(B, 8, H, W, device=DEV), torch.zeros(B, 8, H, W, device=DEV)
        for t in range(T):
            xt = Xd[:, t]
            for i, cell in enumerate(cells):
                hs[i], cs[i] = cell(xt, (hs[i], cs[i]))
                xt = hs[i]
            h3, c3 = nb(Xd[:, t], (h3, c3))
        pred = torch.einsum("oc,bchw->bohw", w, hs[-1]) + b[None, :, None, None]
        for m in cells + [nb]:
            (eng,) = m._engines.values()
            assert list(eng.pool) == [key] and len(eng.pool[key]) == T and all(ws.in_use for ws in eng.pool[key]), it
        loss = (pred * R.to(DEV)).sum() + (h3 * R3.to(DEV)).sum()
        loss.backward()
        got = {"pred": pred.detach(), "h3": h3.detach(), "dX": Xd.grad, "grad.conv.weight": w.grad[:, :, None, None],
               "grad.conv.bias": b.grad, "grad.nb": nb.conv.weight.grad}
        for i, cell in enumerate(cells):
            got[f"grad.layers.{i}.conv.weight"], got[f"grad.layers.{i}.conv.bias"] = cell.conv.weight.grad, cell.conv.bias.grad
        del pred, loss, hs, cs, h3, c3, xt
        for m in cells + [nb]:
            assert len(spaces(m)) == T and not any(ws.in_use for ws in spaces(m)), it

        if it == 0:
            leaf = {k: v.double().requires_grad_(True) for k, v in params.items()}
            w3o = w3.double().requires_grad_(True)
            Xo = X.double().requires_grad_(True)
            po = O.convlstm_forward(Xo, leaf)
            h3o = c3o = torch.zeros(B, 8, H, W, dtype=torch.float64)
            for t in range(T):
                h3o, c3o = O.cell_forward(Xo[:, t], h3o, c3o, w3o, None)
            ((po * R.double()).sum() + (h3o * R3.double()).sum()).backward()
            ref = {"pred": po.detach(), "h3": h3o.detach(), "dX": Xo.grad, "grad.nb": w3o.grad}
            ref.update({"grad." + k: v.grad for k, v in leaf.items()})
            first = got
        else:
            same(got, first)            # ... and the reused workspaces give the same bits
        check(got, ref, dtype)


# ================================================================== 2. two live graphs on one module
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_live_graphs_on_one_module(pkg, dtype):
    net = make_net(pkg, "plain", dtype)
    (X1, R1, _), (X2, R2, _) = batch("plain", 11), batch("plain", 12)
    alone1, alone2 = run_std(net, X1, dense(R1)), run_std(net, X2, dense(R2))
    o1, o2 = oracle(("plain", "pred", 11), "plain", X1, dense(R1)), oracle(("plain", "pred", 12), "plain", X2, dense(R2))
    check(alone1, o1, dtype)
    check(alone2, o2, dtype)
    # the joint loss is the sum of the two: so is its f64 gradient
    joint_ref = {k: o1[k] + o2[k] for k in o1 if k.startswith("grad.")}

    for separate in (False, True):
        zero(net)
        A, Bx = X1.to(DEV).requires_grad_(True), X2.to(DEV).requires_grad_(True)
        p1, p2 = net(A), net(Bx)
        assert len(spaces(net, train=True)) == 2 and all(ws.in_use for ws in spaces(net))
        if separate:                    # one backward() each, the younger graph first
            (p2 * R2.to(DEV)).sum().backward()
            (p1 * R1.to(DEV)).sum().backward()
        else:
            ((p1 * R1.to(DEV)).sum() + (p2 * R2.to(DEV)).sum()).backward()
        assert torch.equal(p1, alone1["pred"]) and torch.equal(p2, alone2["pred"])
        assert torch.equal(A.grad, alone1["dX"]) and torch.equal(Bx.grad, alone2["dX"]), separate
        check(grads_of(net), joint_ref, dtype)
        del p1, p2
        assert len(spaces(net)) == 2 and all(ws.train and not ws.in_use for ws in spaces(net)), separate


# ================================================================== 3. work between forward and backward
@pytest.mark.parametrize("dtype", DTYPES)
def test_work_between_forward_and_backward_changes_no_bit(pkg, dtype):
    """A forward in between repacks Wf / Wd, may reuse the engine-wide split-K scratch and asks the pool for a workspace:
    the first graph's gradients must not notice."""
    net = make_net(pkg, "plain", dtype)
    (X1, R1, _), (X2, _, _) = batch("plain", 11), batch("plain", 12)
    base = run_std(net, X1, dense(R1))
    check(base, oracle(("plain", "pred", 11), "plain", X1, dense(R1)), dtype)

    def no_grad_forward():
        with torch.no_grad():
            net(X2.to(DEV))

    def other_batch_size():
        net(X2[:1].to(DEV).requires_grad_(True))            # its graph dies at once

    def live_graph():
        return net(X2.to(DEV).requires_grad_(True))          # kept alive until after the backward

    for between in (no_grad_forward, other_batch_size, live_graph):
        same(run_std(net, X1, dense(R1), between), base)
    assert not any(ws.in_use for ws in spaces(net))


# ================================================================== 4. retained graphs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["pred", "seq", "cell"])
def test_retained_graph_backward_twice_doubles_every_gradient(pkg, kind, dtype):
    mod, graph, ref = subject(pkg, kind, dtype)
    one = single(mod, graph, 11)
    check(one, ref(11), dtype)
    zero(mod)
    loss, leaves, outs = graph(11)
    loss.backward(retain_graph=True)
    loss.backward()
    two = collect(mod, leaves, outs)
    for k, v in one.items():
        assert torch.equal(two[k], 2 * v if k.startswith(("d", "grad.")) else v), k


@pytest.mark.parametrize("kind", ["pred", "seq", "cell"])
def test_retained_graph_across_another_forward_is_refused_or_right(pkg, kind):
    """backward(retain_graph=True), a same-shape forward of other data, backward again: the first backward returned the
    workspace, the forward took it.  Two outcomes are allowed: a RuntimeError that names the retained graph / workspace, or
    the same gradient bit for bit -- never BPTT over the other batch's activations."""
    mod, graph, ref = subject(pkg, kind, "f32")
    one = single(mod, graph, 11)
    check(one, ref(11), "f32")
    zero(mod)
    loss, leaves, outs = graph(11)
    loss.backward(retain_graph=True)
    same(collect(mod, leaves, outs), one)
    other = graph(12)                                   # kept alive
    drop_grads(mod, leaves)
    try:
        loss.backward()
    except RuntimeError as e:
        print(f"  refused: {e}")
        assert re.search(r"retain", str(e)) and re.search(r"workspace", str(e)), str(e)
    else:
        same(collect(mod, leaves, outs), one)
    del other, loss
    same(single(mod, graph, 11), one)                   # the module goes on working either way
    gc.collect()
    assert not any(ws.in_use for ws in spaces(mod))


# ================================================================== 5. weights changed before backward
@pytest.mark.parametrize("again", [False, True], ids=["plain", "then-another-forward"])
@pytest.mark.parametrize("kind,name", [("pred", "layers.0.conv.weight"), ("pred", "layers.1.conv.weight"), ("pred", "conv.weight"),
                                       ("seq", "layers.0.conv.weight"), ("seq", "conv.weight"), ("cell", "conv.weight")])
def test_weight_changed_in_place_before_backward_is_refused(pkg, kind, name, again):
    """The dgrad reads the engine's packed image of the weights, which every forward rewrites; the head's backward reads the
    head weight itself.  Both are saved tensors: torch's version check refuses the backward, before any launch -- and the
    graph that never ran its backward still returns its workspace when it dies."""
    mod, graph, _ = subject(pkg, kind, "f32")
    loss, leaves, outs = graph(11)
    with torch.no_grad():
        dict(mod.named_parameters())[name].add_(0.1)
    other = graph(12) if again else None
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    assert all(p.grad is None for p in mod.parameters()) and all(v.grad is None for v in leaves.values())
    assert sum(ws.in_use for ws in spaces(mod)) == (2 if again else 1)
    del loss, leaves, outs, other
    gc.collect()
    assert not any(ws.in_use for ws in spaces(mod))


@pytest.mark.parametrize("kind", ["pred", "seq", "cell"])
def test_bias_changed_in_place_before_backward_changes_nothing(pkg, kind):
    """No backward kernel reads a bias (torch's conv does not save it either): no error, the same bits."""
    mod, graph, ref = subject(pkg, kind, "f32")
    one = single(mod, graph, 11)
    check(one, ref(11), "f32")
    zero(mod)
    loss, leaves, outs = graph(11)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("bias"):
                p.add_(0.1)
    loss.backward()
    same(collect(mod, leaves, outs), one)


# ================================================================== 6. double backward
@pytest.mark.parametrize("kind", ["pred", "seq", "cell"])
def test_double_backward_is_refused_not_dropped(pkg, kind):
    mod, graph, ref = subject(pkg, kind, "f32")
    one = single(mod, graph, 11)
    check(one, ref(11), "f32")
    zero(mod)
    loss, leaves, outs = graph(11)
    gs = torch.autograd.grad(loss, list(leaves.values()), create_graph=True)
    for k, g in zip(leaves, gs):
        assert torch.equal(g, one["d" + k]), k
        assert g.grad_fn is not None, f"d{k} came back without a graph: a penalty built on it would silently contribute nothing"
    with pytest.raises(RuntimeError, match="twice"):
        sum(g.square().sum() for g in gs).backward()
    del loss, gs
    same(single(mod, graph, 11), one)


# ================================================================== 7. input and cotangent forms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_input_forms(pkg, shape, dtype):
    """x permuted, sliced, f64, bf16: the glue makes the contiguous f32 copy the kernels read, so every route gives its
    contiguous f32 twin's bits, and x.grad comes back in x's own layout and dtype."""
    s, base = SHAPES[shape], shape.split("-")[0]
    net = make_net(pkg, shape, dtype)
    X, R, _ = batch(shape, 11)
    twin = run_std(net, X, dense(R))
    (eng,) = net._engines.values()                      # (the one make_net built)
    assert eng.cfgs[0].xfold == FOLDED[shape]
    check(twin, oracle((base, "pred", 11), shape, X, dense(R)), dtype)
    rest = [k for k in twin if k != "dX"]

    Xt = X.permute(1, 0, 2, 3, 4).contiguous().to(DEV).requires_grad_(True)              # (T, B, C, H, W)
    same(run(net, Xt.permute(1, 0, 2, 3, 4), dense(R)), twin, rest)
    assert torch.equal(Xt.grad.permute(1, 0, 2, 3, 4), twin["dX"])

    wide = torch.zeros(s["B"], s["T"], s["C"], s["H"], 2 * s["W"], device=DEV)
    wide[..., ::2] = X.to(DEV)
    wide[..., 1::2] = 7.0                                                                # must not be read
    wide.requires_grad_(True)
    same(run(net, wide[..., ::2], dense(R)), twin, rest)
    assert torch.equal(wide.grad[..., ::2], twin["dX"]) and not wide.grad[..., 1::2].any()

    x64 = X.double().to(DEV).requires_grad_(True)
    same(run(net, x64, dense(R)), twin, rest)
    assert x64.grad.dtype == torch.float64 and torch.equal(x64.grad.float(), twin["dX"]) and torch.equal(x64.grad, twin["dX"].double())

    Xb = X.bfloat16()
    twin_b = run_std(net, Xb.float(), dense(R))
    check(twin_b, oracle((base, "pred", "bf16-x"), shape, Xb.float(), dense(R)), dtype)
    xb = Xb.to(DEV).requires_grad_(True)
    same(run(net, xb, dense(R)), twin_b, rest)
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, twin_b["dX"].bfloat16())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_cotangent_forms(pkg, shape, dtype):
    """Expanded (stride 0), cropped and strided cotangents against dense ones of the same values."""
    base = shape.split("-")[0]
    net = make_net(pkg, shape, dtype)
    X, R, _ = batch(shape, 11)

    # pred.sum(): one element, expanded
    twin = run_std(net, X, lambda p: (p * torch.ones_like(p)).sum())
    check(twin, oracle((base, "pred", "ones"), shape, X, lambda p: p.sum()), dtype)
    same(run_std(net, X, lambda p: p.sum()), twin)

    # a loss on an inner window: the twin gets the same cotangent as a dense tensor
    def crop(p):
        return p[:, :, 1:-1, 2:-3].square().mean()

    got = run_std(net, X, crop)
    check(got, oracle((base, "pred", "crop"), shape, X, crop), dtype)
    pd = got["pred"].clone().requires_grad_(True)
    crop(pd).backward()
    G = pd.grad.contiguous()
    assert not G[:, :, 0].any() and G[:, :, 1:-1, 2:-3].any()
    same(run_std(net, X, lambda p: (p * G).sum()), got)

    # every second channel of seq, pred unused (its cotangent is absent)
    net_s = make_net(pkg, shape, dtype, seq=True)
    DS = torch.zeros(X.shape[0], SHAPES[shape]["T"] * SHAPES[shape]["out"], X.shape[3], X.shape[4])
    DS[:, 1::2] = 1.0
    twin = run_std(net_s, X, lambda p, q: (q * DS.to(q)).sum())
    check(twin, oracle((base, "seq", "odd"), shape, X, lambda p, q: q[:, 1::2].sum(), seq=True), dtype)
    same(run_std(net_s, X, lambda p, q: q[:, 1::2].sum()), twin)


@pytest.mark.parametrize("dtype", DTYPES)
def test_default_route_of_a_sequence_module_always_takes_the_per_step_head_backward(pkg, dtype):
    """net(x) of a return_sequence module with a loss on pred alone runs head_backward_seq and BPTT with per-step head
    gradients, as it does when seq has a cotangent too (model._CallOpts.seq_always) -- not the one-step head backward a call
    with state takes then, whose dw_head is summed in another order: the same loss plus (seq * 0).sum(), a zero cotangent
    for seq, gives the same bits."""
    net = make_net(pkg, "plain", dtype, seq=True)
    X, R, _ = batch("plain", 12)
    alone = run_std(net, X, lambda p, q: dense(R)(p))
    same(run_std(net, X, lambda p, q: dense(R)(p) + (q * 0).sum()), alone)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cell_state_forms(pkg, dtype):
    """h and c as channel slices of wider tensors, and as one zero expanded to (B, Ch, H, W)"""
    B, Ch, H, W = CELL["B"], CELL["Ch"], CELL["H"], CELL["W"]
    cell = make_cell(pkg, dtype)
    x, h, c, Dh, Dc = cell_data(11)
    loss = cell_loss(Dh, Dc)
    twin = run_cell_std(cell, x, h, c, loss)
    check(twin, oracle_cell(("cell", 11), x, h, c, loss), dtype)
    rest = [k for k in twin if k not in ("dx", "dh", "dc")]

    xd = x.to(DEV).requires_grad_(True)
    bh, bc = (torch.full((B, 2 * Ch, H, W), 7.0, device=DEV) for _ in range(2))
    bh[:, :Ch], bc[:, Ch:] = h.to(DEV), c.to(DEV)
    bh.requires_grad_(True), bc.requires_grad_(True)
    same(run_cell(cell, xd, bh[:, :Ch], bc[:, Ch:], loss), twin, rest)
    assert torch.equal(xd.grad, twin["dx"])
    assert torch.equal(bh.grad[:, :Ch], twin["dh"]) and not bh.grad[:, Ch:].any()
    assert torch.equal(bc.grad[:, Ch:], twin["dc"]) and not bc.grad[:, :Ch].any()

    x, h, c, Dh, Dc = cell_data(11, zero_state=True)
    twin = run_cell_std(cell, x, h, c, loss)
    check(twin, oracle_cell(("cell", 11, "zero-state"), x, h, c, loss), dtype)
    xd = x.to(DEV).requires_grad_(True)
    z = torch.zeros(1, 1, 1, 1, device=DEV).expand(B, Ch, H, W)                           # every stride 0
    same(run_cell(cell, xd, z, z, loss), twin, rest)
    assert torch.equal(xd.grad, twin["dx"])


# ================================================================== 8. frozen parameters
@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_parameters(pkg, dtype):
    s = SHAPES["plain"]
    net = make_net(pkg, "plain", dtype)
    X, R, _ = batch("plain", 11)
    ref = oracle(("plain", "pred", 11), "plain", X, dense(R))

    # nothing requires grad, grad mode on: an inference workspace, returned at once; no training workspace is ever made
    net.requires_grad_(False)
    assert torch.is_grad_enabled()
    pred = net(X.to(DEV))
    assert not pred.requires_grad and pred.grad_fn is None
    (ws,) = spaces(net)
    assert ws.key == (s["B"], s["T"], s["H"], s["W"], False, False) and not ws.in_use and spaces(net, train=True) == []
    check({"pred": pred}, ref, dtype, ["pred"])

    all_frozen = run_std(net, X, dense(R))                  # only X requires grad
    net.requires_grad_(True)
    base = run_std(net, X, dense(R))
    check(base, ref, dtype)
    assert all(all_frozen[k] is None for k in base if k.startswith("grad."))
    same(all_frozen, base, ["pred", "dX"])
    assert torch.equal(pred, base["pred"])

    net.layers[0].requires_grad_(False)
    part = run_std(net, X, dense(R))
    frozen = [k for k in base if k.startswith("grad.layers.0.")]
    assert len(frozen) == 2 and all(part[k] is None for k in frozen)
    same(part, base, [k for k in base if k not in frozen])
    assert not any(ws.in_use for ws in spaces(net))


# ================================================================== 9. lifetime
def test_workspaces_return_to_the_pool_when_graphs_die(pkg):
    net = make_net(pkg, "plain", "f32")
    X, _, _ = batch("plain", 11)
    Xd = X.to(DEV).requires_grad_(True)
    for _ in range(4):
        pred = net(Xd)
        assert pred.requires_grad
        del pred                                            # no backward
    (ws,) = spaces(net)
    assert ws.train and not ws.in_use

    kept = [net(Xd) for _ in range(3)]
    assert len(spaces(net)) == 3 and all(ws.in_use for ws in spaces(net))
    kept.clear()
    assert len(spaces(net)) == 3 and not any(ws.in_use for ws in spaces(net))
    pred = net(Xd)
    assert len(spaces(net)) == 3 and sum(ws.in_use for ws in spaces(net)) == 1


# ================================================================== 10. a side stream
@pytest.mark.parametrize("dtype", DTYPES)
def test_side_stream_gives_the_default_streams_bits(pkg, dtype):
    """Every launch and every temporary of the glue follows torch.cuda.current_stream()."""
    net = make_net(pkg, "plain", dtype)
    X, R, _ = batch("plain", 11)
    base = run_std(net, X, dense(R))
    check(base, oracle(("plain", "pred", 11), "plain", X, dense(R)), dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run_std(net, X, dense(R))
    torch.cuda.synchronize()
    same(got, base)


# ================================================================== 11. a deepcopy twin on the device
@pytest.mark.parametrize("dtype", DTYPES)
def test_deepcopy_twin_shares_nothing(pkg, dtype):
    net = make_net(pkg, "plain", dtype)
    (X1, R1, _), (X2, R2, _) = batch("plain", 11), batch("plain", 12)
    alone = run_std(net, X1, dense(R1))                     # (its engine exists now)
    check(alone, oracle(("plain", "pred", 11), "plain", X1, dense(R1)), dtype)
    twin = copy.deepcopy(net)
    assert twin._engines == {} and all(cell._engines == {} for cell in twin.layers)
    with torch.no_grad():
        for p in twin.parameters():
            p.mul_(1.25)
    twin_alone = run_std(twin, X2, dense(R2))
    check(twin_alone, oracle(("plain", "pred", 12, "x1.25"), "plain", X2, dense(R2),
                             params={k: 1.25 * v for k, v in params_of("plain").items()}), dtype)

    zero(net), zero(twin)
    A, Bx = X1.to(DEV).requires_grad_(True), X2.to(DEV).requires_grad_(True)
    a, b = net(A), twin(Bx)
    (a * R1.to(DEV)).sum().backward()
    (b * R2.to(DEV)).sum().backward()
    same({"pred": a.detach(), "dX": A.grad, **grads_of(net)}, alone)
    same({"pred": b.detach(), "dX": Bx.grad, **grads_of(twin)}, twin_alone)
    assert not {id(e) for e in net._engines.values()} & {id(e) for e in twin._engines.values()}
    assert len(net._engines) == 1 and len(twin._engines) == 1
