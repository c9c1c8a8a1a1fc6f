"""Fine-tuning without a GPU: nint_seq.train_from's plan contract (the backward plan of (s, f) IS the plan of the sub-stack of
layers f .. L-1), the argument checks of the field and of nint_adam_flat_groups[_guarded], the f64 host model of the grouped
AdamW step (tests/finetune_model.py) against torch.optim.AdamW, the train_from rule of the autograd path, and FusedAdam's
groups, table and state_dict."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import finetune_model as FM
from test_launch_plan_cpu import _seq_of

E_ARG, E_ALIGN = -1, -4
STACKS = [dict(C_=5, hidden=[64, 32, 16], ks=[5, 3, 3]), dict(C_=5, hidden=[16, 16, 16, 16], ks=[3, 3, 3, 3])]
REC_FIELDS = ("index", "bwd", "op", "layer", "t", "kernel", "dtype", "epi", "wn", "wk", "ntw", "mt", "strip", "gx", "gy", "nt_begin")


def _struct(stack, dtype, wave=4, fuse=0, has_init=False, dh_seq=False, zero=False):
    s = _seq_of(B=2, T=3, H=20, W=40, dtype=dtype, wave=wave, fuse=fuse, has_init=has_init, zero=zero, need_dx=False, **stack)
    if dh_seq:
        s.dh_seq = 3 << 30
    return s


def _plan(s, bwd=1):
    from nasa_niswan_amd import _lib
    cap = 8 * (s.T + s.L + 1) * s.L
    recs = (_lib.NintLaunchRec * cap)()
    n = _lib.load().nint_debug_seq_plan(C.byref(s), bwd, recs, cap)
    if n < 0:
        return n
    assert n <= cap
    return [tuple(getattr(r, k) for k in REC_FIELDS) for r in recs[:n]]


def _copy(s):
    from nasa_niswan_amd import _lib
    v = _lib.NintSeq()
    C.memmove(C.byref(v), C.byref(s), C.sizeof(s))
    return v


def _sub_stack(s, f):
    """The sub-stack of include/nint.h's train_from contract, built here from its words: layers f .. L-1, the input slab h[f-1]
    from image B on, need_dx = 0, zero_dstate and an explicit fuse_bwd mask shifted down by f layers, everything else kept."""
    from nasa_niswan_amd import _lib
    v = _copy(s)
    es = 2 if s.dtype == _lib.NINT_BF16 else 4
    L = s.L - f
    v.train_from, v.L, v.need_dx, v.dx = 0, L, 0, None
    v.zero_dstate = s.zero_dstate >> (2 * f)
    if s.fuse_bwd & 0x40000000:
        m = s.fuse_bwd
        v.fuse_bwd = 0x40000000 | ((m & 0xff) >> f) | ((((m >> 8) & 0xff) >> f) << 8) | ((((m >> 16) & 0xff) >> f) << 16)
    v.xs = s.h[f - 1] + s.B * s.g.Hh * s.g.Wh * s.layer[f].Cxp * es
    for name in ("layer", "h", "c", "gates", "dG", "dh", "dc", "dW", "db"):
        src, dst = getattr(s, name), getattr(v, name)
        for l in range(_lib.NINT_MAX_LAYERS):
            if l < L:
                dst[l] = src[l + f]
            elif name == "layer":
                dst[l] = _lib.NintLayer()
            else:
                dst[l] = None
    return v


def _relabel(recs, f):
    li = REC_FIELDS.index("layer")
    return [r[:li] + (r[li] + f,) + r[li + 1:] for r in recs]


# =========================================================================== 1. the plan contract
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("stack", STACKS, ids=["64-32-16", "16x4"])
def test_backward_plan_of_a_frozen_prefix_is_the_plan_of_the_sub_stack(stack, dtype):
    L = len(stack["hidden"])
    n = 0
    for wave, fuse, has_init, dh_seq in itertools.product((0, 1, 2, 4, 5), (0, 1, 2), (False, True), (False, True)):
        s = _struct(stack, dtype, wave, fuse, has_init, dh_seq, zero=not has_init)
        base_b, base_f = _plan(s, 1), _plan(s, 0)
        assert isinstance(base_b, list) and base_b and isinstance(base_f, list)
        what = (wave, fuse, has_init, dh_seq)
        for f in range(0, L + 1):
            s.train_from = f
            assert _plan(s, 0) == base_f, (what, f)                     # the forward plan does not read the field
            got = _plan(s, 1)
            assert isinstance(got, list), (what, f, got)
            if f == 0:
                assert got == base_b, what                              # today's plan
            elif f == L:
                assert got == [], what                                  # the head alone: nothing planned
            else:
                sub = _sub_stack(s, f)
                want = _plan(sub, 1)
                assert isinstance(want, list) and want, (what, f)
                assert got == _relabel(want, f), (what, f)
                assert all(r[REC_FIELDS.index("layer")] >= f for r in got)
                n += 1
        s.train_from = 0
    assert n == 60 * (L - 1)


def test_explicit_fuse_masks_move_down_with_the_layers():
    """layer 2 fused and running layer 1's pointwise backward on its x columns (bits 2 and 8 + 2), then the classic layer 2
    doing so (bit 16 + 2): under train_from = 1 these are bits 1, 9 and 17 of the sub-stack"""
    for mask in (0x40000000 | 1 << 2 | 1 << 10, 0x40000000 | 1 << 18, 0x40000000 | 1 << 1 | 1 << 2):
        for dtype in ("f32", "bf16"):
            s = _struct(STACKS[0], dtype, 4, mask, zero=True)
            for f in (1, 2):
                s.train_from = f
                got, want = _plan(s, 1), _plan(_sub_stack(s, f), 1)
                assert isinstance(got, list) and got and got == _relabel(want, f), (hex(mask), dtype, f)


# =========================================================================== 2. argument checks
def test_train_from_argument_checks():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    s = _struct(STACKS[0], "bf16", 4, 0, zero=True)
    L = s.L
    assert isinstance(_plan(s), list)
    for bad in (-1, L + 1, 1 << 20):
        s.train_from = bad
        assert _plan(s) == E_ARG, bad
        assert lib.nint_seq_bwd(C.byref(s), None) == E_ARG, bad         # before any launch: readable without a GPU
    for f in (1, 2, L):
        s.train_from = f
        assert isinstance(_plan(s), list)
        s.need_dx = 1                                                    # (dx is set: with f = 0 this struct plans)
        assert _plan(s) == E_ARG, f
        s.need_dx = 0
        for parts in (1, 2):
            s.bwd_parts = parts
            assert _plan(s) == E_ARG, (f, parts)
        s.bwd_parts = 0
    s.train_from, s.need_dx = 0, 1
    assert isinstance(_plan(s), list)
    s.need_dx, s.bwd_parts = 0, 1
    assert isinstance(_plan(s), list)
    s.bwd_parts = 0


def test_frozen_layers_need_no_buffers_and_no_weight_gradient_workspace():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    for dtype in ("f32", "bf16"):
        s = _struct(STACKS[0], dtype, 4, 0, zero=True)
        L = s.L
        need = [(lib.nint_wgrad_workspace_bytes(C.byref(s.layer[l]), s.dtype, s.n_cu) + 255) // 256 * 256 for l in range(L)]
        assert all(v > 0 for v in need)
        for f in range(1, L + 1):
            s.train_from = f
            want = _plan(s)
            v = _copy(s)
            for l in range(f):
                v.gates[l] = v.dG[l] = v.dh[l] = v.dc[l] = v.dW[l] = v.db[l] = None
            assert _plan(v) == want, (dtype, f)
            if f < L:
                v.gates[f] = None                                        # ... a trained layer's are still required
                assert _plan(v) == E_ARG, (dtype, f)
                v.gates[f] = s.gates[f]
            # the workspace of the trained layers alone is enough (wave 0: no d/dh piece of the bottom layer in its head)
            v.wg_partial_bytes, v.wave = sum(need[f:]), 0
            s.wave = 0
            assert _plan(v) == _plan(s), (dtype, f)
            s.wave = 4
        s.train_from = L
        s.wg_partial = None                                              # nothing planned: no workspace at all
        assert _plan(s) == []


def _groups(rows):
    from nasa_niswan_amd import _lib
    return (_lib.NintOptGroup * max(len(rows), 1))(*[_lib.NintOptGroup(*r) for r in rows])


def test_grouped_adam_argument_checks():
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    assert _lib.NINT_MAX_OPT_GROUPS == 2 * _lib.NINT_MAX_LAYERS + 2 == 18
    assert C.sizeof(_lib.NintOptGroup) == 32
    nan, inf = float("nan"), float("inf")
    good = [(3, 130, 1e-3, 1e-2), (130, 131, 1e-4, 0.0), (131, 900, 3e-4, 0.1)]
    bad_tables = {
        "empty group": [(3, 3, 1e-3, 0.0)], "reversed group": [(5, 3, 1e-3, 0.0)],
        "gap": [(3, 130, 1e-3, 0.0), (131, 900, 1e-3, 0.0)], "overlap": [(3, 130, 1e-3, 0.0), (129, 900, 1e-3, 0.0)],
        "unsorted": [(131, 900, 1e-3, 0.0), (3, 131, 1e-3, 0.0)],
        "negative lr": [(3, 130, -1e-3, 0.0)], "nan lr": [(3, 130, nan, 0.0)], "inf lr": [(3, 130, inf, 0.0)],
        "negative decay": good[:2] + [(131, 900, 1e-3, -0.1)], "nan decay": [(3, 130, 1e-3, nan)], "inf decay": [(3, 130, 1e-3, inf)],
    }
    plain = lambda tab, n, p=16, step=1: lib.nint_adam_flat_groups(p, 16, 16, 16, tab, n, 0.5, 0.999, 1e-8, step, 1.0, None)
    guard = lambda tab, n, state=16, gstate=16, scratch=16, max_norm=1.0, nb=None: lib.nint_adam_flat_groups_guarded(
        16, 16, 16, 16, tab, n, 0.5, 0.999, 1e-8, 1.0, max_norm, 1, state, gstate, scratch,
        lib.nint_grad_norm_scratch_bytes() if nb is None else nb, None)
    for name, rows in bad_tables.items():
        assert plain(_groups(rows), len(rows)) == E_ARG, name
        assert guard(_groups(rows), len(rows)) == E_ARG, name
    many = [(i, i + 1, 1e-3, 0.0) for i in range(_lib.NINT_MAX_OPT_GROUPS + 1)]
    for fn in (plain, guard):
        assert fn(_groups(good), 0) == E_ARG and fn(_groups(good), -1) == E_ARG
        assert fn(_groups(many), len(many)) == E_ARG
        assert fn(None, 3) == E_ARG
    assert plain(_groups(good), 3, p=None) == E_ARG
    assert plain(_groups(good), 3, step=0) == E_ARG                      # step is 1-based
    assert guard(_groups(good), 3, gstate=None) == E_ARG
    assert guard(_groups(good), 3, state=None) == E_ARG
    assert guard(_groups(good), 3, max_norm=-1.0) == E_ARG and guard(_groups(good), 3, max_norm=nan) == E_ARG
    assert guard(_groups(good), 3, nb=8) == E_ARG                        # scratch too small
    # a valid table in front of a misaligned buffer: the alignment check is the last one before the launches
    assert guard(_groups(good), 3, gstate=20) == E_ALIGN
    assert guard(_groups(good), 3, state=20) == E_ALIGN
    assert guard(_groups(many[:-1]), len(many) - 1, scratch=20) == E_ALIGN   # (NINT_MAX_OPT_GROUPS groups are a valid table)


# =========================================================================== 3. the host model against torch.optim.AdamW
def test_host_model_of_the_grouped_step_matches_torch_adamw():
    n, b1, b2, eps = 4097, 0.5, 0.999, 1e-8
    groups = [(0, 130, 1e-3, 1e-2), (130, 131, 1e-4, 0.0), (131, 4000, 3e-4, 0.1)]
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal(n).astype(np.float32)
    tp = [torch.nn.Parameter(torch.from_numpy(p0[b:e].copy())) for b, e, _, _ in groups]
    opt = torch.optim.AdamW([dict(params=[t], lr=lr, weight_decay=wd) for t, (_, _, lr, wd) in zip(tp, groups)], lr=1e-3,
                            betas=(b1, b2), eps=eps, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for step in range(1, 6):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
        for t, (b, e, _, _) in zip(tp, groups):
            t.grad = torch.from_numpy(g[b:e].copy())
        opt.step()
        p64, m64, v64 = FM.grouped_adamw(p, g, m, v, groups, b1, b2, eps, step)
        p, m, v = (a.astype(np.float32) for a in (p64, m64, v64))       # (as stored: the next step starts from f32)
        for t, (b, e, _, _) in zip(tp, groups):
            st = opt.state[t]
            for mine, ref in ((p[b:e], t.detach().numpy()), (m[b:e], st["exp_avg"].numpy()), (v[b:e], st["exp_avg_sq"].numpy())):
                np.testing.assert_allclose(mine, ref, rtol=2e-6, atol=1e-7)
            worst = max(worst, float(np.abs(p[b:e].astype(np.float64) - t.detach().numpy().astype(np.float64)).max()))
        assert np.array_equal(p[4000:], p0[4000:]) and not m[4000:].any() and not v[4000:].any()    # the frozen tail
    print(f"host model against torch.optim.AdamW over five steps: max |p - torch| {worst:.3e}")


def test_decay_free_group_of_the_model_is_plain_adam():
    rng = np.random.default_rng(5)
    p, g = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    z = np.zeros(64, np.float32)
    assert FM.decay_multiplier(1e-3, 0.0) == 1.0
    got = FM.grouped_adamw(p, g, z, z, [(0, 64, 1e-3, 0.0)], 0.5, 0.999, 1e-8, 1)
    from oracle import small_audit as SM
    ref = SM.adam(p, g, z, z, 1e-3, 0.5, 0.999, 1e-8, 1)
    np.testing.assert_allclose(got[0], ref["p"][0], rtol=1e-14, atol=0)


# =========================================================================== 4. the rule, and FusedAdam's groups
def test_train_from_rule():
    from nasa_niswan_amd.model import train_from_rule as rule
    assert rule(True, [False, False, False]) == 0                        # the input's gradient passes through every layer
    assert rule(True, [False, False, True]) == 0
    assert rule(False, [True, True, True]) == 0
    assert rule(False, [False, True, True]) == 1
    assert rule(False, [False, False, True]) == 2
    assert rule(False, [False, True, False]) == 1                        # any requires_grad pattern: the lowest layer decides
    assert rule(False, [False, False, False]) == 3                       # the head alone
    assert rule(False, [False]) == 1 and rule(False, [True]) == 0


def _net(hidden=(8, 4, 4)):
    import nasa_niswan_amd as pkg
    torch.manual_seed(0)
    return pkg.ConvLSTM(3, list(hidden), [3] * len(hidden), len(hidden), out_channels=2)


TODAY = ["params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused"]


def test_default_fused_adam_is_what_it_was():
    from nasa_niswan_amd.optim import FlatParams, FusedAdam
    net = _net()
    opt = FusedAdam(FlatParams(net), lr=1e-3, betas=(0.5, 0.999))
    assert not opt.grouped and opt.n0 == 0
    assert len(opt.param_groups) == 1 and list(opt.param_groups[0]) == TODAY
    assert opt.param_groups[0]["weight_decay"] == 0 and len(opt.param_groups[0]["params"]) == 8
    assert all(p.requires_grad for p in net.parameters())
    sd = opt.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(8))
    assert all(sorted(v) == ["exp_avg", "exp_avg_sq", "step"] for v in sd["state"].values())
    assert sorted(sd["param_groups"][0]) == sorted(TODAY) and sd["param_groups"][0]["params"] == list(range(8))


@pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step")      # (no device step on a machine without a GPU)
@pytest.mark.parametrize("freeze", [0, 1, 3])
def test_fused_adam_groups_table_and_state_dict_round_trip_with_torch_adamw(freeze):
    from nasa_niswan_amd.optim import FlatParams, FusedAdam
    net, L = _net(), 3
    flat = FlatParams(net)
    scales = [0.1, 0.5, 1.0]
    opt = FusedAdam(flat, lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-2, freeze_layers=freeze, layer_lr_scale=scales)
    params = list(net.parameters())
    assert [p.requires_grad for p in params] == [False] * (2 * freeze) + [True] * (8 - 2 * freeze)
    assert opt.grouped and opt.n0 == flat.offsets[2 * freeze]
    want_lr = [1e-3 * s for s in scales[freeze:]] + [1e-3 * scales[-1]]     # the head goes with the top layer
    assert [g["lr"] for g in opt.param_groups] == want_lr
    assert [[id(p) for p in g["params"]] for g in opt.param_groups] == [[id(params[2 * l]), id(params[2 * l + 1])]
                                                                         for l in range(freeze, L + 1)]
    assert all(g["weight_decay"] == 1e-2 for g in opt.param_groups)
    # the table: weight and bias of every trained layer, the bias without decay; it tiles [n0, numel)
    tab = [(r.begin, r.end, r.lr, r.weight_decay) for r in opt.group_table()]
    FM.check_table(tab, flat.numel)
    assert tab[0][0] == opt.n0 and tab[-1][1] == flat.numel and len(tab) == 2 * (L + 1 - freeze)
    for k, (b, e, lr, wd) in enumerate(tab):
        i = 2 * freeze + k
        assert (b, e) == (flat.offsets[i], flat.offsets[i] + params[i].numel())
        assert lr == want_lr[k // 2] and wd == (1e-2 if k % 2 == 0 else 0.0)
    # torch.optim.AdamW over filter(requires_grad) with the same groups: state dicts load both ways
    mirror = [torch.nn.Parameter(p.detach().clone()) for p in params[2 * freeze:]]
    tw = torch.optim.AdamW([dict(params=mirror[2 * j:2 * j + 2], lr=g["lr"]) for j, g in enumerate(opt.param_groups)], lr=1e-3,
                           betas=(0.5, 0.999), weight_decay=1e-2, foreach=False)
    assert [list(g) for g in tw.state_dict()["param_groups"]] == [list(g) for g in opt.state_dict()["param_groups"]]
    for q in mirror:
        q.grad = torch.randn_like(q)
    tw.step()
    opt.load_state_dict(tw.state_dict())
    for (p, off), q in zip(opt.trained, mirror):
        k = p.numel()
        assert torch.equal(opt.exp_avg[off:off + k].view(q.shape), tw.state[q]["exp_avg"])
        assert torch.equal(opt.exp_avg_sq[off:off + k].view(q.shape), tw.state[q]["exp_avg_sq"])
        assert float(opt.state[p]["step"]) == 1.0
    assert not opt.exp_avg[:opt.n0].any()                                # the frozen layers have no moments
    assert opt._step == 1
    tw2 = torch.optim.AdamW([dict(params=mirror[2 * j:2 * j + 2]) for j in range(len(opt.param_groups))], lr=1.0, foreach=False)
    tw2.load_state_dict(opt.state_dict())
    assert [g["lr"] for g in tw2.param_groups] == [g["lr"] for g in opt.param_groups]
    for q in mirror:
        assert torch.equal(tw2.state[q]["exp_avg"], tw.state[q]["exp_avg"])
    # a scheduler drives every group, and the next table follows
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    sch.step()
    assert [r.lr for r in opt.group_table()][::2] == [0.5 * v for v in want_lr]


def test_fused_adam_refuses_what_it_cannot_group():
    from nasa_niswan_amd.optim import FlatParams, FusedAdam
    net = _net()
    flat = FlatParams(net)
    for kw in (dict(freeze_layers=4), dict(freeze_layers=-1), dict(weight_decay=-1.0), dict(weight_decay=float("nan")),
               dict(layer_lr_scale=[1.0, 1.0]), dict(layer_lr_scale=[1.0, -1.0, 1.0])):
        with pytest.raises(ValueError):
            FusedAdam(flat, **kw)
    lin = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="ConvLSTM"):
        FusedAdam(FlatParams(lin), weight_decay=0.1)
    assert len(FusedAdam(flat, layer_lr_scale=[1.0, 1.0, 1.0, 2.0]).param_groups) == 4     # a factor of the head's own


def test_checkpoint_with_other_groups_is_refused_unless_the_optimizer_is_reset(tmp_path):
    from nasa_niswan_amd.optim import FlatParams, FusedAdam
    from nasa_niswan_amd.utils import load_checkpoint, save_checkpoint
    net = _net()
    full = FusedAdam(FlatParams(net), lr=1e-3)
    path = str(tmp_path / "generator.pth.tar")
    save_checkpoint(net, full, path, [1e-3], 7)
    net2 = _net()
    with torch.no_grad():
        for p in net2.parameters():
            p.add_(1.0)
    tuned = FusedAdam(FlatParams(net2), lr=1e-3, freeze_layers=1, layer_lr_scale=[1.0, 0.5, 1.0])
    with pytest.raises(ValueError, match="reset_optimizer"):
        load_checkpoint(path, net2, tuned, 1e-4)
    load_checkpoint(path, net2, tuned, 1e-4, reset_optimizer=True)
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values()))
    assert [g["lr"] for g in tuned.param_groups] == [1e-3 * 0.5, 1e-3, 1e-3] and tuned._step == 0
    # a matching optimizer loads, and the CLI learning rate keeps each group's factor
    tuned2 = FusedAdam(FlatParams(_net()), lr=1e-3, freeze_layers=1, layer_lr_scale=[1.0, 0.5, 1.0])
    save_checkpoint(net2, tuned, path, [1e-3], 7)
    load_checkpoint(path, _net(), tuned2, 1e-4)
    assert [g["lr"] for g in tuned2.param_groups] == pytest.approx([1e-4 * 0.5, 1e-4, 1e-4])


def test_train_py_flags(tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("nint_train_cli", os.path.join(root, "nasa-niswan_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.get_arguments(["--snapshot-dir", str(tmp_path)])
    assert (a.freeze_layers, a.weight_decay, a.layer_lr_scale, a.reset_optimizer) == (0, 0.0, None, False)
    a = mod.get_arguments(["--snapshot-dir", str(tmp_path), "--freeze-layers", "2", "--weight-decay", "0.01", "--layer-lr-scale",
                           "0.1", "0.5", "1", "--reset-optimizer"])
    assert (a.freeze_layers, a.weight_decay, a.layer_lr_scale, a.reset_optimizer) == (2, 0.01, [0.1, 0.5, 1.0], True)
    for bad in (["--freeze-layers", "4"], ["--layer-lr-scale", "1", "1"]):
        with pytest.raises(SystemExit):
            mod.get_arguments(["--snapshot-dir", str(tmp_path)] + bad)
