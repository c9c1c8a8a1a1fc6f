"""oracle/guarded_alloc.py must see what it claims to see: every mutation below is one the GPU memory-contract tests rely on
the helper to catch, made here on CPU tensors (``devices="all"``) by plain host writes.  Also the exact-size claim of the
weight-gradient workspace, through the library's own planner (no GPU): the engine's sizing rule without any slack plans what
1 GiB plans."""
import ctypes as C
import importlib.util
import io
import os
import re
from contextlib import redirect_stdout

import pytest
import torch

from oracle import guarded_alloc as GA

import test_launch_plan_cpu as TLP

ME = "test_guarded_alloc_cpu.py"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gt(mode="poison", **kw):
    return GA.GuardedTorch(mode, devices="all", **kw)


def _arena_of(gt, t):
    return next(a for a in gt.arenas if a.nbytes and a.arena.data_ptr() + a.front == t.data_ptr())


def test_unmodified_run_passes_and_counts():
    gt = _gt()
    a = gt.empty(3, 5, dtype=torch.float32)
    b = gt.zeros(7, dtype=torch.uint8)
    c = gt.full((4,), 2.5)
    d = gt.guard_copy(torch.arange(6.0).view(2, 3))
    a.fill_(1.0); b.fill_(9); c.mul_(2); d.add_(1)         # writes inside the payloads, up to their last byte
    assert gt.verify() == 4
    assert c.tolist() == [5.0] * 4 and d.tolist() == [[1, 2, 3], [4, 5, 6]]
    assert all(x.is_contiguous() for x in (a, b, c, d))


def test_guard_size_rule():
    assert GA.guard_bytes(0) == 64 * 1024
    assert GA.guard_bytes(100 * 256 * 4) == 4 * 100 * 256 * 4 and GA.guard_bytes(16385) == 68 * 1024    # whole pages
    gt = _gt(row_stride=20000)
    assert gt.guard == 80 * 1024 and gt.guard % 4096 == 0
    with pytest.raises(AssertionError):
        _gt(row_stride=40000, guard=64 * 1024)            # a guard smaller than four rows is refused, not measured
    t = gt.empty(5, dtype=torch.float64)
    a = _arena_of(gt, t)
    assert a.front == a.back == gt.guard and a.arena.numel() == 2 * gt.guard + 40
    if a.arena.data_ptr() % 256 == 0:
        assert t.data_ptr() % 256 == 0


@pytest.mark.parametrize("side,where,rel", [("back", "first", 0), ("front", "last", -1)])
def test_one_byte_next_to_the_payload_is_seen(side, where, rel):
    gt = _gt()
    other = gt.zeros(11, dtype=torch.float32)
    t = gt.empty(2, 3, 5, dtype=torch.bfloat16)           # 60 bytes: the back guard starts at byte 60, not at a rounded-up one
    a = _arena_of(gt, t)
    pos = a.front + a.nbytes if side == "back" else a.front - 1
    a.arena[pos] = 0x5A
    with pytest.raises(GA.GuardError) as e:
        gt.verify()
    msg = str(e.value)
    want = a.nbytes if side == "back" else -1
    assert f"{side} guard" in msg and "1 byte(s)" in msg and f"[{want}, {want}]" in msg
    assert "(2, 3, 5)" in msg and "bfloat16" in msg and re.search(ME + r":\d+", msg)
    assert "may exceed" not in msg and "(11,)" not in msg          # the neighbour is not blamed
    del other


def test_last_byte_of_the_back_guard_warns_that_the_overrun_may_exceed_it():
    gt = _gt()
    t = gt.empty(9, dtype=torch.float32)
    a = _arena_of(gt, t)
    a.arena[-1] = 0
    with pytest.raises(GA.GuardError, match="overrun may exceed the guard") as e:
        gt.verify()
    assert f"[{36 + a.back - 1}, {36 + a.back - 1}]" in str(e.value) and "back guard" in str(e.value)
    # ... and the first byte of the front guard
    gt = _gt("zero")
    t = gt.empty(9, dtype=torch.float32)
    _arena_of(gt, t).arena[0] = 1
    with pytest.raises(GA.GuardError, match="overrun may exceed the guard"):
        gt.verify()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_empty_payloads_are_nan_or_zero(dtype):
    for mode in ("poison", "zero"):
        gt = _gt(mode)
        a = gt.empty(2, 3, 4, 5, dtype=dtype)             # empty(B, O, H, W)
        b = gt.empty((2, 3), dtype=dtype)
        c = gt.empty_like(a)
        src = torch.ones(3, 2, dtype=dtype)
        d = gt.empty_like(src)
        for t, shape in ((a, (2, 3, 4, 5)), (b, (2, 3)), (c, (2, 3, 4, 5)), (d, (3, 2))):
            assert tuple(t.shape) == shape and t.dtype == dtype
            assert bool(torch.isnan(t).all()) if mode == "poison" else bool((t == 0).all())
        assert gt.verify() == 4
    gt = _gt("poison")
    assert gt.empty(6, dtype=torch.int32).tolist() == [-1] * 6


def test_zeros_payloads_are_zero_in_both_modes():
    for mode in ("poison", "zero"):
        gt = _gt(mode)
        z = gt.zeros(4, 6, dtype=torch.float32)
        zl = gt.zeros_like(torch.ones(5, dtype=torch.float64))
        u = gt.zeros(33, dtype=torch.uint8)
        assert GA.bits(z).sum() == 0 and GA.bits(zl).sum() == 0 and GA.bits(u).sum() == 0
        assert zl.dtype == torch.float64 and tuple(zl.shape) == (5,)
        a = _arena_of(gt, z)
        assert int(a.arena[a.front - 1]) == GA.FILL[mode] and int(a.arena[a.front + a.nbytes]) == GA.FILL[mode]
        gt.verify()


def test_cpu_allocations_pass_through_when_only_cuda_is_guarded():
    gt = GA.GuardedTorch("poison", devices="cuda")
    t = gt.empty(4, dtype=torch.float32)
    z = gt.zeros(4, device="cpu")
    f = gt.full((3,), 1.0)
    l = gt.empty_like(z)
    assert not gt.arenas and gt.verify() == 0
    assert t._base is None and z._base is None and f._base is None and l._base is None
    # everything else is torch's own
    assert gt.float32 is torch.float32 and gt.nn is torch.nn and gt.cat is torch.cat
    # a call the carver does not reproduce is torch's too
    out = torch.empty(2)
    assert _gt().zeros(2, out=out) is out


def test_patched_restores_module_torch_after_an_exception():
    import nasa_niswan_amd.engine as E
    import nasa_niswan_amd.trainer as TR
    before = {name: __import__("importlib").import_module("nasa_niswan_amd." + name).torch for name in GA.MODULES}
    assert all(v is torch for v in before.values())
    with pytest.raises(ZeroDivisionError):
        with GA.patched(mode="poison", devices="all") as gt:
            assert E.torch is gt and TR.torch is gt
            assert bool(torch.isnan(E.torch.empty(3, dtype=torch.float32)).all())
            1 / 0
    for name in GA.MODULES:
        assert __import__("importlib").import_module("nasa_niswan_amd." + name).torch is torch, name


def _stand_in_kernel(out: torch.Tensor, x: torch.Tensor, skip):
    """writes out = 2 * x through numpy into the payload's memory, but never touches element `skip`"""
    o, xs = out.numpy().reshape(-1), x.numpy().reshape(-1)
    for i in range(o.size):
        if i != skip:
            o[i] = 2 * xs[i]


def test_an_unwritten_output_element_differs_between_zero_and_poison():
    x = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    res = {}
    for skip in (None, 17):
        for mode in ("zero", "poison"):
            gt = _gt(mode)
            out = gt.empty(2, 3, 4, dtype=torch.float32)
            _stand_in_kernel(out, gt.guard_copy(x), skip)
            gt.verify()
            res[skip, mode] = out.clone()
    assert GA.same_bits(res[None, "zero"], res[None, "poison"])
    assert not GA.same_bits(res[17, "zero"], res[17, "poison"])
    assert bool(torch.isnan(res[17, "poison"]).any()) and not bool(torch.isnan(res[17, "zero"]).any())
    # the bitwise comparison sees what == does not: NaN payloads compare equal to themselves, -0.0 differs from 0.0
    n = torch.full((3,), float("nan"))
    assert GA.same_bits(n, n.clone()) and not GA.same_bits(torch.zeros(1), -torch.zeros(1))


def test_guard_copy_carries_values_dtype_and_requires_grad():
    gt = _gt()
    w = torch.randn(3, 4, dtype=torch.float64, requires_grad=True)
    g = gt.guard_copy(w)
    assert GA.same_bits(g, w) and g.requires_grad and g.is_leaf and g.dtype == torch.float64
    m = gt.guard_module(torch.nn.Conv2d(2, 3, 1))
    assert all(_arena_of(gt, p) is not None and p.requires_grad for p in m.parameters())
    (m(torch.ones(1, 2, 2, 2)).sum() + (g * g).sum()).backward()
    assert g.grad is not None and m.weight.grad is not None
    gt.verify()


# ------------------------------------------------------------------------------ the exact-size claim, through the planner
STACKS = [(5, [20, 12], [5, 3]), (40, [32, 16, 16], [3, 3, 3]), (64, [32], [3]), (4, [8, 8, 4], [3, 3, 3]), (3, [5], [3]),
          (16, [32, 16], [7, 7]), (6, [16], [1]), (1, [16], [3])]
GRIDS = [(13, 37), (8, 32), (9, 33), (3, 5)]


@pytest.mark.parametrize("BT", [(1, 1), (2, 3), (8, 8)], ids=["BT1", "BT6", "BT64"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_exact_wgrad_workspace_plans_what_a_gib_plans(dtype, BT):
    """wg_partial_bytes = sum over the layers of nint_wgrad_workspace_bytes rounded up to 256 -- the engine's rule, with no
    slack -- must give the launch list of a 1 GiB workspace.  Where that size has no room for layer 0's parked d/dh (merge_d,
    wave 4 / 5: B * H * W * Chp elements) the dgrad pair falls away by design: compared at wave = 2, as
    test_backward_plan_checks_the_weight_gradient_workspace documents."""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    B, T = BT
    n = 0
    for Cx, hidden, ks in STACKS:
        for H, W in GRIDS:
            for wave in (None, 0, 4, 5):
                s = TLP._seq_of(C_=Cx, hidden=hidden, ks=ks, B=B, T=T, H=H, W=W, dtype=dtype, wave=wave, need_dx=False)
                sized = sum((lib.nint_wgrad_workspace_bytes(C.byref(s.layer[l]), s.dtype, s.n_cu) + 255) // 256 * 256
                            for l in range(s.L))
                assert 0 < sized < s.wg_partial_bytes
                if sized < B * H * W * s.layer[0].Chp * (2 if dtype == "bf16" else 4) and s.wave in (4, 5):
                    s.wave = 2
                want = TLP._library_plan(s, True)
                assert any(g.pass_ == "bwd" for _, g in want)
                s.wg_partial_bytes = sized
                assert TLP._library_plan(s, True) == want, (Cx, hidden, ks, H, W, wave)
                n += 1
    assert n == len(STACKS) * len(GRIDS) * 4


# ------------------------------------------------------------------------------ tools/fuzz_shapes.py --guarded, without a GPU
@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("fuzz_shapes_guarded", os.path.join(ROOT, "tools", "fuzz_shapes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MODES = [[], ["--trainer"], ["--cell"], ["--dataset"], ["--state"], ["--train-opts"], ["--stateful"], ["--finetune"], ["--big"], ["--wide"]]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: (m or ["plain"])[0])
def test_guarded_does_not_change_the_draw(tool, mode):
    def listed(extra):
        buf = io.StringIO()
        with redirect_stdout(buf):
            tool.main(["--list", "--n", "9", "--seed", "5"] + mode + extra)
        return buf.getvalue()
    plain = listed([])
    assert plain.count("\n") == 9 and listed(["--guarded"]) == plain and listed(["--guarded", "--self-check"]) == plain
    args = tool.parse(["--n", "3"] + mode + ["--guarded", "--self-check"])
    assert args.guarded and args.guard_self_check and not args.self_check       # the reference is not corrupted as well
    for case in tool.draw_cases(5, 9, args.mode, args.big, args.wide):
        s = tool.case_row_stride(case)
        assert s > 0 and GA.guard_bytes(s) >= 4 * s
        assert "--guarded --only %d" % case["it"] in tool.replay_line(args, case)


def test_compare_fails_on_a_nan_in_the_device_result_whatever_the_gate(tool):
    """no `err <= tol` form of the screen lets a NaN through: a poisoned byte that reaches a result fails the comparison"""
    nan = float("nan")
    g = torch.Generator().manual_seed(0)
    t = torch.randn(2, 3, 4, 5, generator=g)
    bad = t.clone()
    bad[1, 2, 3, 4] = nan
    for dtype in ("f32", "bf16"):
        assert tool.compare("ok", dtype, {"pred": t.clone(), "loss": 1.0}, {"pred": t, "loss": 1.0}) == 0.0
        for res, ref in (({"pred": bad}, {"pred": t}), ({"loss": nan}, {"loss": 1.0}), ({"norm": nan}, {"norm": 2.0}),
                         ({"grad.layers.0.conv.weight": bad}, {"grad.layers.0.conv.weight": t})):
            with pytest.raises(AssertionError):
                tool.compare("nan", dtype, res, ref)
    # the bf16 sums that are gated on their factors
    dG = torch.randn(4, 8, 3, 3, generator=g)
    db = dG.sum(dim=(0, 2, 3))
    dbn = db.clone()
    dbn[5] = nan
    tool.check_bias_grad("ok", "b", db, db, dG, dG, "bf16")
    for args in ((dbn, db, dG, dG), (dbn, db, None, dG)):
        with pytest.raises(AssertionError):
            tool.check_bias_grad("nan", "b", *args, "bf16")
    h, dp = torch.randn(2, 4, 3, 3, generator=g), torch.randn(2, 2, 3, 3, generator=g)
    dW = torch.einsum("bohw,bchw->oc", dp.double(), h.double()).float()
    dWn = dW.clone()
    dWn[1, 2] = nan
    tool.check_head_wgrad("ok", dW, dW, h, h, dp)
    for hs in (h, None):
        with pytest.raises(AssertionError):
            tool.check_head_wgrad("nan", dWn, dW, hs, h, dp)
    assert not (tool._err("f32", bad, t) <= 1e9) and not (tool._err("bf16", bad, t) <= 1e9)
