"""The guarded Adam step without a GPU: the comparator of tests/grad_clip_model.py has teeth, both new C entries validate
their arguments before any launch, and FusedAdam / train.py validate theirs.

A faithful numpy emulation of the control kernel (f64, sums in another order than math.fsum's) passes ``check_state`` over a
sequence of calls that clips, does not clip, skips and resumes; each plausible kernel bug below fails it:

    a coef without the + 1e-6; a coef not clamped to 1; s = gs * coef^2; a step that advances on a skipped call; bias
    correction taken from the number of calls instead of the applied steps; a norm that ignores grad_scale
"""
import ctypes as C
import math

import numpy as np
import pytest

import grad_clip_model as GM
from oracle import small_audit as SM

f32 = np.float32
LR, B1, B2 = 1e-3, 0.5, 0.999


def fails(fn):
    with pytest.raises(SM.AuditError):
        fn()


def emulate_guard(state, g, gs, max_norm, skip, lr=LR, b1=B1, b2=B2, mut=None):
    """adam_guard_kernel on a copy of ``state``: the reduction as 256 strided partials folded pairwise, then thread 0's f64 arithmetic"""
    st = np.array(state, np.float64)
    g64 = np.asarray(g, f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        part = np.array([np.sum(g64[b::256] ** 2) for b in range(256)])
        while part.size > 1:
            part = part[: part.size // 2] + part[part.size // 2:]
        S = float(part[0])
    gs = float(f32(gs))
    norm = math.sqrt(S) if mut == "norm_ignores_grad_scale" else gs * math.sqrt(S)
    finite = math.isfinite(S)
    coef = 1.0
    if max_norm > 0:
        c = max_norm / norm if mut == "no_1e-6" else max_norm / (norm + 1e-6)
        coef = c if (c < 1.0 or mut == "no_clamp") else 1.0
    apply = finite or not skip
    step = (st[GM.CALLS] if mut == "bias_correction_from_calls" else st[GM.APPLIED]) + 1.0
    st[GM.APPLIED] += 1.0 if (apply or mut == "step_advances_on_skip") else 0.0
    st[GM.SKIPPED] += 0.0 if apply else 1.0
    st[GM.CLIPPED] += 1.0 if (finite and coef < 1.0) else 0.0
    st[GM.CALLS] += 1.0
    if finite:
        st[GM.SUM_NORM] += norm
        st[GM.FINITE] += 1.0
        st[GM.MAX_NORM] = max(st[GM.MAX_NORM], norm)
    st[GM.S_], st[GM.NORM], st[GM.COEF] = S, norm, coef
    st[GM.SCALE] = float(f32(gs * coef * coef)) if mut == "coef_squared" else float(f32(gs * coef))
    st[GM.STEP_SIZE] = float(f32(lr / (1.0 - b1 ** step)))
    st[GM.SQRT_BC2] = float(f32(math.sqrt(1.0 - b2 ** step)))
    st[GM.APPLY] = 1.0 if apply else 0.0
    st[14] = st[15] = 0.0
    return st


def grad(seed=0, n=5000, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(f32)


def run(calls, mut=None, mut_at=None):
    """a sequence of (g, gs, max_norm, skip) calls, each audited against the state the call before left"""
    st, worst = np.zeros(GM.STATE), 0.0
    for i, (g, gs, mx, skip) in enumerate(calls):
        new = emulate_guard(st, g, gs, mx, skip, mut=mut if (mut_at is None or mut_at == i) else None)
        worst = max(worst, GM.check_state(new, g, g.size, gs, mx, skip, LR, B1, B2, before=st))
        st = new
    return st, worst


def sequence():
    """clips (norm ~ 70 > 1), does not clip (max_norm 1e3), skips a NaN, applies again with grad_scale 0.5, applies an inf unguarded"""
    bad = grad(3)
    bad[1234] = np.nan
    inf = grad(4)
    inf[-1] = np.inf
    return [(grad(1), 1.0, 1.0, True), (grad(2), 1.0, 1e3, True), (bad, 1.0, 1.0, True), (grad(5), 0.5, 1.0, True),
            (grad(6), 0.5, 0.0, True), (inf, 1.0, 1.0, False)]


def test_faithful_emulation_passes_and_counts():
    st, worst = run(sequence())
    assert worst <= 1.0
    assert (st[GM.APPLIED], st[GM.SKIPPED], st[GM.CLIPPED], st[GM.CALLS], st[GM.FINITE]) == (5, 1, 2, 6, 4)
    assert st[GM.APPLY] == 1.0 and math.isinf(st[GM.S_]) and st[GM.COEF] == 0.0


def test_model_is_clip_grad_norm_and_torch_bias_correction():
    """the model's coef is torch.nn.utils.clip_grad_norm_'s on f64 tensors, its step scalars torch.optim.Adam's"""
    import torch
    g = grad(7)
    for mx in (0.5, 50.0, 1e4):
        t = torch.zeros(g.size, dtype=torch.float64)
        t.grad = torch.from_numpy(g.astype(np.float64) * 0.5)
        total = float(torch.nn.utils.clip_grad_norm_([t], mx))
        c = GM.control(GM.sum_squares(g), 0.5, mx, False, 2.0, LR, B1, B2)
        assert abs(c["norm"] - total) <= 4 * 2.0 ** -52 * total
        np.testing.assert_allclose(t.grad.numpy(), g.astype(np.float64) * 0.5 * c["coef"], rtol=1e-15)
        assert c["step"] == 3.0 and c["step_size"] == float(f32(LR / (1 - B1 ** 3))) and (c["coef"] < 1) == (mx < total)


@pytest.mark.parametrize("mut,at", [("no_1e-6", 0), ("no_clamp", 1), ("coef_squared", 0), ("step_advances_on_skip", 2),
                                    ("bias_correction_from_calls", 3), ("norm_ignores_grad_scale", 3),
                                    ("norm_ignores_grad_scale", 4)])
def test_mutations_fail(mut, at):
    fails(lambda: run(sequence(), mut=mut, mut_at=at))


def test_check_state_sees_a_wrong_sum_and_wrong_counters():
    g = grad(8)
    good = emulate_guard(np.zeros(GM.STATE), g, 1.0, 1.0, True)
    assert GM.check_state(good, g, g.size, 1.0, 1.0, True, LR, B1, B2) <= 1.0
    for k, v in ((GM.S_, good[GM.S_] * (1 + 1e-9)), (GM.CALLS, 2.0), (GM.CLIPPED, 0.0), (GM.MAX_NORM, 0.0), (GM.FINITE, 0.0),
                 (GM.SUM_NORM, 0.0), (GM.SQRT_BC2, good[GM.SQRT_BC2] * (1 + 2.0 ** -22)), (GM.APPLY, 0.0)):
        bad = good.copy()
        bad[k] = v
        fails(lambda: GM.check_state(bad, g, g.size, 1.0, 1.0, True, LR, B1, B2))
    fails(lambda: GM.check_state(good, g, g.size - 1, 1.0, 1.0, True, LR, B1, B2))      # one element left out of the sum


def test_new_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """NINT_E_ARG / NINT_E_ALIGN come back before any HIP call (the pattern of tests/test_abi.py)"""
    from nasa_niswan_amd import _lib
    lib = _lib.load()
    E_ARG, E_ALIGN = -1, -4
    nb = lib.nint_grad_norm_scratch_bytes()
    assert nb == 8 * _lib.NINT_GRAD_NORM_BLOCKS and _lib.NINT_OPT_STATE >= 14
    assert lib.nint_grad_norm_flat(None, 10, 1.0, 16, 16, nb, None) == E_ARG
    assert lib.nint_grad_norm_flat(16, 10, 1.0, None, 16, nb, None) == E_ARG
    assert lib.nint_grad_norm_flat(16, 10, 1.0, 16, None, nb, None) == E_ARG
    assert lib.nint_grad_norm_flat(16, 10, 1.0, 16, 16, nb - 1, None) == E_ARG          # scratch too small
    assert lib.nint_grad_norm_flat(20, 10, 1.0, 20, 16, nb, None) == E_ALIGN            # out not 8-byte aligned (g may be)
    assert lib.nint_grad_norm_flat(20, 10, 1.0, 16, 12, nb, None) == E_ALIGN            # scratch not 8-byte aligned

    def guarded(p=16, g=16, m=16, v=16, max_norm=1.0, state=16, scratch=16, sb=nb):
        return lib.nint_adam_flat_guarded(p, g, m, v, 10, 1e-3, 0.5, 0.999, 1e-8, 1.0, max_norm, 1, state, scratch, sb, None)
    for k in ("p", "g", "m", "v", "state", "scratch"):
        assert guarded(**{k: None}) == E_ARG, k
    assert guarded(max_norm=-1.0) == E_ARG and guarded(max_norm=float("nan")) == E_ARG
    assert guarded(max_norm=-0.5, state=20) == E_ARG                                     # (the argument check comes first)
    assert guarded(sb=nb - 8) == E_ARG and guarded(sb=0) == E_ARG
    assert guarded(state=20) == E_ALIGN and guarded(scratch=4) == E_ALIGN


def test_fused_adam_validates_its_arguments():
    import torch
    from nasa_niswan_amd.optim import FlatParams, FusedAdam
    flat = FlatParams(torch.nn.Linear(3, 2))
    for bad in (-1.0, float("nan"), float("inf"), -1e-30):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdam(flat, max_grad_norm=bad)
    plain = FusedAdam(flat)
    assert not plain.guarded and plain.max_grad_norm is None
    with pytest.raises(RuntimeError, match="guarded"):
        plain.grad_stats()
    for kw in (dict(max_grad_norm=0), dict(max_grad_norm=2.5), dict(skip_nonfinite=True)):
        opt = FusedAdam(flat, **kw)
        assert opt.guarded
        assert opt.grad_stats()["applied"] == 0 and math.isnan(opt.grad_stats()["mean_norm"])
        # the dict stays torch's Adam format: the clip settings are constructor arguments, not state
        sd = opt.state_dict()
        assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        assert "max_grad_norm" not in sd["param_groups"][0] and set(sd["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
        sd["state"][0]["step"] = torch.tensor(7.0)
        sd["state"][1]["step"] = torch.tensor(7.0)
        opt.load_state_dict(sd)                                  # seeds the device counter
        assert opt.grad_stats()["applied"] == 7 and float(opt.state_dict()["state"][1]["step"]) == 7.0
        torch.optim.Adam(flat.params).load_state_dict(opt.state_dict())


def test_train_py_flags_land_in_configurations_json(tmp_path):
    import json
    from nasa_niswan_amd.train import get_arguments
    args = get_arguments(["--snapshot-dir", str(tmp_path), "--clip-grad-norm", "1.5", "--skip-nonfinite-steps"])
    assert args.clip_grad_norm == 1.5 and args.skip_nonfinite_steps is True
    cfg = json.load(open(tmp_path / "configurations.json"))
    assert cfg["clip_grad_norm"] == 1.5 and cfg["skip_nonfinite_steps"] is True
    args = get_arguments(["--snapshot-dir", str(tmp_path)])
    assert args.clip_grad_norm is None and args.skip_nonfinite_steps is False
