"""The guarded Adam step on the MI355X: nint_grad_norm_flat and nint_adam_flat_guarded through the C ABI against the f64 host
model of tests/grad_clip_model.py and the Adam audit of oracle/small_audit.py, then FusedAdam / FusedTrainer / train.py with
``max_grad_norm`` and ``skip_nonfinite`` against the oracle fit loop with torch.nn.utils.clip_grad_norm_.

Sizes: 1, 3, 255, 256, 257 and 1029 elements sit in the first pass of the norm kernel's strided loop (one workgroup, its edge,
several workgroups); 3 * 262144 + 1000 makes the one-element loop iterate; 256*32*256 + 77 is past grid1d's cap, so Adam's
grid-stride loop runs, and past 8 * 262144 threads, so the norm kernel's four-element loop runs twice with a 77-element tail.
Every size is also run with the buffers' base offset by one float (4-byte aligned only)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import grad_clip_model as GM
from oracle import small_audit as SM

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NORM_THREADS = 256 * 1024                  # NINT_GRAD_NORM_BLOCKS workgroups of 1024 threads
BIG = 256 * 32 * 256 + 77
SIZES = [1, 3, 255, 256, 257, 1029, 3 * NORM_THREADS + 1000, BIG]
LR, EPS = 1e-3, 1e-8


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import nasa_niswan_amd as pkg
    return pkg.load_library()


@pytest.fixture(scope="module")
def pkg(lib):
    import nasa_niswan_amd as p
    return p


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a, offset=0):
    """device copy of a 1-d f32 array whose pointer is ``offset`` floats past an allocation's (aligned) base"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    t = buf[offset:]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == (4 * offset) % 16
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


class Guard:
    """state + scratch of nint_adam_flat_guarded, and one audited call"""

    def __init__(self, lib):
        from nasa_niswan_amd import _lib
        self.lib = lib
        self.state = torch.zeros(_lib.NINT_OPT_STATE, dtype=torch.float64, device="cuda")
        self.nb = lib.nint_grad_norm_scratch_bytes()
        self.scratch = torch.full((self.nb // 8,), float("nan"), dtype=torch.float64, device="cuda")   # (never read before written)

    def call(self, p, g, m, v, gs, max_norm, skip, b1=0.5, b2=0.999, n=None, audit=True, what=""):
        """one call; the state against the model; p, m, v against the Adam audit with grad_scale = the device's s (applied) or
        bit-unchanged (skipped).  Returns the state read back."""
        n = p.numel() if n is None else n
        before = [host(t).copy() for t in (p, g, m, v)]
        st0 = host(self.state).copy()
        rc = self.lib.nint_adam_flat_guarded(P(p), P(g), P(m), P(v), n, LR, b1, b2, EPS, gs, max_norm, int(skip), P(self.state),
                                             P(self.scratch), self.nb, None)
        assert rc == 0, rc
        st = host(self.state).copy()
        worst = GM.check_state(st, before[1], n, gs, max_norm, skip, LR, b1, b2, before=st0)
        np.testing.assert_array_equal(host(g), before[1])           # the gradient is read-only
        after = [host(t) for t in (p, m, v)]
        if st[GM.APPLY] == 0.0:
            for a, b, k in zip(after, (before[0], before[2], before[3]), "pmv"):
                SM.check_equal(a, b, f"{what}: skipped step, {k}")
        elif audit:
            ref = SM.adam(*(b[:n] for b in before), LR, b1, b2, EPS, int(st[GM.APPLIED]), float(st[GM.SCALE]))
            for a, k in zip(after, "pmv"):
                r, bound = ref[k]
                err = np.abs(a[:n].astype(np.float64) - r)
                # the audit's bound, with the margin for the device's f64 pow / sqrt / divide in step_size and sqrt_bc2: a few
                # 2^-53 relative against the half-ulp-f32 host-cast term of the bound inflates it by less than 2^-26
                bad = ~(err <= bound * (1.0 + 2.0 ** -20))
                ratio = float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)))) if n else 0.0
                print(f"{what} step {int(st[GM.APPLIED])} {k}: worst ratio {ratio:.4f}")
                assert not bad.any(), (what, k, int(np.argmax(bad)), ratio)
        print(f"{what}: S {st[GM.S_]!r} norm {st[GM.NORM]!r} coef {st[GM.COEF]!r} apply {st[GM.APPLY]}; state worst ratio {worst:.3f}")
        return st


def adam_data(rng, n, offset=0, scale=1.0):
    g = (rng.standard_normal(n) * scale).astype(f32)
    p = rng.standard_normal(n).astype(f32)
    return dev(p, offset), dev(g, offset), dev(np.zeros(n, f32), offset), dev(np.zeros(n, f32), offset)


def plain_twin(lib, p, g, m, v, step, gs, b1=0.5, b2=0.999):
    """nint_adam_flat at `step` on copies of the buffers"""
    q = [t.clone() for t in (p, m, v)]
    assert lib.nint_adam_flat(P(q[0]), P(g), P(q[1]), P(q[2]), p.numel(), LR, b1, b2, EPS, step, gs, None) == 0
    return [host(t) for t in q]


# =========================================================================== the reduction
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "base+1float"])
@pytest.mark.parametrize("n", SIZES)
def test_norm_is_exact_on_integer_data_and_repeats_bit_for_bit(lib, n, offset):
    rng = np.random.default_rng(n)
    gi = rng.integers(-8, 9, n)
    want = float(int((gi.astype(np.int64) ** 2).sum()))              # < 2^53: exact in f64 whatever the order
    g = dev(gi.astype(f32), offset)
    nb = lib.nint_grad_norm_scratch_bytes()
    outs, states = [], []
    for rep in range(2):
        out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        scratch = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda")
        assert lib.nint_grad_norm_flat(P(g), n, 0.5, P(out), P(scratch), nb, None) == 0
        outs.append(host(out).copy())
        p, _, m, v = adam_data(np.random.default_rng(1), n, offset)
        gd = Guard(lib)
        states.append(gd.call(p, g, m, v, 0.5, 1.0, True, audit=(rep == 0 and n <= 1029), what=f"int n={n}"))
    assert outs[0][0] == want and states[0][GM.S_] == want, (outs[0][0], states[0][GM.S_], want)
    GM._close(outs[0][1], 0.5 * math.sqrt(want), GM.REL64 * 0.5 * math.sqrt(want), "norm of nint_grad_norm_flat")
    assert bits(outs[0]) == bits(outs[1]) and bits(states[0]) == bits(states[1])


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "base+1float"])
@pytest.mark.parametrize("n", [257, 1029, 3 * NORM_THREADS + 1000, BIG])
def test_norm_of_random_f32_data_within_the_fixed_order_summation_bound(lib, n, offset):
    rng = np.random.default_rng(100 + n)
    mags = np.array([1e-12, 1e-6, 1.0, 1.0, 124.0, 1e4], f32)        # heavy-tailed, like the z-scored inputs
    gh = (mags[rng.integers(0, mags.size, n)] * rng.standard_normal(n)).astype(f32)
    g = dev(gh, offset)
    nb = lib.nint_grad_norm_scratch_bytes()
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    scratch = torch.empty(nb // 8, dtype=torch.float64, device="cuda")
    assert lib.nint_grad_norm_flat(P(g), n, 0.25, P(out), P(scratch), nb, None) == 0
    S, norm = (float(x) for x in host(out))
    ref = GM.sum_squares(gh)
    print(f"n={n}: S {S!r} fsum {ref!r} |diff|/bound {abs(S - ref) / (n * 2.0 ** -53 * ref):.3e}")
    assert abs(S - ref) <= n * 2.0 ** -53 * ref
    GM._close(norm, 0.25 * math.sqrt(S), GM.REL64 * 0.25 * math.sqrt(S), "norm")
    # ... and the guarded entry folds the same partials to the same bits
    p, _, m, v = adam_data(rng, n, offset)
    st = Guard(lib).call(p, g, m, v, 0.25, 0.0, True, audit=False, what=f"random n={n}")
    assert st[GM.S_] == S and st[GM.NORM] == norm


def test_empty_bucket_is_a_call_with_norm_zero(lib):
    p, g, m, v = adam_data(np.random.default_rng(2), 8)
    keep = [host(t).copy() for t in (p, m, v)]
    gd = Guard(lib)
    st = gd.call(p, g, m, v, 1.0, 1.0, True, n=0, what="n=0")
    assert (st[GM.S_], st[GM.NORM], st[GM.COEF], st[GM.CALLS], st[GM.APPLIED]) == (0.0, 0.0, 1.0, 1.0, 1.0)
    for t, k in zip((p, m, v), keep):
        SM.check_equal(host(t), k, "n = 0 touches nothing")
    out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    assert lib.nint_grad_norm_flat(P(g), 0, 1.0, P(out), P(gd.scratch), gd.nb, None) == 0
    assert host(out).tolist() == [0.0, 0.0]


# =========================================================================== branches of the guarded step
@pytest.mark.parametrize("b1", [0.5, 0.9], ids=lambda b: f"beta1={b}")
@pytest.mark.parametrize("max_norm", [1e6, 0.0], ids=["norm<max_norm", "max_norm=0"])
def test_unclipped_guarded_steps_equal_plain_adam_bit_for_bit(lib, max_norm, b1):
    """coef == 1: s == grad_scale, and step_size / sqrt_bc2 formed on the device equal the host's: three steps, each equal to
    nint_adam_flat at the same step on copies of the same buffers"""
    rng = np.random.default_rng(5)
    n = 1029
    p, g, m, v = adam_data(rng, n, 1)
    gd = Guard(lib)
    for step in (1, 2, 3):
        g.copy_(dev(rng.standard_normal(n).astype(f32)))
        want = plain_twin(lib, p, g, m, v, step, 0.5, b1)
        st = gd.call(p, g, m, v, 0.5, max_norm, True, b1=b1, what=f"unclipped max_norm={max_norm}")
        assert st[GM.COEF] == 1.0 and st[GM.SCALE] == 0.5 and st[GM.APPLIED] == step and st[GM.CLIPPED] == 0
        for t, w, k in zip((p, m, v), want, "pmv"):
            SM.check_equal(host(t), w, f"step {step} {k}")


@pytest.mark.parametrize("n,offset,gs", [(257, 0, 1.0), (257, 0, 0.5), (1029, 1, 1.0), (1029, 1, 0.5), (BIG, 1, 0.5)])
def test_clipped_steps_pass_the_adam_audit_with_the_device_scale(lib, n, offset, gs):
    """norm > max_norm over three steps with different coefficients (the gradient grows); grad_scale 0.5 is the two-rank case"""
    rng = np.random.default_rng(6)
    p, g, m, v = adam_data(rng, n, offset)
    gd = Guard(lib)
    coefs = []
    for step in (1, 2, 3) if n < BIG else (1,):
        g.copy_(dev((rng.standard_normal(n) * step).astype(f32)))
        st = gd.call(p, g, m, v, gs, 0.75, True, what=f"clipped n={n} gs={gs}")
        assert st[GM.COEF] < 1.0 and st[GM.CLIPPED] == step and st[GM.APPLIED] == step
        # the scaled gradient's norm is max_norm (up to the 1e-6 of the formula)
        assert abs(st[GM.SCALE] / gs * st[GM.NORM] - 0.75) <= 1e-6 * 0.75 + 1e-6
        coefs.append(st[GM.COEF])
    assert len(set(coefs)) == len(coefs)
    s = gd.state.cpu().tolist()
    assert s[GM.MAX_NORM] == s[GM.NORM] and s[GM.FINITE] == len(coefs)


BAD_AT = [pytest.param(lambda n: 0, id="element0"), pytest.param(lambda n: n - 1, id="last-element"),
          pytest.param(lambda n: 8 * NORM_THREADS + 5, id="grid-stride-tail"),
          pytest.param(lambda n: 5 * NORM_THREADS + 12345, id="second-pass")]


@pytest.mark.parametrize("at", BAD_AT)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_nonfinite_gradient_is_skipped_and_the_next_step_is_step_one(lib, bad, at):
    rng = np.random.default_rng(7)
    n = BIG
    p, g, m, v = adam_data(rng, n, 1)
    clean = host(g).copy()
    poisoned = clean.copy()
    poisoned[at(n)] = bad
    g.copy_(torch.from_numpy(poisoned))
    gd = Guard(lib)
    st = gd.call(p, g, m, v, 1.0, 1e9, True, what="non-finite")      # (call() checks p, m, v bit-unchanged)
    assert (st[GM.APPLY], st[GM.APPLIED], st[GM.SKIPPED], st[GM.CALLS], st[GM.FINITE]) == (0.0, 0.0, 1.0, 1.0, 0.0)
    assert not math.isfinite(st[GM.S_])
    g.copy_(torch.from_numpy(clean))
    want = plain_twin(lib, p, g, m, v, 1, 1.0)
    st = gd.call(p, g, m, v, 1.0, 1e9, True, audit=False, what="after the skip")
    assert (st[GM.APPLY], st[GM.APPLIED], st[GM.SKIPPED], st[GM.CALLS]) == (1.0, 1.0, 1.0, 2.0)
    for t, w, k in zip((p, m, v), want, "pmv"):
        SM.check_equal(host(t), w, f"first applied step {k}")


def test_nonfinite_gradient_without_the_guard_is_applied(lib):
    rng = np.random.default_rng(8)
    n = 1029
    p, g, m, v = adam_data(rng, n)
    gh = host(g).copy()
    gh[700] = np.nan
    g.copy_(torch.from_numpy(gh))
    want = plain_twin(lib, p, g, m, v, 1, 1.0)
    gd = Guard(lib)
    st = gd.call(p, g, m, v, 1.0, 0.0, False, audit=False, what="NaN, skip_nonfinite = 0")
    assert (st[GM.APPLY], st[GM.APPLIED], st[GM.SKIPPED]) == (1.0, 1.0, 0.0) and math.isnan(st[GM.S_])
    ph = host(p)
    assert math.isnan(ph[700]) and np.isfinite(np.delete(ph, 700)).all()
    SM.check_equal(ph, want[0], "an unguarded NaN step is plain Adam's")


# =========================================================================== optimizer and trainer
def cfg0():
    g = np.load(os.path.join(GOLD, "cfg0_train.npz"))
    params = {k[len("params0."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("params0.")}
    return g, params, torch.from_numpy(g["X"]), torch.from_numpy(g["y"]), float(g["lr"]), tuple(float(b) for b in g["betas"])


def cfg0_trainer(pkg, params, lr, betas, **kw):
    from nasa_niswan_amd.trainer import FusedTrainer
    net = pkg.ConvLSTM(4, [8], [3], 1).cuda()
    net.load_state_dict(params)
    return net, FusedTrainer(net, lr=lr, betas=betas, halo=(0, 0), **kw)


_ORACLE = {}


def oracle_clipped_loop(max_norm):
    """three steps of the oracle fit loop (convlstm_oracle.train_step's body) with torch.nn.utils.clip_grad_norm_ between
    backward and the Adam step; computed once"""
    if max_norm in _ORACLE:
        return _ORACLE[max_norm]
    from oracle import convlstm_oracle as O
    _, params, X, y, lr, betas = cfg0()
    p = params
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}
    norms, losses, gmax = [], [], 0.0
    for step in (1, 2, 3):
        leaf = {k: t.detach().clone().requires_grad_(True) for k, t in p.items()}
        pred = O.crop_pred(O.convlstm_forward(X, leaf), (0, 0), y.shape[-2:]).squeeze()
        loss = O.loss_mse_l1(y, pred)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(leaf.values()), max_norm)))
        out = {k: O.adam_step_numpy(p[k].numpy(), leaf[k].grad.numpy(), m[k].numpy(), v[k].numpy(), step, lr, betas) for k in p}
        p = {k: torch.from_numpy(o[0]) for k, o in out.items()}
        m = {k: torch.from_numpy(o[1]) for k, o in out.items()}
        v = {k: torch.from_numpy(o[2]) for k, o in out.items()}
        losses.append(float(loss.detach()))
    _ORACLE[max_norm] = (p, m, v, norms, losses)
    return _ORACLE[max_norm]


def moments(tr):
    return {k: (tr.optimizer.state[p]["exp_avg"].detach().cpu(), tr.optimizer.state[p]["exp_avg_sq"].detach().cpu())
            for k, p in tr.model.named_parameters()}


def test_trainer_with_a_huge_max_grad_norm_equals_the_unclipped_trainer_bit_for_bit(pkg):
    _, params, X, y, lr, betas = cfg0()
    runs = []
    for kw in ({}, dict(max_grad_norm=1e9, skip_nonfinite=True)):
        net, tr = cfg0_trainer(pkg, params, lr, betas, **kw)
        losses = [float(tr.step(X.cuda(), y.cuda())) for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, tr.flat.data.cpu(), tr.optimizer.exp_avg.cpu(), tr.optimizer.exp_avg_sq.cpu(), tr))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1:4], runs[1][1:4]):
        assert torch.equal(a, b)
    gs = runs[1][4].grad_stats()
    assert (gs["applied"], gs["skipped"], gs["clipped"], gs["calls"], gs["last_coef"]) == (3, 0, 0, 3, 1.0)
    assert 0 < gs["mean_norm"] <= gs["max_norm"] and math.isfinite(gs["last_norm"])
    with pytest.raises(RuntimeError, match="guarded"):
        runs[0][4].grad_stats()


def test_clipped_trainer_matches_the_oracle_fit_loop_with_clip_grad_norm(pkg):
    """BASELINE configs[0], three steps, max_grad_norm 0.25 against gradient norms near 0.84: every step clips, each with its
    own coefficient.  Parameters at the tolerances of test_fused_trainer_matches_reference_fit_loop_cfg0 (max 6.5e-4, mean
    2e-6: Adam's first updates are +-lr whatever the gradient's scale, so they cannot tell a clipped step from an unclipped
    one) -- and therefore the moments too: exp_avg is linear in the clipped gradients, compared at that test's gradient
    tolerance 1e-3 max|ref| + 1e-7; exp_avg_sq is quadratic in them, so twice the relative term and the square of the
    absolute one, 2e-3 max|ref| + 1e-14."""
    MAXN = 0.25
    _, params, X, y, lr, betas = cfg0()
    p_ref, m_ref, v_ref, norms, losses = oracle_clipped_loop(MAXN)
    coefs = [MAXN / (nm + 1e-6) for nm in norms]
    print(f"  oracle norms {norms}, coefficients {coefs}")
    assert all(nm > MAXN for nm in norms) and len(set(coefs)) == 3          # checked on the CPU first: all three steps clip
    net, tr = cfg0_trainer(pkg, params, lr, betas, max_grad_norm=MAXN)
    _, plain = cfg0_trainer(pkg, params, lr, betas)
    for step in range(3):
        loss = float(tr.step(X.cuda(), y.cuda()))
        plain.step(X.cuda(), y.cuda())
        st = tr.grad_stats()
        print(f"  step {step + 1}: loss {loss:.7f} oracle {losses[step]:.7f}; norm {st['last_norm']:.7f} oracle {norms[step]:.7f}, "
              f"coef {st['last_coef']:.7f}")
        assert abs(loss - losses[step]) < 2e-6
        assert abs(st["last_norm"] - norms[step]) <= 1e-3 * norms[step] and abs(st["last_coef"] - coefs[step]) <= 1e-3 * coefs[step]
    st = tr.grad_stats()
    assert (st["applied"], st["clipped"], st["skipped"], st["calls"]) == (3, 3, 0, 3)
    assert abs(st["mean_norm"] - np.mean(norms)) <= 1e-3 * np.mean(norms) and abs(st["max_norm"] - max(norms)) <= 1e-3 * max(norms)
    for k, w in net.state_dict().items():
        d = (w.cpu() - p_ref[k]).abs()
        print(f"  {k}: max |dW| {float(d.max()):.2e}, mean {float(d.mean()):.2e}")
        assert float(d.max()) <= 6.5e-4 and float(d.mean()) <= 2e-6
    mo, mo_plain = moments(tr), moments(plain)
    for k in p_ref:
        em, ev = float((mo[k][0] - m_ref[k]).abs().max()), float((mo[k][1] - v_ref[k]).abs().max())
        print(f"  {k}: exp_avg err {em:.2e} of max {float(m_ref[k].abs().max()):.2e}; exp_avg_sq err {ev:.2e} of max {float(v_ref[k].abs().max()):.2e}")
        assert em <= 1e-3 * float(m_ref[k].abs().max()) + 1e-7, k
        assert ev <= 2e-3 * float(v_ref[k].abs().max()) + 1e-14, k
        assert not torch.equal(mo[k][0], mo_plain[k][0])                  # the clipped and the unclipped run do differ here
        # ... by the clip coefficient: far outside the tolerance above
        assert float((mo_plain[k][0] - m_ref[k]).abs().max()) > 0.5 * float(m_ref[k].abs().max())


def test_trainer_skips_a_batch_with_a_nan_and_trains_on(pkg, tmp_path):
    from nasa_niswan_amd.utils import load_checkpoint, save_checkpoint
    _, params, X, y, lr, betas = cfg0()
    net, tr = cfg0_trainer(pkg, params, lr, betas, skip_nonfinite=True)
    Xd, yd = X.cuda(), y.cuda()
    tr.step(Xd, yd)
    keep = [t.clone() for t in (tr.flat.data, tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq)]
    Xbad = Xd.clone()
    Xbad[1, 2, 3, 17, 5] = float("nan")
    assert math.isnan(float(tr.step(Xbad, yd)))
    for t, k in zip((tr.flat.data, tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq), keep):
        assert torch.equal(t, k)
    st = tr.grad_stats()
    assert (st["applied"], st["skipped"], st["calls"]) == (1, 1, 2) and math.isnan(st["last_norm"])
    # the following clean batch trains, as the second step of a run that never saw the bad batch
    _, twin = cfg0_trainer(pkg, params, lr, betas)
    for _ in range(2):
        want = float(twin.step(Xd, yd))
    assert float(tr.step(Xd, yd)) == want and torch.equal(tr.flat.data, twin.flat.data)
    assert torch.equal(tr.optimizer.exp_avg_sq, twin.optimizer.exp_avg_sq)
    st = tr.grad_stats(reset=True)
    assert (st["applied"], st["skipped"], st["calls"]) == (2, 1, 3)
    st = tr.grad_stats()
    assert (st["applied"], st["skipped"], st["calls"], st["max_norm"]) == (2, 0, 0, 0.0)
    # a checkpoint after the skipped step carries step = applied steps, in torch's Adam format
    ck = str(tmp_path / "generator.pth.tar")
    save_checkpoint(net, tr.optimizer, ck, [lr], 1)
    sd = torch.load(ck, weights_only=True)["optimizer_state_dict"]
    assert [float(s["step"]) for s in sd["state"].values()] == [2.0] * 4
    ref = torch.optim.Adam(pkg.ConvLSTM(4, [8], [3], 1).cuda().parameters(), lr=lr, betas=betas)
    ref.load_state_dict(sd)
    assert all(float(s["step"]) == 2.0 for s in ref.state.values())
    # ... and seeds the device counter of a resumed run: its next step is the twin's third
    net2, tr2 = cfg0_trainer(pkg, params, lr, betas, skip_nonfinite=True, max_grad_norm=1e9)
    load_checkpoint(ck, net2, tr2.optimizer, lr, map_location="cuda")
    assert tr2.grad_stats()["applied"] == 2
    assert float(tr2.step(Xd, yd)) == float(twin.step(Xd, yd)) and torch.equal(tr2.flat.data, twin.flat.data)


# =========================================================================== two ranks on one device
def _ddp_rank(rank, world, port, out, overlap):
    """One rank (gloo group, both ranks on cuda:0; the pattern of tests/test_gpu_train.py): three clipped steps, then a step
    with a NaN in rank 1's shard only, then a clean step."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import nasa_niswan_amd as p
    from nasa_niswan_amd.trainer import FusedTrainer
    from nasa_niswan_amd.utils import shard_indices
    torch.manual_seed(100 + rank)
    net = p.ConvLSTM(6, [16, 8], [3, 3], 2, out_channels=2, compute_dtype="f32").cuda()
    tr = FusedTrainer(net, lr=1e-2, halo=(2, 2), overlap_allreduce=overlap, max_grad_norm=1e-3, skip_nonfinite=True)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(4, 3, 6, 20, 28, generator=g)
    y = torch.randn(4, 2, 16, 24, generator=g)

    def snap():
        torch.cuda.synchronize()
        return {"w": tr.flat.data.cpu().clone(), "m": tr.optimizer.exp_avg.cpu().clone(), "v": tr.optimizer.exp_avg_sq.cpu().clone(),
                "state": tr.optimizer._opt_state.cpu().clone(), "stats": tr.grad_stats()}
    res = {}
    for step in range(5):
        idx = shard_indices(4, step, rank, world, 2, shuffle=False)[0]
        Xs = X[idx].clone()
        if step == 3 and rank == 1:
            Xs[0, 1, 2, 9, 9] = float("nan")
        tr.step(Xs.cuda(), y[idx].cuda())
        res[step] = snap()
    torch.save(res, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True], ids=["one-allreduce", "overlap_allreduce"])
def test_two_ranks_take_the_same_decisions_from_the_same_bits(pkg, tmp_path, overlap):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "ddp")
    mp.spawn(_ddp_rank, args=(2, port, out, overlap), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=False), torch.load(out + ".1", weights_only=False)
    for step in range(5):
        for k in ("w", "m", "v"):
            assert torch.equal(r0[step][k], r1[step][k]), (step, k)
        assert bits(r0[step]["state"].numpy()) == bits(r1[step]["state"].numpy()), step
    st = r0[2]["stats"]
    assert (st["applied"], st["clipped"], st["skipped"], st["calls"]) == (3, 3, 0, 3) and st["last_coef"] < 1.0
    assert float(r0[2]["state"][GM.SCALE]) < 0.5                         # s = coef / world
    # the NaN in rank 1's shard: BOTH ranks skip, nothing moves on either
    st = r0[3]["stats"]
    assert (st["applied"], st["skipped"], st["calls"]) == (3, 1, 4) and math.isnan(st["last_norm"])
    for k in ("w", "m", "v"):
        assert torch.equal(r0[3][k], r0[2][k]) and torch.equal(r1[3][k], r1[2][k]), k
    st = r0[4]["stats"]
    assert (st["applied"], st["skipped"], st["calls"], st["clipped"]) == (4, 1, 5, 4)
    assert not torch.equal(r0[4]["w"], r0[3]["w"]) and bool(torch.isfinite(r0[4]["w"]).all())


# =========================================================================== train.py
def test_train_py_with_clipping_prints_the_gradient_line(pkg, tmp_path, monkeypatch, capsys):
    from nasa_niswan_amd import train as T
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    snap = tmp_path / "s"
    argv = ["--model", "LSTM-cfg0", "--in-channels", "4", "--hidden-channels", "8", "--kernel-size", "3", "--num-layers", "1",
            "--sequence-length", "4", "--input-size", "32", "32", "--grid", "32", "32", "--batch-size", "2", "--num-epochs", "2",
            "--learning-rate", "1e-4", "--synthetic-steps", "24", "--dtype", "f32", "--snapshot-dir", str(snap)]
    logger = T.main(T.get_arguments(argv + ["--clip-grad-norm", "1", "--skip-nonfinite-steps"]))
    lines = capsys.readouterr().out.splitlines()
    epoch = [l for l in lines if l.startswith("Epoch: ")]
    grad = [l for l in lines if l.startswith("  grad norm: mean ")]
    assert len(epoch) == 2 and len(grad) == 2, lines
    for l in grad:
        mt = re.fullmatch(r"  grad norm: mean ([0-9.]+), max ([0-9.]+), clipped (\d+), skipped (\d+) of (\d+) steps", l)
        assert mt, l
        mean, mx, clipped, skipped, calls = float(mt[1]), float(mt[2]), int(mt[3]), int(mt[4]), int(mt[5])
        assert 0 < mean <= mx and skipped == 0 and calls == 9 and 0 <= clipped <= 9       # 17 windows in batches of 2, per epoch
    assert len(logger["MSELoss"]) == 2 and np.isfinite(logger["MSELoss"]).all()
    cfg = json.load(open(snap / "configurations.json"))
    assert cfg["clip_grad_norm"] == 1.0 and cfg["skip_nonfinite_steps"] is True
    with open(snap / "logger.npy", "rb") as f:                            # still three stacked arrays
        a, b, c = np.load(f), np.load(f), np.load(f)
        assert a.shape == b.shape == c.shape == (2,) and f.read() == b""
