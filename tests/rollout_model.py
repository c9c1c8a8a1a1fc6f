"""CPU model of ROLL-OUT TRAINING (TEST INFRASTRUCTURE ONLY): ``closed_loop_model.forward`` with the fed
value made explicitly straight-through,

    for every step t >= free_from:   x[:, t, C-O:] = p + (round_ET(p) - p).detach(),    p = head(h^{L-1} after step t-1)

so the forward value is the closed-loop model's, bit for bit, and the gradient passes the rounding with derivative 1 instead
of going through a dtype cast.  Run it in f64 under CPU autograd: ``grads`` returns every gradient the device produces."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

import closed_loop_model as CLM
import cyclic_model as CM


def forward(x, params, free_from: Optional[int] = None, cyclic: bool = False, storage: Optional[str] = "f32",
            h0: Optional[List[torch.Tensor]] = None, c0: Optional[List[torch.Tensor]] = None):
    """x (B,T,C,H,W) -> dict(pred, seq, hs, cs, x_fed) as closed_loop_model.forward returns them"""
    L = CM.num_layers_of(params)
    B, T, C, H, W = x.shape
    w, b = params["conv.weight"], params["conv.bias"]
    O = w.shape[0]
    s = T if free_from is None else int(free_from)
    if s < 0 or O > C or (s == 0 and h0 is None):
        raise ValueError("closed loop: 0 <= free_from, O <= C, and free_from = 0 only from a given state")
    hs, cs = [], []
    for i in range(L):
        ch = params[f"layers.{i}.conv.bias"].shape[0] // 4
        hs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if h0 is None else h0[i])
        cs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if c0 is None else c0[i])
    outs, fed = [], []
    for t in range(T):
        x_t = x[:, t]
        if t >= s:
            p = F.conv2d(hs[-1], w, b)
            x_t = torch.cat([x_t[:, :C - O], p + (CLM.round_et(p, storage) - p).detach()], dim=1)
        fed.append(x_t)
        for i in range(L):
            hs[i], cs[i] = CM.cell_forward(x_t, hs[i], cs[i], params[f"layers.{i}.conv.weight"], params[f"layers.{i}.conv.bias"], cyclic)
            x_t = hs[i]
        outs.append(F.conv2d(hs[-1], w, b))
    return dict(pred=outs[-1], seq=torch.cat(outs, dim=1), hs=hs, cs=cs, x_fed=torch.stack(fed, dim=1))


def grads(x, params, free_from, cyclic, storage, dpred=None, dseq=None, h0=None, c0=None, dhT=None, dcT=None):
    """Every gradient of  <pred, dpred> + <seq, dseq> + sum <h_T, dhT> + sum <c_T, dcT>  in the dtype of x (f64 in the tests):
    dict(pred, seq, x_fed, dx, params {name: grad}, dh0 [..], dc0 [..]).  ``free_from`` None or >= T: the open-loop model."""
    x = x.detach().clone().requires_grad_(True)
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    st = {}
    if h0 is not None:
        st = dict(h0=[t.detach().clone().requires_grad_(True) for t in h0], c0=[t.detach().clone().requires_grad_(True) for t in c0])
    r = forward(x, p, free_from, cyclic, storage, **st)
    tot = x.new_zeros(())
    if dpred is not None:
        tot = tot + (r["pred"] * dpred.to(x.dtype)).sum()
    if dseq is not None:
        tot = tot + (r["seq"] * dseq.to(x.dtype)).sum()
    for outs, cots in ((r["hs"], dhT), (r["cs"], dcT)):
        for o, d in zip(outs, cots or []):
            if d is not None:
                tot = tot + (o * d.to(x.dtype)).sum()
    tot.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(pred=r["pred"].detach(), seq=r["seq"].detach(), x_fed=r["x_fed"].detach(), dx=zero(x),
                params={k: zero(v) for k, v in p.items()},
                dh0=[zero(t) for t in st.get("h0", [])], dc0=[zero(t) for t in st.get("c0", [])])


# ------------------------------------------------------------------ the cases of tests/test_gpu_rollout.py, and their references
# closed_loop_model.CASES with synthetic weights whose feedback columns in layer 0 are scaled up: with the oracle's small
# weights the fed-back term moves the gradients by less than the gates of tests/test_gpu_parity.py, and a backward pass
# WITHOUT the feedback term would pass them.  At FEED_SCALE = 60 every parameter's roll-out gradient is many f32 gates away
# from the teacher-forced gradient on the same input, and with two or more fed steps at least one parameter is more than two
# bf16 gates (rel-L2 4e-2) away (asserted by tests/test_rollout_cpu.py for `all` and `thin`).
FEED_SCALE = 60.0
F32_GATE = lambda ref: 1e-3 * float(ref.abs().max()) + 1e-6         # max-abs error of an f32 gradient
BF16_GATE = 2e-2                                                    # rel-L2 error of a bf16 gradient


def case_params(c, dtype=torch.float32, seed=3):
    from oracle import convlstm_oracle as O
    p = O.synth_params(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=c["O"], seed=seed, dtype=dtype)
    p["layers.0.conv.weight"][:, c["C"] - c["O"]:c["C"]] *= FEED_SCALE
    return p


def case_data(c, seed=11):
    """X, an initial state, and cotangents of pred, seq and the final state (f32, as the device receives them)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    f = lambda *s, scale=1.0: torch.from_numpy((scale * rng.standard_normal(s)).astype(np.float32))
    d = dict(X=f(B, T, c["C"], H, W), h0=[f(B, ch, H, W, scale=0.5) for ch in c["hidden"]],
             c0=[f(B, ch, H, W, scale=0.5) for ch in c["hidden"]])
    # (the cotangents of the head outputs carry a mean: the head's bias gradient is their plain sum plus the fed term's, and with
    # zero-mean cotangents that sum is a difference of large numbers -- its relative error would measure the draw)
    d.update(dpred=0.5 + f(B, c["O"], H, W), dseq=0.5 + f(B, T * c["O"], H, W), dhT=[f(B, ch, H, W, scale=0.1) for ch in c["hidden"]],
             dcT=[f(B, ch, H, W, scale=0.1) for ch in c["hidden"]])
    return d


_REF = {}


def reference(case: str, cyclic: bool, F_: int, with_state: bool):
    """(roll-out gradients, teacher-forced gradients on the same x_fed) of a case in f64, fed values rounded to f32 (the f32
    model that both storage types are held against); computed once"""
    key = (case, cyclic, F_, with_state)
    if key not in _REF:
        c = CLM.CASES[case]
        d, p = case_data(c), case_params(c, torch.float64)
        kw = dict(dpred=d["dpred"], dseq=d["dseq"])
        if with_state:
            kw.update(h0=[t.double() for t in d["h0"]], c0=[t.double() for t in d["c0"]], dhT=d["dhT"], dcT=d["dcT"])
        ro = grads(d["X"].double(), p, F_, cyclic, "f32", **kw)
        tf = grads(ro["x_fed"], p, None, cyclic, "f32", **kw)
        _REF[key] = (ro, tf)
    return _REF[key]


def separation(ro, tf):
    """per parameter: (max-abs distance of the two gradients in f32 gates, their rel-L2 distance in bf16 gates)"""
    out = {}
    for k, g in ro["params"].items():
        t = tf["params"][k]
        out[k] = (float((g - t).abs().max()) / F32_GATE(g), float((g - t).norm() / g.norm()) / BF16_GATE)
    return out
