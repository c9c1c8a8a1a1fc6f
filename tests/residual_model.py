"""CPU model of the RESIDUAL HEAD (TEST INFRASTRUCTURE ONLY): ``sampled_model.forward`` -- the stack, the
rounding, the straight-through fed value of tests/closed_loop_model.py / rollout_model.py -- with the head predicting the
increment,

    p_t = x_t[:, C-O:] + head(h^{L-1} after step t),      x_t as the model saw it,
    for every (b, t) with fed[b, t]:   x[b, t, C-O:] = p + (round_ET(p) - p).detach(),    p = p_{t-1}[b]

``fed`` is None (nothing fed), a step index s (``fed[b, t] = (t >= s)``) or a (B, T) mask; step 0 is never fed (p_{-1} has no
base).  ``skip=False`` detaches the base of the fed images: the forward values stay, the identity path from p_t into p_{t-1} is
cut -- the gradients a backward pass WITHOUT the ``+ g_u`` term of nint_head_feedback_bwd_res would give."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

import closed_loop_model as CLM
import cyclic_model as CM
import rollout_model as RM
import sampled_model as SM


def fed_mask(fed, B: int, T: int) -> torch.Tensor:
    if fed is None:
        return torch.zeros(B, T, dtype=torch.bool)
    if isinstance(fed, int):
        return SM.suffix(B, T, fed)
    return torch.as_tensor(fed).bool()


def forward(x, params, fed=None, cyclic: bool = False, storage: Optional[str] = "f32",
            h0: Optional[List[torch.Tensor]] = None, c0: Optional[List[torch.Tensor]] = None, skip: bool = True):
    """x (B,T,C,H,W) -> dict(pred, seq, hs, cs, x_fed) as rollout_model.forward returns them"""
    L = CM.num_layers_of(params)
    B, T, C, H, W = x.shape
    w, b = params["conv.weight"], params["conv.bias"]
    O = w.shape[0]
    fed = fed_mask(fed, B, T)
    if tuple(fed.shape) != (B, T) or O > C or bool(fed[:, 0].any()):
        raise ValueError("residual head: fed is (B, T), O <= C, and step 0 is never fed")
    hs, cs = [], []
    for i in range(L):
        ch = params[f"layers.{i}.conv.bias"].shape[0] // 4
        hs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if h0 is None else h0[i])
        cs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if c0 is None else c0[i])
    outs, seen = [], []
    for t in range(T):
        x_t = x[:, t]
        m = fed[:, t].view(B, 1, 1, 1)
        if bool(fed[:, t].any()):
            p = outs[-1]
            val = p + (CLM.round_et(p, storage) - p).detach()
            x_t = torch.cat([x_t[:, :C - O], torch.where(m, val, x_t[:, C - O:])], dim=1)
        seen.append(x_t)
        base = x_t[:, C - O:]
        if not skip:
            base = torch.where(m, base.detach(), base)
        inp = x_t
        for i in range(L):
            hs[i], cs[i] = CM.cell_forward(inp, hs[i], cs[i], params[f"layers.{i}.conv.weight"], params[f"layers.{i}.conv.bias"], cyclic)
            inp = hs[i]
        outs.append(F.conv2d(hs[-1], w, b) + base)
    return dict(pred=outs[-1], seq=torch.cat(outs, dim=1), hs=hs, cs=cs, x_fed=torch.stack(seen, dim=1))


def grads(x, params, fed, cyclic, storage, dpred=None, dseq=None, h0=None, c0=None, dhT=None, dcT=None, skip: bool = True):
    """rollout_model.grads for this model: every gradient of <pred, dpred> + <seq, dseq> + sum <h_T, dhT> + sum <c_T, dcT>"""
    x = x.detach().clone().requires_grad_(True)
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    st = {}
    if h0 is not None:
        st = dict(h0=[t.detach().clone().requires_grad_(True) for t in h0], c0=[t.detach().clone().requires_grad_(True) for t in c0])
    r = forward(x, p, fed, cyclic, storage, skip=skip, **st)
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


def recursion(x, params, fed, cyclic, storage, dpred=None, dseq=None):
    """The same gradients WITHOUT autograd across steps: the rule of nint_seq_bwd_rollout_residual written out.  Every step is
    differentiated by itself (its inputs cut loose), and the steps are tied by hand, for u = T-1 ... 0:
        g_u      = l_u + fed[u+1] * (xi_{u+1} + g_{u+1})        (g_{T-1} = l_{T-1}; xi_u: d/dx of step u's STACK on the feedback channels)
        the stack of step u receives g_u on its head output and the state cotangents of step u+1
        dx_u     = the stack's d/dx, plus g_u on the feedback channels where (u, b) is unfed, zero there where it is fed
    Zero initial state.  Returns dict(dx, params, g (T,B,O,H,W))."""
    L = CM.num_layers_of(params)
    B, T, C, H, W = x.shape
    P = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    w, b = P["conv.weight"], P["conv.bias"]
    O = w.shape[0]
    fed = fed_mask(fed, B, T)
    hs = [torch.zeros(B, P[f"layers.{i}.conv.bias"].shape[0] // 4, H, W, dtype=x.dtype) for i in range(L)]
    cs = [torch.zeros_like(h) for h in hs]
    steps, p_prev = [], None
    for t in range(T):
        x_t = x[:, t].detach()
        if bool(fed[:, t].any()):
            x_t = torch.cat([x_t[:, :C - O], torch.where(fed[:, t].view(B, 1, 1, 1), CLM.round_et(p_prev, storage), x_t[:, C - O:])], dim=1)
        x_in = x_t.clone().requires_grad_(True)
        h_in = [h.detach().clone().requires_grad_(True) for h in hs]
        c_in = [c.detach().clone().requires_grad_(True) for c in cs]
        inp, h_out, c_out = x_in, [], []
        for i in range(L):
            h, c = CM.cell_forward(inp, h_in[i], c_in[i], P[f"layers.{i}.conv.weight"], P[f"layers.{i}.conv.bias"], cyclic)
            h_out.append(h); c_out.append(c); inp = h
        d = F.conv2d(h_out[-1], w, b)
        p_prev = (d + x_in[:, C - O:]).detach()
        steps.append((x_in, h_in, c_in, h_out, c_out, d))
        hs, cs = [h.detach() for h in h_out], [c.detach() for c in c_out]
    l = torch.zeros(T, B, O, H, W, dtype=x.dtype)
    if dseq is not None:
        l += dseq.to(x.dtype).view(B, T, O, H, W).transpose(0, 1)
    if dpred is not None:
        l[T - 1] += dpred.to(x.dtype)
    g = torch.zeros_like(l)
    dx = torch.zeros_like(x)
    names = list(P)
    gp = {k: torch.zeros_like(v) for k, v in P.items()}
    dh = [torch.zeros_like(h) for h in hs]
    dc = [torch.zeros_like(c) for c in cs]
    carry = torch.zeros(B, O, H, W, dtype=x.dtype)          # fed[u+1] * (xi_{u+1} + g_{u+1})
    for u in range(T - 1, -1, -1):
        x_in, h_in, c_in, h_out, c_out, d = steps[u]
        g[u] = l[u] + carry
        outs = [d] + h_out + c_out
        cots = [g[u]] + dh + dc
        ins = [x_in] + h_in + c_in + [P[k] for k in names]
        got = torch.autograd.grad(outs, ins, cots, allow_unused=True)
        got = [torch.zeros_like(i) if v is None else v for i, v in zip(ins, got)]
        gx, dh, dc = got[0], list(got[1:1 + L]), list(got[1 + L:1 + 2 * L])
        for k, v in zip(names, got[1 + 2 * L:]):
            gp[k] += v
        m = fed[:, u].view(B, 1, 1, 1)
        xi = gx[:, C - O:]
        carry = torch.where(m, xi + g[u], torch.zeros_like(xi))
        dx[:, u] = gx
        dx[:, u, C - O:] = torch.where(m, torch.zeros_like(xi), xi + g[u])
    return dict(dx=dx, params=gp, g=g)


# ------------------------------------------------------------------ the cases of tests/test_gpu_residual.py, and their references
# closed_loop_model.CASES (B = 2, T = 4, 13 x 37: thin / single / all folded with k = 5, wide plain with c0 = 37, O = 3) and
#   chv128   the top layer has 72 hidden channels: Chp = 80 (f32) / 96 (bf16) > 64, so the CHV = 128 head instances run
#   longrow  W = 261 > 256: a thread of the feedback kernel's row pass takes a second pixel
CASES = dict(CLM.CASES)
CASES["chv128"] = dict(C=5, O=2, hidden=[8, 72], ks=[3, 3], **CLM.GRID)
CASES["longrow"] = dict(C=4, O=2, hidden=[8], ks=[3], B=2, T=3, H=5, W=261)
# A mask for B = 2, T = 4: a mixed step, a full step, a step nobody is fed at behind F
MASK = torch.tensor([[0, 1, 1, 0],
                     [0, 0, 1, 0]], dtype=torch.bool)
# Weights: the oracle's synthetic ones AS THEY ARE.  rollout_model.case_params scales layer 0's feedback columns by 60 so that the fed
# term stands out of a head that starts afresh every step; here the skip term carries the whole cotangent of every later step,
# and with the plain weights the three gradients -- residual, residual without the skip term, non-residual -- are already 20 to
# 600 gates apart in every parameter of every case (tests/test_residual_cpu.py asserts it).  The scaled columns also put the bf16
# storage-rounding floor of layer 0's weight gradient AT the 2e-2 gate: the EXISTING non-residual teacher-forced trainer step on
# the `thin` case with those weights measures rel-L2 1.8e-2 ... 2.5e-2 over eight batch draws, so a gate held
# there would measure the draw.  Data and cotangents (with a mean): rollout_model.case_data.
def case_params(c, dtype=torch.float32, seed=3):
    from oracle import convlstm_oracle as O
    return O.synth_params(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=c["O"], seed=seed, dtype=dtype)


case_data = RM.case_data
_REF = {}


def _kw(d, with_state):
    kw = dict(dpred=d["dpred"], dseq=d["dseq"])
    if with_state:
        kw.update(h0=[t.double() for t in d["h0"]], c0=[t.double() for t in d["c0"]], dhT=d["dhT"], dcT=d["dcT"])
    return kw


def _key(fed):
    return fed if fed is None or isinstance(fed, int) else tuple(map(tuple, torch.as_tensor(fed).int().tolist()))


def reference(case: str, cyclic: bool, fed, with_state: bool = False):
    """(residual gradients, the same with the skip term dropped, the non-residual model's) of a case in f64, fed values rounded to
    f32 (the f32 model that both storage types are held against); computed once"""
    key = (case, cyclic, _key(fed), with_state)
    if key not in _REF:
        c = CASES[case]
        d, p = case_data(c), case_params(c, torch.float64)
        kw = _kw(d, with_state)
        m = fed_mask(fed, c["B"], c["T"])
        X = d["X"].double()
        _REF[key] = (grads(X, p, m, cyclic, "f32", **kw), grads(X, p, m, cyclic, "f32", skip=False, **kw),
                     SM.grads(X, p, m, cyclic, "f32", **kw))
    return _REF[key]


def separation(a, b):
    """per parameter: (max-abs distance of two gradients in f32 gates, their rel-L2 distance in bf16 gates), a the reference"""
    out = {}
    for k, g in a["params"].items():
        t = b["params"][k]
        out[k] = (float((g - t).abs().max()) / RM.F32_GATE(g), float((g - t).norm() / g.norm()) / RM.BF16_GATE)
    return out
