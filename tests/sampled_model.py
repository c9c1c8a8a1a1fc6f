"""CPU model of SCHEDULED SAMPLING (TEST INFRASTRUCTURE ONLY): ``rollout_model.forward`` with the scalar
``free_from`` taken to a mask ``fed`` of shape (B, T),

    for every (b, t) with fed[b, t]:   x[b, t, C-O:] = p + (round_ET(p) - p).detach(),    p = head(h^{L-1}[b] after step t-1)

and every other image of every step sees ``x`` as given.  The pieces -- the stack, the rounding, the straight-through form,
the cases' weights and data -- are those of tests/closed_loop_model.py and tests/rollout_model.py, by import:
``fed[b, t] = (t >= s)`` is ``rollout_model`` at ``free_from = s`` exactly, values and gradients (tests/test_sampled_cpu.py)."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

import closed_loop_model as CLM
import cyclic_model as CM
import rollout_model as RM


def suffix(B: int, T: int, s: int) -> torch.Tensor:
    """the mask of free_from = s: (B, T) bool, fed[b, t] = (t >= s)"""
    return (torch.arange(T) >= s).view(1, T).expand(B, T).clone()


def forward(x, params, fed=None, cyclic: bool = False, storage: Optional[str] = "f32",
            h0: Optional[List[torch.Tensor]] = None, c0: Optional[List[torch.Tensor]] = None):
    """x (B,T,C,H,W), fed (B,T) bool or None (nothing fed) -> dict(pred, seq, hs, cs, x_fed) as rollout_model.forward returns them"""
    L = CM.num_layers_of(params)
    B, T, C, H, W = x.shape
    w, b = params["conv.weight"], params["conv.bias"]
    O = w.shape[0]
    fed = torch.zeros(B, T, dtype=torch.bool) if fed is None else torch.as_tensor(fed).bool()
    if tuple(fed.shape) != (B, T) or O > C or (bool(fed[:, 0].any()) and h0 is None):
        raise ValueError("scheduled sampling: fed is (B, T), O <= C, and step 0 is fed only from a given state")
    hs, cs = [], []
    for i in range(L):
        ch = params[f"layers.{i}.conv.bias"].shape[0] // 4
        hs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if h0 is None else h0[i])
        cs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if c0 is None else c0[i])
    outs, seen = [], []
    for t in range(T):
        x_t = x[:, t]
        if bool(fed[:, t].any()):
            p = F.conv2d(hs[-1], w, b)
            val = p + (CLM.round_et(p, storage) - p).detach()
            x_t = torch.cat([x_t[:, :C - O], torch.where(fed[:, t].view(B, 1, 1, 1), val, x_t[:, C - O:])], dim=1)
        seen.append(x_t)
        for i in range(L):
            hs[i], cs[i] = CM.cell_forward(x_t, hs[i], cs[i], params[f"layers.{i}.conv.weight"], params[f"layers.{i}.conv.bias"], cyclic)
            x_t = hs[i]
        outs.append(F.conv2d(hs[-1], w, b))
    return dict(pred=outs[-1], seq=torch.cat(outs, dim=1), hs=hs, cs=cs, x_fed=torch.stack(seen, dim=1))


def grads(x, params, fed, cyclic, storage, dpred=None, dseq=None, h0=None, c0=None, dhT=None, dcT=None):
    """rollout_model.grads under a mask: every gradient of <pred, dpred> + <seq, dseq> + sum <h_T, dhT> + sum <c_T, dcT>"""
    x = x.detach().clone().requires_grad_(True)
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    st = {}
    if h0 is not None:
        st = dict(h0=[t.detach().clone().requires_grad_(True) for t in h0], c0=[t.detach().clone().requires_grad_(True) for t in c0])
    r = forward(x, p, fed, cyclic, storage, **st)
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


# ------------------------------------------------------------------ the cases of tests/test_gpu_sampled.py, and their references
# The `thin` (folded, O = 1) and `wide` (plain, c0 = 37, O = 3) stacks of closed_loop_model.CASES at B = 3, T = 5 on the same
# 13 x 37 grid: 481 pixels per image, so the backward launch's 256-thread workgroups straddle image boundaries.  Weights and
# data: rollout_model.case_params / case_data (layer 0's feedback columns scaled by FEED_SCALE).
CASES = {k: {**CLM.CASES[k], "B": 3, "T": 5} for k in ("thin", "wide")}
# columns t0 ... t4 per image: a mixed step (t1), a full-but-one step (t2), an empty step behind F (t3), a re-entry (t4),
# and an image that is never fed
MASK = torch.tensor([[0, 1, 1, 0, 1],
                     [0, 0, 1, 0, 0],
                     [0, 0, 0, 0, 0]], dtype=torch.bool)
# ... and one with step 0 fed, from a given state (forward only)
MASK0 = torch.tensor([[1, 0, 1, 0, 1],
                      [0, 1, 0, 0, 0],
                      [1, 1, 0, 0, 1]], dtype=torch.bool)

_REF = {}


def _kw(d, with_state):
    kw = dict(dpred=d["dpred"], dseq=d["dseq"])
    if with_state:
        kw.update(h0=[t.double() for t in d["h0"]], c0=[t.double() for t in d["c0"]], dhT=d["dhT"], dcT=d["dcT"])
    return kw


def reference(case: str, cyclic: bool, with_state: bool = False):
    """(masked gradients under MASK, teacher-forced gradients on the same x_fed, full roll-out gradients from F = 1) of a case
    in f64, fed values rounded to f32; computed once"""
    key = (case, cyclic, with_state)
    if key not in _REF:
        c = CASES[case]
        d, p = RM.case_data(c), RM.case_params(c, torch.float64)
        kw = _kw(d, with_state)
        sm = grads(d["X"].double(), p, MASK, cyclic, "f32", **kw)
        tf = grads(sm["x_fed"], p, None, cyclic, "f32", **kw)
        ro = RM.grads(d["X"].double(), p, 1, cyclic, "f32", **kw)
        _REF[key] = (sm, tf, ro)
    return _REF[key]
