"""CPU model of the CLOSED-LOOP forward pass (TEST INFRASTRUCTURE ONLY): the reference's stack
(model.py:253-274, through tests/cyclic_model.py, whose ``cyclic=False`` is the oracle's own arithmetic) with one rule added --

    for every step t >= free_from:   x[:, t, C-O:] = round_ET( head(h^{L-1} after step t-1) )

``round_ET`` is one round-to-nearest-even to the storage type ("f32", "bf16"; None: no rounding, the exact-arithmetic model
for f64 runs).  Step 0 sees the head of the initial state, so ``free_from = 0`` needs one.  ``free_from >= T`` (or None) is the
open-loop model."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

import cyclic_model as CM


def round_et(p: torch.Tensor, storage: Optional[str]) -> torch.Tensor:
    if storage is None:
        return p
    et = {"f32": torch.float32, "bf16": torch.bfloat16}[storage]
    return p.to(et).to(p.dtype)            # torch rounds to nearest even


def forward(x, params, free_from: Optional[int] = None, cyclic: bool = False, storage: Optional[str] = "f32",
            h0: Optional[List[torch.Tensor]] = None, c0: Optional[List[torch.Tensor]] = None):
    """x (B,T,C,H,W) -> dict(pred (B,O,H,W), seq (B,T*O,H,W), hs, cs, x_fed (B,T,C,H,W): x as the model saw it)"""
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
            x_t = torch.cat([x_t[:, :C - O], round_et(F.conv2d(hs[-1], w, b), storage)], dim=1)
        fed.append(x_t)
        for i in range(L):
            hs[i], cs[i] = CM.cell_forward(x_t, hs[i], cs[i], params[f"layers.{i}.conv.weight"], params[f"layers.{i}.conv.bias"], cyclic)
            x_t = hs[i]
        outs.append(F.conv2d(hs[-1], w, b))
    return dict(pred=outs[-1], seq=torch.cat(outs, dim=1), hs=hs, cs=cs, x_fed=torch.stack(fed, dim=1))


# The shapes of tests/test_gpu_closed_loop.py: B = 2 (image index t*B + b), T = 4, a ragged 13 x 37 grid (H no multiple of 8,
# W no multiple of 16 or 32, W >= P).  O = head outputs = feedback channels, the last O of C.
#   thin    folded input (C = 4, k = 5 folds in f32 and bf16), O = 1
#   wide    plain input: c0 = 37 straddles a 16-byte group in both storage types, O = 3
#   single  a one-layer stack on the folded input
#   all     O == C: every input channel is fed back (folded)
GRID = dict(B=2, T=4, H=13, W=37)
CASES = {
    "thin": dict(C=4, O=1, hidden=[16, 8], ks=[5, 3], **GRID),
    "wide": dict(C=40, O=3, hidden=[16, 8], ks=[5, 3], **GRID),
    "single": dict(C=4, O=1, hidden=[16], ks=[5], **GRID),
    "all": dict(C=3, O=3, hidden=[16, 8], ks=[5, 3], **GRID),
}
FOLDED = {"thin": True, "wide": False, "single": True, "all": True}
