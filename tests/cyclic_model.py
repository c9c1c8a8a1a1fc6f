"""CPU model of the ConvLSTM with CYCLIC LONGITUDE (TEST INFRASTRUCTURE ONLY): the reference's cell and stack
(model.py:216-231, 253-274) with one change -- the gate convolution pads its input circularly in x and with zeros in y:

    F.pad(cat, (p, p, 0, 0), mode="circular")   then   conv2d(padding=(p, 0))

so column 0 and column W-1 are neighbours and rows keep the reference's zero padding.  Parameters are the dict of
oracle/convlstm_oracle.py (keys of the reference ``state_dict``); runs in f32 or f64 under torch autograd.  With
``cyclic=False`` it is the oracle's own arithmetic."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F


def num_layers_of(params) -> int:
    n = 0
    while f"layers.{n}.conv.weight" in params:
        n += 1
    return n


def cell_forward(x, h, c, weight, bias, cyclic: bool = True):
    """model.py:216-231 with the padding of the gate convolution as the only difference"""
    ch = h.shape[1]
    p = weight.shape[-1] // 2
    cat = torch.cat([x, h], dim=1)                                       # model.py:219
    if cyclic and p > 0:
        gates = F.conv2d(F.pad(cat, (p, p, 0, 0), mode="circular"), weight, bias, padding=(p, 0))
    else:
        gates = F.conv2d(cat, weight, bias, padding=p)                   # model.py:220
    gi, gf, gg, go = torch.split(gates, ch, dim=1)                       # model.py:221
    gi, gf, gg, go = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
    c_new = c * gf + gi * gg                                             # model.py:228
    return go * torch.tanh(c_new), c_new                                 # model.py:229


def forward(x, params, cyclic: bool = True, return_sequence: bool = False, return_states: bool = False,
            h0: Optional[List[torch.Tensor]] = None, c0: Optional[List[torch.Tensor]] = None):
    """model.py:253-274.  x (B,T,C,H,W) -> pred (B,O,H,W) [, seq (B,T*O,H,W)] [, hs, cs]"""
    L = num_layers_of(params)
    B, T, _, H, W = x.shape
    hs, cs = [], []
    for i in range(L):
        ch = params[f"layers.{i}.conv.bias"].shape[0] // 4
        hs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if h0 is None else h0[i])
        cs.append(torch.zeros(B, ch, H, W, dtype=x.dtype) if c0 is None else c0[i])
    outs = []
    for t in range(T):
        x_t = x[:, t]
        for i in range(L):
            hs[i], cs[i] = cell_forward(x_t, hs[i], cs[i], params[f"layers.{i}.conv.weight"], params[f"layers.{i}.conv.bias"], cyclic)
            x_t = hs[i]
        if return_sequence:
            outs.append(F.conv2d(hs[-1], params["conv.weight"], params["conv.bias"]))
    res = [F.conv2d(hs[-1], params["conv.weight"], params["conv.bias"])]
    if return_sequence:
        res.append(torch.cat(outs, dim=1))
    if return_states:
        res += [hs, cs]
    return tuple(res) if len(res) > 1 else res[0]


# The shapes of tests/test_gpu_cyclic.py: the smallest at which the wrap can go wrong.  slack = roundup(W, 32) - W columns
# between the interior and the right-hand halo of the slab; P = max k // 2.
#   A  slack 12 >= P = 2: the wrapped dG columns lie wholly in the slack the weight gradient walks; layer 0 folded
#   B  no slack; three layers: the forward wavefront and the BPTT merges are live
#   C  P = 3 > slack 2: the right-hand halo straddles slack and pad; layer 0 folded, k = 7
#   D  an UNFOLDED input slab, wrapped at the head of the pass (Cin = 32: nint_xfold_pays is 0 for f32 and bf16; the 40
#      channels first drawn fold in both)
#   E  the production width and stack
CASES = {
    "A": dict(C=3, hidden=[16, 8], ks=[5, 3], B=2, T=3, H=9, W=20),
    "B": dict(C=3, hidden=[32, 16, 16], ks=[5, 3, 3], B=2, T=3, H=8, W=32),
    "C": dict(C=4, hidden=[16], ks=[7], B=2, T=3, H=9, W=30),
    "D": dict(C=32, hidden=[16, 16], ks=[3, 3], B=2, T=3, H=8, W=20),
    "E": dict(C=5, hidden=[64, 32, 16], ks=[5, 3, 3], B=1, T=2, H=16, W=144),
}
FOLDED = {"A": True, "B": True, "C": True, "D": False, "E": True}      # layer 0, both storage types (nint_xfold_pays)
