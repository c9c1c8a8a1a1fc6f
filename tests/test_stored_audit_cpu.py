"""The comparators of oracle/stored_audit.py have teeth (CPU only, no GPU).

A synthetic "kernel output" is built on the CPU for two shapes: the f64 reference passed through exactly the roundings
the error model documents (bf16 storage of gates / h / dG / dx / the transient dh pieces, f32 c and dc), with the
convolutions accumulated in f32 by torch's CPU kernels (another order than the GPU's).  It must pass the audit; each
mutation below is a plausible kernel bug and must fail it:

  1. one output pixel at a tile edge (row 8k-1, column 31) taken from its neighbour;
  2. one 16-column block of one tile taken from the wrong gate;
  3. one tap x one channel chunk dropped from one pixel's pre-activation;
  4. one bf16 value moved by 2 ulps where the bound is tightest;
  5. one halo or padding element set nonzero;
  6. dc of one pixel taken one BPTT step late;
  7. one wave-4 dh piece missing.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import convlstm_oracle as O
from oracle import stored_audit as SA

# (C, hidden, ks, xfold of layer 0, B, T, H, W): a bench-like first layer (62 channels folded, hidden 64, k = 5; 16 x 40
# so that rows 7 / 15 and column 31 are tile edges) and a ragged three-layer stack
SHAPES = {
    "bench-layer": (62, [64], [5], True, 1, 2, 16, 40),
    "ragged-stack": (7, [24, 16, 8], [5, 3, 3], False, 2, 3, 13, 37),
}


def _et(geo, v):
    return v.to(geo.et).double()


def fake_pass(geo, Ws, bs, X, dh_T, dc_T, has_init=False, h0=None, c0=None, mut=None):
    """CPU emulation of nint_seq_fwd + nint_seq_bwd with the documented roundings.  X (T*B, Cx, H, W).  Returns the dict
    stored_audit.audit reads.  mut: None or (name, args) of one mutation applied inside the emulated arithmetic."""
    mut = mut or (None, None)
    B, T, L = geo.B, geo.T, len(geo.layers)
    sl = lambda t: slice(t * B, (t + 1) * B)
    Wb = [W.float().to(geo.et).float() for W in Ws]
    x = _et(geo, X)
    hs = [torch.zeros((T + 1) * B, ly.Ch, geo.H, geo.W, dtype=torch.float64) for ly in geo.layers]
    cs = [torch.zeros((T + 1) * B, ly.Ch, geo.H, geo.W, dtype=torch.float64) for ly in geo.layers]
    gs = [torch.zeros(T * B, 4 * ly.Ch, geo.H, geo.W, dtype=torch.float64) for ly in geo.layers]
    if has_init:
        for l in range(L):
            hs[l][:B], cs[l][:B] = _et(geo, h0[l]), c0[l].float().double()
    for t in range(T):
        for l in range(L):
            ly = geo.layers[l]
            xin = x[sl(t)] if l == 0 else hs[l - 1][sl(t + 1)]
            cat = torch.cat([xin, hs[l][sl(t)]], dim=1).float()
            z = F.conv2d(cat, Wb[l], bs[l].float(), padding=ly.k // 2)          # f32 accumulation, torch's order
            if mut[0] == "drop_chunk" and (l, t) == mut[1][:2]:
                _, _, n, y, xx, ky, kx, c0_, c1_ = mut[1]
                p = ly.k // 2
                z[n, :, y, xx] -= (Wb[l][:, c0_:c1_, ky, kx] * cat[n, c0_:c1_, y + ky - p, xx + kx - p]).sum(dim=1)
            Ch = ly.Ch
            gi, gf, gg, go = torch.sigmoid(z[:, :Ch]), torch.sigmoid(z[:, Ch:2 * Ch]), torch.tanh(z[:, 2 * Ch:3 * Ch]), torch.sigmoid(z[:, 3 * Ch:])
            c = cs[l][sl(t)].float() * gf + gi * gg
            h = go * torch.tanh(c)
            gs[l][sl(t)] = _et(geo, torch.cat([gi, gf, gg, go], dim=1))
            cs[l][sl(t + 1)] = c.double()
            hs[l][sl(t + 1)] = _et(geo, h)
    # backward: classic steps, except layer 0, whose dh arrives in two stored pieces (wave 4)
    dG = [torch.zeros_like(g) for g in gs]
    dc = [torch.zeros(B, ly.Ch, geo.H, geo.W) if dc_T[l] is None else dc_T[l].float().clone() for l, ly in enumerate(geo.layers)]
    dx = torch.zeros(T * B, geo.layers[0].Cx, geo.H, geo.W, dtype=torch.float64)
    late = None

    def dgrad(l, t):
        ly = geo.layers[l]
        return torch.nn.grad.conv2d_input((B, ly.Cx + ly.Ch, geo.H, geo.W), Wb[l], dG[l][sl(t)].float(), padding=ly.k // 2)

    for t in range(T - 1, -1, -1):
        for l in range(L - 1, -1, -1):
            ly = geo.layers[l]
            ph = (torch.zeros(B, ly.Ch, geo.H, geo.W) if dh_T[l] is None else _et(geo, dh_T[l]).float()) if t == T - 1 \
                else dgrad(l, t + 1)[:, -ly.Ch:]
            px = dgrad(l + 1, t)[:, :geo.layers[l + 1].Cx] if l < L - 1 else torch.zeros_like(ph)
            if l == 0 and L > 1:
                if mut[0] == "drop_piece" and t == mut[1]:
                    px = torch.zeros_like(px)
                dh = _et(geo, ph).float() + _et(geo, px).float()
            else:
                dh = _et(geo, _et(geo, ph).float() + px).float()
            g = gs[l][sl(t)].float()
            Ch = ly.Ch
            gi, gf, gg, go = g[:, :Ch], g[:, Ch:2 * Ch], g[:, 2 * Ch:3 * Ch], g[:, 3 * Ch:]
            cp, cn = cs[l][sl(t)].float(), cs[l][sl(t + 1)].float()
            dcv = dc[l]
            if mut[0] == "dc_late" and (l, t) == mut[1][:2]:
                _, _, n, y, xx = mut[1]
                dcv = dcv.clone()
                dcv[n, :, y, xx] = late[n, :, y, xx]
            if mut[0] == "dc_late" and l == mut[1][0] and t == mut[1][1] + 1:
                late = dc[l].clone()
            tc = torch.tanh(cn)
            dct = dcv + dh * go * (1 - tc * tc)
            d_o = dh * tc
            dG[l][sl(t)] = _et(geo, torch.cat([dct * gg * gi * (1 - gi), dct * cp * gf * (1 - gf), dct * gi * (1 - gg * gg),
                                                d_o * go * (1 - go)], dim=1))
            dc[l] = dct * gf
        ly0 = geo.layers[0]
        v = dgrad(0, t)[:, :ly0.Cx]
        if ly0.xfold:
            acc = torch.zeros_like(v)
            for kx in range(ly0.k):
                m = torch.zeros_like(Wb[0])
                m[..., kx] = 1
                acc += _et(geo, torch.nn.grad.conv2d_input((B, ly0.Cx + ly0.Ch, geo.H, geo.W), Wb[0] * m, dG[0][sl(t)].float(),
                                                           padding=ly0.k // 2)[:, :ly0.Cx]).float()
            dx[sl(t)] = acc.double()
        else:
            dx[sl(t)] = _et(geo, v)
    dh_fin = [_et(geo, dgrad(l, 0)[:, -geo.layers[l].Ch:]) for l in range(L)]
    raw = {"xs": SA.write_xs(geo, x)}
    for l, ly in enumerate(geo.layers):
        raw[f"h{l}"] = SA.write_halo(geo, hs[l], ly.Chp)
        raw[f"dG{l}"] = SA.write_dG(geo, l, dG[l])
        raw[f"gates{l}"] = SA.write_gates(geo, l, gs[l])
    return {"x": x, "h": hs, "c": cs, "gates": gs, "dG": dG, "dx": dx, "dh_fin": dh_fin,
            "dc_fin": [d.double() for d in dc], "raw": raw}


def _setup(name, dtype, seed=0):
    C, hidden, ks, xfold, B, T, H, W = SHAPES[name]
    L = len(hidden)
    geo = SA.Geo.make(B, T, H, W, [(C if l == 0 else hidden[l - 1], hidden[l], ks[l], xfold and l == 0) for l in range(L)],
                      2 if dtype == "bf16" else 4)
    p = O.synth_params(C, hidden, ks, L, seed=seed)
    Ws = [p[f"layers.{l}.conv.weight"] for l in range(L)]
    bs = [p[f"layers.{l}.conv.bias"] for l in range(L)]
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(T * B, C, H, W, generator=g)
    dh_T = [0.1 * torch.randn(B, h, H, W, generator=g) for h in hidden]
    dc_T = [0.1 * torch.randn(B, h, H, W, generator=g) for h in hidden]
    h0 = [0.5 * torch.randn(B, h, H, W, generator=g) for h in hidden]
    c0 = [torch.randn(B, h, H, W, generator=g) for h in hidden]
    dh_T = [_et(geo, d).float() for d in dh_T]
    return geo, Ws, bs, X, dh_T, dc_T, h0, c0


def _run(name, dtype, mut=None, has_init=False, st_edit=None):
    geo, Ws, bs, X, dh_T, dc_T, h0, c0 = _setup(name, dtype)
    st = fake_pass(geo, Ws, bs, X, dh_T, dc_T, has_init, h0, c0, mut)
    if st_edit:
        st_edit(geo, st)
    return SA.audit(geo, Ws, bs, st, dh_T, dc_T, has_init), geo, st


def _fmt(w):
    return "  ".join(f"{k} {v:.3f}" for k, v in sorted(w.items()))


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_faithful_synthetic_output_passes(name, dtype):
    for has_init in (False, True):
        w, geo, st = _run(name, dtype, has_init=has_init)
        print(f"  {name} {dtype} has_init={has_init}: max err/bound  {_fmt(w)}")
        assert set(w) >= {"gates", "c", "h", "dG", "dx"}
        assert max(w.values()) <= 1.0, w
        assert SA.check_padding(geo, st["raw"]) == []


def _tile_edge(geo, st):
    g = st["gates"][0]
    g[0, :, 7, 31] = g[0, :, 7, 32]


def _wrong_gate(geo, st):
    g, Ch = st["gates"][0], geo.layers[0].Ch
    g[0, Ch:Ch + 16, 8:16, 0:16] = g[0, 0:16, 8:16, 0:16]            # block 0 of gate f in tile (1, 0) holds gate i


def _two_ulps(W0, b0, geo, st):
    """the element whose bound is smallest against its ulp, moved by two bf16 ulps"""
    B = geo.B
    res = SA.fwd_launch(geo, 0, st["x"][:B], None, None, W0, b0)
    ref, bound = res["gates"]
    stored = st["gates"][0][:B]
    ulp = 2 * SA.halfulp(stored.abs(), geo.u_et)
    i = int(torch.argmin(torch.where(stored != 0, bound / ulp, torch.full_like(bound, float("inf")))))
    flat = stored.reshape(-1)
    bits = flat[i].to(torch.bfloat16).view(torch.int16) + 2
    flat[i] = bits.view(torch.bfloat16).double()


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_every_mutation_fails_the_audit(name, dtype):
    """f32 storage has no storage rounding: its bound is the f32 arithmetic alone (gamma_n and the activations), and the
    same mutations fail it -- except 4, which is about a bf16 rounding (an f32 stash holds the register itself)."""
    geo, Ws, bs, X, dh_T, dc_T, h0, c0 = _setup(name, dtype)
    L, T = len(geo.layers), geo.T
    ly = geo.layers[0]
    chunk = (ly.Cx, ly.Cx + min(geo.kc, ly.Ch))                        # one K-step of the h source (32 bf16 / 16 f32 channels)
    cases = {
        "1 tile-edge pixel from its neighbour": (None, _tile_edge, "gates"),
        "2 16-column block from the wrong gate": (None, _wrong_gate, "gates"),
        "3 one tap x channel chunk dropped": (("drop_chunk", (0, 1, 0, 6, 20, 0, 2) + chunk), None, "gates"),
        "4 one bf16 value moved by 2 ulps": (None, functools.partial(_two_ulps, Ws[0], bs[0]), "gates"),
        "6 dc of one pixel one BPTT step late": (("dc_late", (0, T - 2, 0, 5, 9)), None, "dG"),
    }
    if L > 1:
        cases["7 a wave-4 dh piece missing"] = (("drop_piece", T - 2), None, "dG")
    if dtype == "f32":
        del cases["4 one bf16 value moved by 2 ulps"]
    for label, (mut, edit, kind) in cases.items():
        w, _, _ = _run(name, dtype, mut=mut, st_edit=edit)
        print(f"  {name} {dtype} mutation {label}: {kind} max err/bound {w[kind]:.2f}   ({_fmt(w)})")
        assert w[kind] > 1.0, (name, dtype, label, w)
    # 5: one halo element of h and one channel-padding column of dG set nonzero
    _, geo, st = _run(name, dtype)
    for key, off in (("h0", 0), ("dG0", None)):
        raw = copy.deepcopy(st["raw"])
        b = raw[key].view(torch.int16 if geo.es == 2 else torch.int32)
        if off is None:                                                 # first pixel of the interior, last padded column
            ly = geo.layers[0]
            Gc = 4 * ly.Ch16
            pix = geo.P * geo.Wh + geo.P
            off = pix * Gc + (Gc - 1) if ly.Ch16 > ly.Ch else pix * Gc - 1     # (no padded column: a ring element)
        b[off] = 0x3f80 if geo.es == 2 else 0x3f800000                  # 1.0
        bad = SA.check_padding(geo, raw)
        print(f"  {name} {dtype} mutation 5 nonzero {key} padding: {bad}")
        assert bad, (name, key)
