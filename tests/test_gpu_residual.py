"""GPU: the residual head -- ``ConvLSTM(feedback=True, residual=True)``: p_t = x_t[feedback channels] + head(h_t),
the _res head entries (nint_head_base), nint_head_feedback_res / _bwd_res, nint_seq_fwd_residual / nint_seq_bwd_rollout_residual.

Shapes: residual_model.CASES -- closed_loop_model.CASES (B = 2, T = 4, 13 x 37: thin / single / all folded with k = 5, wide plain
with c0 = 37 and O = 3: an odd first channel for the bf16 dword pairing and a span across a 16-byte group), `chv128` (72 top
channels: the CHV = 128 instances) and `longrow` (W = 261: a thread's second pixel in the feedback kernel's row pass); f32 and
bf16, zero padding and cyclic longitude.
References: the twin entries and compositions of existing entries (bit for bit), the library's own open-loop pass on the fed
input (bit for bit), tests/residual_model.py in f64 under CPU autograd at the standing gates of tests/test_gpu_parity.py /
test_gpu_rollout.py -- f32: outputs rtol 1e-4 / atol 1e-5, gradients <= 1e-3 * max|grad| + 1e-6; bf16: rel-L2 <= 2e-2 against
the f32 model, or twice the storage-rounding floor of the EXISTING non-residual teacher-forced path on the same fed input where
that floor is above the gate (the rule of tests/test_gpu_rollout.py).  tests/test_residual_cpu.py asserts on the CPU model that
a backward pass without the skip term, or of the non-residual head, is tens of gates away in every parameter."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_model as CLM
import residual_model as RES
import rollout_model as RM
import sampled_model as SM
import test_gpu_memory_contract as MC
from test_gpu_closed_loop import pkg                                  # noqa: F401  (the fixture)
from test_gpu_parity import assert_bf16, assert_close_grad, assert_close_out
from test_gpu_rollout import _grads_on_device, _ref_grad, _rel

pytestmark = pytest.mark.gpu
BOTH = ("f32", "bf16")
CYC = dict(argvalues=[False, True], ids=["zero-pad", "cyclic"])
FOLDED = {**CLM.FOLDED, "chv128": True, "longrow": True}
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


def _lib():
    from nasa_niswan_amd import _lib as L
    return L, L.load()


# ====================================================================== the C entries, alone
# (name, Cx, O, Ch, k of a folded slab or 0, H, W)
ENTRY = [("thin-folded", 4, 1, 8, 5, 13, 37), ("plain-straddle", 40, 3, 8, 0, 13, 37), ("all-folded", 3, 3, 8, 5, 13, 37),
         ("chv-128", 5, 2, 72, 3, 13, 37), ("long-row", 4, 2, 8, 3, 3, 261)]
ENTRY_IDS = [e[0] for e in ENTRY]
N_ = 2


class Setup:
    """one head problem: a top-layer h slab of 2N images (the one-step entries read images [1, 1 + N); a sequence entry with B
    images per step reads from image B on), the head, and an input slab of two steps of N images packed from `src` (B = N, T = 2:
    step 0 the base images [0, N), step 1 the images [N, 2N))"""

    def __init__(self, lib, L, ex, dt, Cx, O_, Ch, k, cyc, H, W, seed=7):
        from nasa_niswan_amd._lib import stream_ptr
        self.lib, self.L, self.ex, self.dt, self.Cx, self.O, self.Ch, self.k, self.cyc, self.H, self.W = lib, L, ex, dt, Cx, O_, Ch, k, cyc, H, W
        self.es, self.et = (2, torch.bfloat16) if dt == 1 else (4, torch.float32)
        kc = lib.nint_kc(dt)
        rup = lambda a, b: (a + b - 1) // b * b
        self.g = MC._geom(lib, H, W, 2)
        self.Chp, self.Cxp, self.c0 = rup(Ch, kc), rup((k or 1) * Cx, kc), Cx - O_
        self.st = stream_ptr()
        gen = torch.Generator().manual_seed(seed)
        self.gen = gen
        g = self.g
        self.h = ex.copy(torch.randn(2 * N_ * g.Hh * g.Wh * self.Chp, generator=gen).to(self.et))     # junk in halo and pad channels too
        self.w = ex.copy(torch.randn(O_, Ch, generator=gen))
        self.b = ex.copy(torch.randn(O_, generator=gen))
        self.src = torch.randn(N_, 2, Cx, H, W, generator=gen)
        self.xs = self.pack(self.src)

    def pack(self, src):
        lib, g = self.lib, self.g
        x = self.ex.copy(src.contiguous())
        slab = self.ex.zeros(2 * N_ * g.Hh * g.Wh * self.Cxp * self.es, torch.uint8)
        if self.k:
            fn = lib.nint_pack_btchw_xfold_cyclic if self.cyc else lib.nint_pack_btchw_xfold
            assert fn(MC.P(x), MC.P(slab), N_, 2, self.Cx, self.k, self.Cxp, C.byref(g), self.dt, self.st) == 0
        else:
            assert lib.nint_pack_btchw(MC.P(x), MC.P(slab), N_, 2, self.Cx, self.Cxp, C.byref(g), self.dt, self.st) == 0
        return slab

    def base(self, xs=None, x_n0=0, null_xs=False):
        hb = self.L.NintHeadBase()
        hb.xs = None if null_xs else (self.xs if xs is None else xs).data_ptr()
        hb.x_n0, hb.Cx, hb.Cxp, hb.c0, hb.xfold_k = x_n0, self.Cx, self.Cxp, self.c0, self.k
        return hb

    def stored_base(self, x_n0=0, n=N_):
        """(n, O, H, W) f32: the values the slab holds in the feedback channels (folded: the pixel's own copy) of images from x_n0"""
        Cs = (self.k or 1) * self.Cx
        full = torch.empty(n, Cs, self.H, self.W, device="cuda")
        assert self.lib.nint_unpack_halo(MC.P(self.xs), MC.P(full), x_n0, n, Cs, self.Cxp, C.byref(self.g), self.dt, self.st) == 0
        first = (self.k // 2) * self.Cx + self.c0
        return full[:, first:first + self.O].contiguous()

    def head(self, fn, *tail):
        return fn(MC.P(self.h), 1, N_, self.Ch, self.Chp, self.O, MC.P(self.w), MC.P(self.b), *tail)


def _entry_params(fn):
    fn = pytest.mark.parametrize("cyc", [0, 1], ids=["zero-pad", "cyclic"])(fn)
    fn = pytest.mark.parametrize("dt", [0, 1], ids=BOTH)(fn)
    return pytest.mark.parametrize("name,Cx,O_,Ch,k,H,W", ENTRY, ids=ENTRY_IDS)(fn)


def _spec(L, ex, kind, O_, T=None):
    """default: (1, 1, 0) without weights; huber: a mix with a Huber term and output weights (per (step, output) with T)"""
    sp = L.NintLossSpec()
    if kind == "default":
        sp.mse, sp.l1, sp.huber, sp.delta, sp.ow, sp.now, sp.osum = 1.0, 1.0, 0.0, 1.0, None, 0, 0.0
        return sp, None
    n = O_ * (T or 1)
    ow = ex.copy((0.5 + torch.arange(n, dtype=torch.float32) % 3))
    sp.mse, sp.l1, sp.huber, sp.delta = 0.5, 0.25, 2.0, 0.7
    sp.ow, sp.now, sp.osum = ow.data_ptr(), n, float(ow[:n].double().sum())
    return sp, ow


def _loss_bufs(ex, L, s, n_img):
    H, W = s.H, s.W
    return dict(dpred=ex.empty(n_img * s.O * H * W, torch.float32, slack=0), dh=ex.empty(n_img * H * W * s.Chp, s.et, slack=0),
                loss=ex.empty(L.NINT_LOSS_SPEC_SCRATCH_FLOATS, torch.float32, slack=0), stats=ex.zeros(L.NINT_LOSS_STATS, torch.float64))


def _loss_out(bufs, s, n_img, L):
    return dict(dpred=bufs["dpred"][:n_img * s.O * s.H * s.W].clone(), dh=bufs["dh"][:n_img * s.H * s.W * s.Chp].clone(),
                loss=bufs["loss"][:1].clone(), stats=bufs["stats"][:L.NINT_LOSS_STATS].clone())


@_entry_params
def test_without_a_base_every_res_entry_is_its_twin(pkg, name, Cx, O_, Ch, k, H, W, dt, cyc):
    """base == NULL and base->xs == NULL (feedback launches: base_n0 / pnext_n0 < 0): pred, seq, the fused pass's dpred / dh / loss
    / stats, every byte of xs, the dpred slab and dh equal the twin's, bit for bit -- masked and unmasked"""
    L, lib = _lib()
    halo, Hc, Wc = (1, 2), H - 2, W - 5

    def call(ex):
        s = Setup(lib, L, ex, dt, Cx, O_, Ch, k, cyc, H, W)
        g, st = C.byref(s.g), s.st
        res = {}
        for tag, hb in (("null", None), ("null-xs", C.byref(s.base(null_xs=True)))):
            a, b = (ex.empty(N_ * O_ * H * W, torch.float32, slack=0) for _ in range(2))
            assert s.head(lib.nint_head_fwd, MC.P(a), g, dt, st) == 0 and s.head(lib.nint_head_fwd_res, MC.P(b), g, dt, hb, st) == 0
            res[f"fwd.{tag}"] = (a[:N_ * O_ * H * W].clone(), b[:N_ * O_ * H * W].clone())
            # the sequence entries: B = 1, T = N (h slot t + 1 = image 1 + t)
            a, b = (ex.empty(N_ * O_ * H * W, torch.float32, slack=0) for _ in range(2))
            seq_args = (MC.P(s.h), 1, N_, Ch, s.Chp, O_, MC.P(s.w), MC.P(s.b))
            assert lib.nint_head_fwd_seq(*seq_args, MC.P(a), g, dt, st) == 0 and lib.nint_head_fwd_seq_res(*seq_args, MC.P(b), g, dt, hb, st) == 0
            res[f"seq.{tag}"] = (a[:N_ * O_ * H * W].clone(), b[:N_ * O_ * H * W].clone())
            y = ex.copy(torch.randn(N_ * O_ * Hc * Wc, generator=s.gen))
            for kind in ("default", "huber"):
                for sq in (False, True):
                    sp, ow = _spec(L, ex, kind, O_, N_ if sq else None)
                    outs = []
                    for fn, extra in ((lib.nint_head_loss_seq_fused_spec if sq else lib.nint_head_loss_fused_spec, ()),
                                      (lib.nint_head_loss_seq_fused_res if sq else lib.nint_head_loss_fused_res, (hb,))):
                        bufs = _loss_bufs(ex, L, s, N_)
                        head = seq_args if sq else (MC.P(s.h), 1, N_, Ch, s.Chp, O_, MC.P(s.w), MC.P(s.b))
                        assert fn(*head, MC.P(y), None, 0.0, C.byref(sp), MC.P(bufs["dpred"]), MC.P(bufs["dh"]), MC.P(bufs["loss"]),
                                  MC.P(bufs["stats"]), g, halo[0], halo[1], Hc, Wc, dt, *extra, st) == 0
                        torch.cuda.synchronize()
                        outs.append(_loss_out(bufs, s, N_, L))
                    for key in outs[0]:
                        res[f"loss.{kind}.{int(sq)}.{key}.{tag}"] = (outs[0][key], outs[1][key])
        # the feedback launch: unmasked and masked
        for tag, fed in (("all", None), ("mask", (C.c_uint8 * N_)(0, 1))):
            xa, xb = s.pack(s.src), s.pack(s.src)
            fb = (MC.P(s.h), 1, N_, Ch, s.Chp, O_, MC.P(s.w), MC.P(s.b))
            lay = (N_, Cx, s.Cxp, s.c0, k, cyc)
            if fed is None:
                assert lib.nint_head_feedback(*fb, MC.P(xa), *lay, g, dt, st) == 0
            else:
                assert lib.nint_head_feedback_sel(*fb, MC.P(xa), *lay, fed, g, dt, st) == 0
            assert lib.nint_head_feedback_res(*fb, MC.P(xb), *lay, -1, fed, g, dt, st) == 0
            res[f"feedback.{tag}"] = (xa.clone(), xb.clone())
            # ... and its adjoint on images [1, 1 + N) of dx / dpred / dh
            dx = ex.copy(torch.randn((1 + N_) * H * W * s.Cxp, generator=torch.Generator().manual_seed(5)).to(s.et))
            dp0 = torch.randn((1 + 2 * N_) * O_ * H * W, generator=torch.Generator().manual_seed(6))
            pair = []
            for twin in (True, False):
                dp, dh = ex.copy(dp0.clone()), ex.empty((1 + N_) * H * W * s.Chp, s.et, slack=0)
                args = (MC.P(dx), 1, MC.P(dp), 1, MC.P(dh), 1, N_, Ch, s.Chp, O_, MC.P(s.w), Cx, s.Cxp, s.c0, k, cyc)
                if not twin:
                    assert lib.nint_head_feedback_bwd_res(*args, -1, fed, g, dt, st) == 0
                elif fed is None:
                    assert lib.nint_head_feedback_bwd(*args, g, dt, st) == 0
                else:
                    assert lib.nint_head_feedback_bwd_sel(*args, fed, g, dt, st) == 0
                torch.cuda.synchronize()
                pair.append((dp[:dp0.numel()].clone(), dh[H * W * s.Chp:(1 + N_) * H * W * s.Chp].clone()))
            res[f"fbb.dpred.{tag}"], res[f"fbb.dh.{tag}"] = (pair[0][0], pair[1][0]), (pair[0][1], pair[1][1])
        torch.cuda.synchronize()
        for key, (a, b) in res.items():
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, key)
        return {key: b for key, (a, b) in res.items()}
    MC.both_ways(f"res twins {name}", call)


@_entry_params
def test_head_fwd_res_is_the_twin_plus_the_stored_base(pkg, name, Cx, O_, Ch, k, H, W, dt, cyc):
    """nint_head_fwd_res / nint_head_fwd_seq_res = the twin's f32 result + the slab's base (the pixel's own copy in a folded slab),
    added on the host in f32: bit for bit.  The one-step entry pairs h image 1 + i with xs image x_n0 + i (x_n0 = 0 and N), the
    sequence entry (B = 1, T = N) h slot t + 1 with xs image t"""
    L, lib = _lib()

    def call(ex):
        s = Setup(lib, L, ex, dt, Cx, O_, Ch, k, cyc, H, W)
        g, st, n = C.byref(s.g), s.st, N_ * O_ * H * W
        plain = ex.empty(n, torch.float32, slack=0)
        assert s.head(lib.nint_head_fwd, MC.P(plain), g, dt, st) == 0
        out = {}
        for x_n0 in (0, N_):
            got = ex.empty(n, torch.float32, slack=0)
            assert s.head(lib.nint_head_fwd_res, MC.P(got), g, dt, C.byref(s.base(x_n0=x_n0)), st) == 0
            torch.cuda.synchronize()
            want = plain[:n].view(N_, O_, H, W) + s.stored_base(x_n0)
            assert torch.equal(got[:n].view(N_, O_, H, W), want), (name, x_n0)
            assert not torch.equal(got[:n], plain[:n])
            out[f"fwd.{x_n0}"] = got[:n].clone()
        seq = ex.empty(n, torch.float32, slack=0)
        assert lib.nint_head_fwd_seq_res(MC.P(s.h), 1, N_, Ch, s.Chp, O_, MC.P(s.w), MC.P(s.b), MC.P(seq), g, dt, C.byref(s.base()), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(seq[:n], out["fwd.0"]), name            # (B = 1: plane block t = image t)
        out["seq"] = seq[:n].clone()
        return out
    MC.both_ways(f"head_fwd_res {name}", call)


@_entry_params
def test_fused_res_entries_equal_their_three_launches(pkg, name, Cx, O_, Ch, k, H, W, dt, cyc):
    """nint_head_loss[_seq]_fused_res = nint_head_fwd[_seq]_res -> nint_loss_crop_spec -> nint_head_bwd[_seq] as the twins are held
    to theirs (tests/test_gpu_loss_spec.py): dpred, dh and the f32 loss bit for bit; the eight stats to 1e-14 -- their f64 partial
    sums are folded in another order by the fused pass, for the twin as for this entry (sum Wd y, which cancels, relative to
    sum Wd |y|).  The default spec with and without a cell map (zero weights in it), a Huber mix with output weights; the
    sequence entry at B = 2, T = 1 and B = 1, T = 2 (per-(step, output) weights)"""
    L, lib = _lib()
    halo, Hc, Wc = (1, 2), H - 2, W - 5

    def call(ex):
        s = Setup(lib, L, ex, dt, Cx, O_, Ch, k, cyc, H, W)
        g, st, n = C.byref(s.g), s.st, N_ * O_ * H * W
        hb = C.byref(s.base())
        y = ex.copy(torch.randn(N_ * O_ * Hc * Wc, generator=s.gen))
        wmap = torch.rand(Hc, Wc, generator=s.gen)
        wmap[0, :3] = 0
        wgt = ex.copy(wmap)
        wsum = float(wmap.double().sum())
        out = {}
        for kind, use_map in (("default", False), ("default", True), ("huber", True)):
            for form in ("step", "seq-B2", "seq-T2"):
                B, T = (N_, 1) if form != "seq-T2" else (1, N_)
                sq = form != "step"
                sp, ow = _spec(L, ex, kind, O_, T if sq else None)
                mp = (MC.P(wgt), wsum) if use_map else (None, 0.0)
                head = (MC.P(s.h), B, T, Ch, s.Chp, O_, MC.P(s.w), MC.P(s.b)) if sq else (MC.P(s.h), 1, N_, Ch, s.Chp, O_, MC.P(s.w), MC.P(s.b))
                fused = _loss_bufs(ex, L, s, N_)
                fn = lib.nint_head_loss_seq_fused_res if sq else lib.nint_head_loss_fused_res
                assert fn(*head, MC.P(y), *mp, C.byref(sp), MC.P(fused["dpred"]), MC.P(fused["dh"]), MC.P(fused["loss"]), MC.P(fused["stats"]),
                          g, halo[0], halo[1], Hc, Wc, dt, hb, st) == 0
                three = _loss_bufs(ex, L, s, N_)
                pred = ex.empty(n, torch.float32, slack=0)
                if sq:
                    assert lib.nint_head_fwd_seq_res(*head, MC.P(pred), g, dt, hb, st) == 0
                    # (the loss takes the sequence tensor (B, T*O, H, W) as O' = T*O outputs and writes d loss / d seq in that order)
                    dseq = ex.empty(n, torch.float32, slack=0)
                    assert lib.nint_loss_crop_spec(MC.P(pred), MC.P(y), *mp, C.byref(sp), MC.P(dseq), MC.P(three["loss"]), MC.P(three["stats"]),
                                                   B, T * O_, H, W, halo[0], halo[1], Hc, Wc, st) == 0
                    assert lib.nint_head_bwd_seq(MC.P(s.h), B, T, Ch, s.Chp, O_, MC.P(s.w), MC.P(dseq), None, MC.P(three["dh"]), None, None, g,
                                                 dt, None, 0, st) == 0
                    torch.cuda.synchronize()
                    three["dpred"] = dseq[:n].view(B, T, O_, H, W).transpose(0, 1).contiguous().view(-1)      # image order t*B + b
                else:
                    assert s.head(lib.nint_head_fwd_res, MC.P(pred), g, dt, hb, st) == 0
                    assert lib.nint_loss_crop_spec(MC.P(pred), MC.P(y), *mp, C.byref(sp), MC.P(three["dpred"]), MC.P(three["loss"]),
                                                   MC.P(three["stats"]), N_, O_, H, W, halo[0], halo[1], Hc, Wc, st) == 0
                    assert lib.nint_head_bwd(MC.P(s.h), 1, N_, Ch, s.Chp, O_, MC.P(s.w), MC.P(three["dpred"]), MC.P(three["dh"]), None, None,
                                             g, dt, None, 0, st) == 0
                torch.cuda.synchronize()
                a, b = _loss_out(fused, s, N_, L), _loss_out(three, s, N_, L)
                for key in a:
                    if key != "stats":
                        assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), (name, kind, use_map, form, key)
                    out[f"{kind}.{int(use_map)}.{form}.{key}"] = a[key]
                Wd = (wgt[:Hc * Wc].view(Hc, Wc) if use_map else torch.ones(Hc, Wc, device="cuda")).double()
                q = ow[:T * O_].view(T, O_).double() if ow is not None else torch.ones(T, O_, device="cuda", dtype=torch.float64)
                mags = float((y[:N_ * O_ * Hc * Wc].view(B, T, O_, Hc, Wc).double().abs() * q.view(1, T, O_, 1, 1) * Wd).sum())
                sa, sb = a["stats"].cpu().numpy(), b["stats"].cpu().numpy()
                ref = np.maximum(np.abs(sa), np.abs(sb))
                ref[2] = max(ref[2], mags)
                assert np.isfinite(sa).all() and (np.abs(sa - sb) <= 1e-14 * ref).all(), (name, kind, use_map, form, sa, sb)
                assert sa[4] == sb[4]
                assert float(a["stats"][7]) == 1.0 and bool(torch.isfinite(a["loss"]).all())
        return out
    MC.both_ways(f"fused res {name}", call)


@_entry_params
def test_head_feedback_res_is_head_fwd_res_then_pack(pkg, name, Cx, O_, Ch, k, H, W, dt, cyc):
    """image N + i of xs receives round_ET(dot + base of image i): every byte of the slab equals nint_pack_btchw[_xfold[_cyclic]] of
    the input with nint_head_fwd_res's f32 output in the feedback channels of the fed images -- so the unfed images, the base
    images and every other channel stay; unmasked, a mixed mask, a mask of zeros (no launch)"""
    L, lib = _lib()

    def call(ex):
        s = Setup(lib, L, ex, dt, Cx, O_, Ch, k, cyc, H, W)
        g, st, n = C.byref(s.g), s.st, N_ * O_ * H * W
        pred = ex.empty(n, torch.float32, slack=0)
        assert s.head(lib.nint_head_fwd_res, MC.P(pred), g, dt, C.byref(s.base()), st) == 0
        torch.cuda.synchronize()
        p = pred[:n].view(N_, O_, H, W)
        out = {}
        for tag, fed in (("all", None), ("mixed", [0, 1]), ("none", [0, 0])):
            src2 = s.src.clone().cuda()
            for i in range(N_):
                if fed is None or fed[i]:
                    src2[i, 1, s.c0:] = p[i]
            want = s.pack(src2.cpu())
            got = s.pack(s.src)
            fp = None if fed is None else (C.c_uint8 * N_)(*fed)
            assert s.head(lib.nint_head_feedback_res, MC.P(got), N_, Cx, s.Cxp, s.c0, k, cyc, 0, fp, g, dt, st) == 0
            torch.cuda.synchronize()
            assert torch.equal(got, want), (name, tag)
            assert torch.equal(got, s.xs) == (tag == "none")
            out[tag] = got.clone()
        # ... and it differs from the non-residual launch on the same data
        plain = s.pack(s.src)
        assert s.head(lib.nint_head_feedback, MC.P(plain), N_, Cx, s.Cxp, s.c0, k, cyc, g, dt, st) == 0
        torch.cuda.synchronize()
        assert not torch.equal(plain, out["all"])
        return out
    MC.both_ways(f"head_feedback_res {name}", call)


@_entry_params
def test_head_feedback_bwd_res_is_its_composition(pkg, name, Cx, O_, Ch, k, H, W, dt, cyc):
    """dpred images [1, 1 + N) and dh equal unpack / unfold of the step's dx -> (dpred + xi) + dpred of images [1 + N, 1 + 2N), two f32
    adds in that order -> nint_head_bwd (dh only), bit for bit; an unfed image keeps dpred and gets W^T dpred; the image in front
    and the images read stay.  Unmasked, mixed, and a mask of zeros"""
    L, lib = _lib()

    def call(ex):
        s = Setup(lib, L, ex, dt, Cx, O_, Ch, k, cyc, H, W)
        g, st = C.byref(s.g), s.st
        gen = torch.Generator().manual_seed(9)
        dx = ex.copy(torch.randn((1 + N_) * H * W * s.Cxp, generator=gen).to(s.et))
        dp0 = torch.randn(1 + 2 * N_, O_, H, W, generator=gen)
        full = torch.empty(N_, Cx, H, W, device="cuda")
        src = C.c_void_p(dx.data_ptr() + H * W * s.Cxp * s.es)
        if k:
            fn = lib.nint_unfold_dx_cyclic if cyc else lib.nint_unfold_dx
            assert fn(src, MC.P(full), N_, Cx, k, s.Cxp, H, W, dt, st) == 0
        else:
            assert lib.nint_unpack_compact(src, MC.P(full), N_, Cx, s.Cxp, H, W, dt, st) == 0
        torch.cuda.synchronize()
        xi = full[:, s.c0:]
        out = {}
        for tag, fed in (("all", None), ("mixed", [1, 0]), ("zeros", [0, 0])):
            dp, dh = ex.copy(dp0.reshape(-1).clone()), ex.empty((1 + N_) * H * W * s.Chp, s.et, slack=0)
            fp = None if fed is None else (C.c_uint8 * N_)(*fed)
            assert lib.nint_head_feedback_bwd_res(MC.P(dx), 1, MC.P(dp), 1, MC.P(dh), 1, N_, Ch, s.Chp, O_, MC.P(s.w), Cx, s.Cxp, s.c0, k, cyc,
                                                  1 + N_, fp, g, dt, st) == 0
            torch.cuda.synchronize()
            d = dp0.cuda()
            gsum = d[1:1 + N_].clone()
            for i in range(N_):
                if fed is None or fed[i]:
                    gsum[i] = (d[1 + i] + xi[i]) + d[1 + N_ + i]
            want_dp = torch.cat([d[:1], gsum, d[1 + N_:]]).reshape(-1)
            dh2 = torch.empty(N_ * H * W * s.Chp, dtype=s.et, device="cuda")
            gs = gsum.contiguous()
            assert lib.nint_head_bwd(MC.P(dh2), 0, N_, Ch, s.Chp, O_, MC.P(s.w), MC.P(gs), MC.P(dh2), None, None, g, dt, None, 0, st) == 0
            torch.cuda.synchronize()
            got_dp, got_dh = dp[:dp0.numel()].clone(), dh[H * W * s.Chp:(1 + N_) * H * W * s.Chp].clone()
            assert torch.equal(got_dp, want_dp), (name, tag, "dpred")
            assert torch.equal(got_dh.view(torch.uint8), dh2.view(torch.uint8)), (name, tag, "dh")
            out[f"dpred.{tag}"], out[f"dh.{tag}"] = got_dp, got_dh
        assert not torch.equal(out["dpred.all"], out["dpred.zeros"])
        return out
    MC.both_ways(f"head_feedback_bwd_res {name}", call)


def test_refusals_come_before_any_launch_and_leave_every_byte(pkg):
    """every refusal of the new entries on real, exactly sized, poisoned buffers: the code comes back, no buffer byte changes and
    every guard byte of oracle/guarded_alloc.py is intact"""
    L, lib = _lib()
    ex = MC.Exact(False)
    s = Setup(lib, L, ex, 1, 40, 3, 8, 0, 0, 13, 37)
    g, st, n = C.byref(s.g), s.st, N_ * s.O * s.H * s.W
    pred = ex.copy(torch.full((n,), 3.0))
    dp = ex.copy(torch.full(((1 + 2 * N_) * s.O * s.H * s.W,), 2.0))
    dh = ex.copy(torch.full(((1 + N_) * s.H * s.W * s.Chp,), 1.0).to(s.et))
    dx = ex.copy(torch.full(((1 + N_) * s.H * s.W * s.Cxp,), 1.0).to(s.et))
    keep = [t.clone() for t in (pred, dp, dh, dx, s.xs, s.h)]

    def bad(**kw):
        hb = s.base()
        for key, v in kw.items():
            setattr(hb, key, v)
        return C.byref(hb)
    codes = []
    for hb, want in ((bad(x_n0=-1), E_ARG), (bad(c0=38), E_ARG), (bad(xfold_k=2), E_ARG), (bad(Cxp=24), E_ARG), (bad(Cx=0), E_ARG),
                     (bad(xs=s.xs.data_ptr() + 8), E_ALIGN)):
        codes.append((s.head(lib.nint_head_fwd_res, MC.P(pred), g, 1, hb, st), want))
        codes.append((lib.nint_head_fwd_seq_res(MC.P(s.h), 1, N_, s.Ch, s.Chp, s.O, MC.P(s.w), MC.P(s.b), MC.P(pred), g, 1, hb, st), want))
    fb = lambda x_n0, b_n0, fed=None: s.head(lib.nint_head_feedback_res, MC.P(s.xs), x_n0, s.Cx, s.Cxp, s.c0, 0, 0, b_n0, fed, g, 1, st)
    codes += [(fb(N_, 1), E_ARG), (fb(0, 1), E_ARG), (fb(N_, 0, (C.c_uint8 * N_)(1, 3)), E_ARG)]
    fbb = lambda p_n0, pn, fed=None: lib.nint_head_feedback_bwd_res(MC.P(dx), 1, MC.P(dp), p_n0, MC.P(dh), 1, N_, s.Ch, s.Chp, s.O, MC.P(s.w),
                                                                    s.Cx, s.Cxp, s.c0, 0, 0, pn, fed, g, 1, st)
    codes += [(fbb(1, 2), E_ARG), (fbb(1, 0), E_ARG), (fbb(1, 1 + N_, (C.c_uint8 * N_)(2, 0)), E_ARG)]
    torch.cuda.synchronize()
    assert all(got == want for got, want in codes), codes
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(keep, (pred, dp, dh, dx, s.xs, s.h)))
    assert ex.done() > 0


# ====================================================================== the whole-sequence passes, the module, the trainer
def res_net(pkg, case, dtype, cyclic, gt=None, residual=True, **kw):
    """the module of a case (residual_model.CASES) with its weights (the oracle's synthetic ones) and its engine built"""
    c = RES.CASES[case]
    net = pkg.ConvLSTM(c["C"], c["hidden"], c["ks"], len(c["hidden"]), out_channels=c["O"], compute_dtype=dtype, lon_cyclic=cyclic,
                       feedback=True, residual=residual, **kw).cuda()
    net.load_state_dict(RES.case_params(c))
    if gt is not None:
        gt.guard_module(net)
    with MC.knobs(XFOLD=FOLDED[case]):
        eng = net._engine(torch.device("cuda", torch.cuda.current_device()))
    assert bool(eng.cfgs[0].xfold) == FOLDED[case]
    if gt is not None:
        MC._fill_unused_weight_tail(eng, gt.fill)
    return net, eng


def engine_run(net, eng, X, feed, wave=None):
    """one residual forward pass driven through the engine, every slab kept"""
    B, T, _, H, W = X.shape
    O_ = net.conv.weight.shape[0]
    with MC.knobs(FORCE_WAVE=wave):
        ws = eng.acquire(B, T, H, W, False, False)
        try:
            net._pack_weights(eng)
            fb = None if feed is None else (net.conv.weight, net.conv.bias, feed)
            eng.forward(ws, X, feedback=fb, residual=O_)
            res = dict(xs=ws.xs.clone(), seq=eng.head_forward_seq(ws, net.conv.weight, net.conv.bias),
                       pred=eng.head_forward(ws, net.conv.weight, net.conv.bias))
            for l in range(len(eng.cfgs)):
                res[f"h{l}"], res[f"c{l}"] = ws.h[l].clone(), ws.c[l].clone()
        finally:
            eng.release(ws)
    torch.cuda.synchronize()
    return res


def substituted(c, X, seq, fed):
    """X with the feedback channels of the fed (b, t) replaced by the (f32) prediction of the step before"""
    B, T, O_ = c["B"], c["T"], c["O"]
    sv = seq.view(B, T, O_, c["H"], c["W"])
    X2 = X.clone()
    m = RES.fed_mask(fed, B, T)
    for b in range(B):
        for t in range(1, T):
            if bool(m[b, t]):
                X2[b, t, c["C"] - O_:] = sv[b, t - 1]
    return X2


def _mask_of(c):
    return RES.MASK[:, :c["T"]].clone()


@pytest.mark.parametrize("cyclic", **CYC)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(RES.CASES))
def test_closed_loop_is_the_open_loop_on_the_fed_input_bit_for_bit(pkg, case, dtype, cyclic):
    """nint_seq_fwd_residual from s = 1, 2 and under a mask, then the residual open-loop pass over the input with the per-step
    predictions substituted: every byte of xs, every h and c slot of every layer and the predictions are identical (the engine's
    own wave mode and the time-major one); M[b, t] = (t >= s) is from = s; the loop is closed, and the head is residual"""
    c = RES.CASES[case]
    net, eng = res_net(pkg, case, dtype, cyclic)
    plain_net, _ = res_net(pkg, case, dtype, cyclic, residual=False)
    X = RES.case_data(c)["X"].cuda()
    B, T = c["B"], c["T"]
    with torch.no_grad():
        for feed in (1, 2, _mask_of(c)):
            for wave in (None, 0):
                a = engine_run(net, eng, X, feed, wave=wave)
                b = engine_run(net, eng, substituted(c, X, a["seq"], feed), None, wave=wave)
                for k in a:
                    assert torch.equal(a[k], b[k]), (case, dtype, cyclic, feed, wave, k)
            if isinstance(feed, int):
                m = engine_run(net, eng, X, SM.suffix(B, T, feed))
                assert all(torch.equal(a[k], m[k]) for k in a), (case, feed, "mask = suffix")
                assert torch.equal(net(X, free_from=feed), a["pred"]) and torch.equal(net(X, free_mask=SM.suffix(B, T, feed)), a["pred"])
            else:
                assert torch.equal(net(X, free_mask=feed), a["pred"])
            open_ = engine_run(net, eng, X, None)
            assert not torch.equal(a["seq"], open_["seq"])
            assert not torch.equal(a["pred"], plain_net(X, **(dict(free_from=feed) if isinstance(feed, int) else dict(free_mask=feed))))
        # nothing fed: the residual teacher-forced module = the non-residual one + the input's tracer, bit for bit
        O_ = c["O"]
        assert torch.equal(net(X), plain_net(X) + X[:, -1, c["C"] - O_:].to(torch.bfloat16 if dtype == "bf16" else torch.float32).float())
        assert torch.equal(net(X, free_from=T), net(X))


def _limits(g, dtype):
    return {k: RM.BF16_GATE for k in g}


@pytest.mark.parametrize("cyclic", **CYC)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", sorted(RES.CASES))
def test_autograd_parity_with_the_cpu_model(pkg, case, dtype, cyclic):
    """net(x[, state], free_from / free_mask, feedback_grad=True) and the teacher-forced call, cotangents on pred and seq (and on the
    returned state): outputs, every parameter gradient, dx -- the skip add on the unfed feedback channels, exact zeros on the fed
    ones -- and the state gradients at the standing gates; and the device's gradient of every parameter is more than a gate away
    from the gradient without the skip term and from the non-residual model's (the CPU model puts both tens of gates away:
    tests/test_residual_cpu.py), so neither a forgotten `+ g_u` nor a non-residual launch can pass.

    bf16: rel-L2 <= 2e-2 against the f32 model, or, where the storage-rounding floor of the EXISTING path is above that, twice that
    floor -- measured here as the non-residual module's teacher-forced gradients on the same fed input against its CPU model (the
    rule of tests/test_gpu_rollout.py, whose cases' scaled feedback columns put some tensors of that path at the gate already)."""
    c = RES.CASES[case]
    B, T, c0 = c["B"], c["T"], c["C"] - c["O"]
    net, eng = res_net(pkg, case, dtype, cyclic, return_sequence=True)
    floor_net, _ = res_net(pkg, case, dtype, cyclic, residual=False, return_sequence=True)
    d = RES.case_data(c)
    X = d["X"].cuda()
    bad = []

    def held(fn, *a):
        try:
            fn(*a)
        except AssertionError as e:
            bad.append(str(e).splitlines()[0])

    cmp_out = (lambda a, b, what: assert_bf16(a, b, what, RM.BF16_GATE)) if dtype == "bf16" else assert_close_out
    feeds = [("tf", None), ("from-1", 1), ("mask", _mask_of(c))] + ([("from-T-1", T - 1)] if case in ("thin", "wide") else [])
    for with_state in ((False, True) if case in ("thin", "wide", "chv128") else (False,)):
        for fname, feed in feeds:
            res, noskip, nonres = RES.reference(case, cyclic, feed, with_state)
            m = RES.fed_mask(feed, B, T)
            tag = f"{case} {dtype} {fname} state={int(with_state)}"
            kw = {} if feed is None else dict(feedback_grad=True)
            if feed is not None and not isinstance(feed, int):
                kw["free_mask"] = feed
            seq, pred, g = _grads_on_device(net, d, X, feed if isinstance(feed, int) else None, with_state, **kw)
            held(cmp_out, seq, res["seq"].float(), f"{tag} seq")
            held(cmp_out, pred, res["pred"].float(), f"{tag} pred")
            fedc = m.view(B, T, 1, 1, 1).expand(B, T, c["O"], c["H"], c["W"])
            assert not bool(g["dx"].cpu()[:, :, c0:][fedc].any()), tag
            limit = {k: RM.BF16_GATE for k in g}
            if dtype == "bf16":
                xf = substituted(c, X, seq, feed)
                _, _, g_tf = _grads_on_device(floor_net, d, xf, None, with_state)
                kws = dict(dpred=d["dpred"], dseq=d["dseq"])
                if with_state:
                    kws.update(h0=[t.double() for t in d["h0"]], c0=[t.double() for t in d["c0"]], dhT=d["dhT"], dcT=d["dcT"])
                tf_dev = RM.grads(xf.cpu().double(), RES.case_params(c, torch.float64), None, cyclic, "f32", **kws)
                for k in g:
                    floor, r = _rel(g_tf[k], _ref_grad(tf_dev, k)), _rel(g[k], _ref_grad(res, k))
                    limit[k] = max(RM.BF16_GATE, 2 * floor)
                    print(f"  {tag} {k}: rel-L2 {r:.3e}  floor (non-residual, teacher-forced) {floor:.3e}")
                    if r > limit[k]:
                        bad.append(f"{tag} {k}: rel-L2 {r:.3e} > {limit[k]:.3e} (floor {floor:.3e})")
            else:
                for k in g:
                    held(assert_close_grad, g[k], _ref_grad(res, k).float(), f"{tag} {k}")
            # the skip term and the base are there: away from both other gradients wherever the CPU model separates them
            for other, what in ((noskip, "without the skip term"), (nonres, "non-residual")):
                if feed is None and other is noskip:
                    continue                                 # (nothing fed: there is no skip term to drop)
                sep = RES.separation(res, other)
                for n in res["params"]:
                    k, t = "d " + n, other["params"][n]
                    if dtype == "bf16":
                        far, dist = sep[n][1] * RM.BF16_GATE / limit[k], _rel(g[k], t) / limit[k]
                    else:
                        far, dist = sep[n][0], float((g[k].cpu().double() - t).abs().max()) / RM.F32_GATE(t)
                    if far > 2 and dist <= 1:
                        bad.append(f"{tag} {k}: within a gate of the gradient {what} (CPU model: {far:.1f} gates apart)")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", BOTH)
def test_mask_equals_from_in_the_gradients_and_need_dx_does_not_matter(pkg, dtype):
    """free_mask = (t >= s) is free_from = s bit for bit, gradients included; the engine's roll-out with and without dx gives the
    same parameter gradients and slab (the one-step d/dx scratch)"""
    c = RES.CASES["thin"]
    net, eng = res_net(pkg, "thin", dtype, True, return_sequence=True)
    d = RES.case_data(c)
    X = d["X"].cuda()
    a = _grads_on_device(net, d, X, 2, False, feedback_grad=True)
    b = _grads_on_device(net, d, X, None, False, feedback_grad=True, free_mask=SM.suffix(c["B"], c["T"], 2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    net.zero_grad()
    pred, seq = net(X, free_from=2, feedback_grad=True)            # x needs no gradient: need_dx = 0
    torch.autograd.backward([pred, seq], [d["dpred"].cuda(), d["dseq"].cuda()])
    for n, p in net.named_parameters():
        assert torch.equal(p.grad, a[2]["d " + n]), n


# ------------------------------------------------------------------ the trainer
LR, BETAS, HALO = 1e-4, (0.5, 0.999), (2, 3)
TRAIN = {"teacher-forced": {}, "rollout": dict(rollout_from=1), "sampled": dict(rollout_from=1, sampling_prob=0.5, sampling_seed=4),
         "rollout-last-step": dict(rollout_from=2)}


def _train_batches(c, n, sq):
    rng = np.random.default_rng(91)
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    Hc, Wc = H - 2 * HALO[0], W - 2 * HALO[1]
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return [(f(B, T, c["C"], H, W), f(*((B, T, c["O"], Hc, Wc) if sq else (B, c["O"], Hc, Wc)))) for _ in range(n)]


def _feeds(c, variant, n):
    """the feed of each of n steps, as FusedTrainer draws it"""
    from nasa_niswan_amd.trainer import FusedTrainer
    kw = TRAIN[variant]
    if "rollout_from" not in kw:
        return [None] * n
    if "sampling_prob" not in kw:
        return [kw["rollout_from"]] * n
    gen = FusedTrainer.sampler(kw["sampling_seed"], 0)
    return [FusedTrainer.draw_mask(gen, c["T"], c["B"], kw["rollout_from"], kw["sampling_prob"]).t().contiguous() for _ in range(n)]


def _cpu_fit(c, batches, feeds, cyclic, sq):
    p = {n: v.clone().requires_grad_(True) for n, v in RES.case_params(c, torch.float64).items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR, betas=BETAS)
    B, T, O_, H, W = c["B"], c["T"], c["O"], c["H"], c["W"]
    out = []
    for (X, y), feed in zip(batches, feeds):
        opt.zero_grad()
        r = RES.forward(X.double(), p, feed, cyclic, "f32")
        o = r["seq"].view(B, T, O_, H, W) if sq else r["pred"]
        dd = y.double() - o[..., HALO[0]:H - HALO[0], HALO[1]:W - HALO[1]]
        loss = (dd * dd).mean() + dd.abs().mean()
        loss.backward()
        grads = {n: v.grad.detach().clone() for n, v in p.items()}
        opt.step()
        out.append(dict(loss=float(loss.detach()), grads=grads, params={n: v.detach().clone() for n, v in p.items()}))
    return out


@pytest.mark.parametrize("variant", sorted(TRAIN))
@pytest.mark.parametrize("dtype", BOTH)
def test_two_trainer_steps_against_cpu_autograd_and_adam(pkg, dtype, variant):
    """FusedTrainer on a residual model -- teacher-forced, rollout_from, sampling_prob (the trainer's own draws replayed on the
    host), with the sequence loss and (rollout-last-step) with the last-step loss -- on the folded cyclic case: the loss of every
    call, the bucket's gradient at the first step and the parameters after each, at the tolerances of tests/test_gpu_rollout.py
    (loss: f32 1e-4 relative + 1e-5, bf16 2e-2 relative; parameters after k Adam steps at lr 1e-4: max |dp| <= k * 2.2 * lr, mean
    |dp| <= 2e-6 in f32, 0.1 * lr * k in bf16; gradients: the standing gates)"""
    from nasa_niswan_amd.trainer import FusedTrainer
    c = RES.CASES["thin"]
    sq = variant != "rollout-last-step"
    batches = _train_batches(c, 2, sq)
    feeds = _feeds(c, variant, 2)
    if variant == "sampled":
        assert any(0 < int(f.sum()) < f[:, 1:].numel() for f in feeds)        # a mixed draw: the masked launches run
    want = _cpu_fit(c, batches, feeds, True, sq)
    net, eng = res_net(pkg, "thin", dtype, True)
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, sequence_loss=sq, **TRAIN[variant])
    names = [n for n, _ in net.named_parameters()]
    for step in (1, 2):
        X, y = batches[step - 1]
        loss = float(tr.step(X.cuda(), y.cuda()))
        if variant == "sampled":
            assert torch.equal(tr.last_mask.t(), feeds[step - 1])
        o = want[step - 1]
        print(f"  {variant} {dtype} step {step}: loss {loss:.7f} cpu {o['loss']:.7f}")
        assert abs(loss - o["loss"]) <= (1e-4 * abs(o["loss"]) + 1e-5 if dtype == "f32" else 2e-2 * abs(o["loss"]))
        if step == 1:
            for i, n in enumerate(names):
                gr = tr.flat.grad_view(i).view(o["grads"][n].shape)
                if dtype == "bf16":
                    assert_bf16(gr, o["grads"][n].float(), f"bucket d {n}", RM.BF16_GATE)
                else:
                    assert_close_grad(gr, o["grads"][n].float(), f"bucket d {n}")
        for n, v in net.state_dict().items():
            dd = (v.cpu().double() - o["params"][n]).abs()
            assert float(dd.max()) <= step * 2.2 * LR, (n, step)
            assert float(dd.mean()) <= (2e-6 if dtype == "f32" else 0.1 * LR * step), (n, step)


def test_trainer_options_compose_and_the_loss_entries_agree(pkg):
    """a residual model under bptt_segments, stateful chunks and a configured loss: segments give the whole window's loss and
    gradients (the base of a step is that step's input: nothing crosses a boundary); the default spec gives the plain step's bits"""
    from nasa_niswan_amd.loss import LossSpec
    from nasa_niswan_amd.trainer import FusedTrainer
    c = RES.CASES["thin"]
    (X, y), = _train_batches(c, 1, False)
    runs = {}
    for name, kw in (("whole", {}), ("segments", dict(bptt_segments=2)), ("spec", dict(loss=LossSpec())), ("stateful", dict(stateful=True))):
        net, _ = res_net(pkg, "thin", "f32", True)
        tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO, **kw)
        runs[name] = (tr.step(X.cuda(), y.cuda()).clone(), tr.flat.grad.clone())
    assert torch.equal(runs["whole"][0], runs["spec"][0]) and torch.equal(runs["whole"][1], runs["spec"][1])
    assert torch.equal(runs["whole"][0], runs["segments"][0])
    assert_close_grad(runs["segments"][1], runs["whole"][1], "segments bucket")
    assert_close_grad(runs["stateful"][1], runs["whole"][1], "stateful bucket (first chunk: the zero state)")
    # ... and evaluate() sees the residual head: the loss of a head of zeros is that of persistence
    net, _ = res_net(pkg, "thin", "f32", True)
    with torch.no_grad():
        net.conv.weight.zero_(); net.conv.bias.zero_()
    tr = FusedTrainer(net, lr=LR, betas=BETAS, halo=HALO)
    pred = tr.evaluate(X.cuda(), y.cuda())
    assert torch.equal(pred, X[:, -1, c["C"] - c["O"]:].cuda())


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("variant", ["sampled", "rollout-last-step"])
def test_trainer_under_the_guarded_allocator(pkg, variant, dtype):
    """tests/test_gpu_memory_contract.py's three runs of two optimizer steps: no store outside an extent, no result from a byte
    the library did not write (the roll-out slab, the one-step d/dx scratch and dh_seq are uninitialised allocations)"""
    from nasa_niswan_amd.trainer import FusedTrainer
    case = "wide" if variant == "rollout-last-step" else "thin"
    c = RES.CASES[case]
    sq = variant != "rollout-last-step"

    def scenario(gt):
        G = (lambda t: t) if gt is None else gt.guard_copy
        net, _ = res_net(pkg, case, dtype, True, gt=gt)
        tr = FusedTrainer(net, lr=1e-3, betas=BETAS, halo=HALO, sequence_loss=sq, max_grad_norm=0.05, **TRAIN[variant])
        res = {}
        for j, (X, y) in enumerate(_train_batches(c, 2, sq)):
            res[f"loss.{j}"] = tr.step(G(X.cuda()), G(y.cuda())).detach().clone()
        res["bucket"], res["bucket.grad"], res["stats"] = tr.flat.data, tr.flat.grad, tr.stats
        return res
    stack = (c["C"], c["hidden"], c["ks"])
    assert MC.three_runs(f"residual-trainer-{variant}-{dtype}", scenario, MC.row_stride(stack, (c["H"], c["W"]))) > 0


def test_refusals_on_the_device(pkg):
    from nasa_niswan_amd._lib import NintError
    from nasa_niswan_amd.trainer import FusedTrainer
    c = RES.CASES["thin"]
    net, eng = res_net(pkg, "thin", "f32", False)
    d = RES.case_data(c)
    X = d["X"].cuda()
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    st = [(h.cuda(), cc.cuda()) for h, cc in zip(d["h0"], d["c0"])]
    with pytest.raises(ValueError, match="step 0 cannot be fed"):
        net(X, st, free_from=0)
    with pytest.raises(ValueError, match="step 0 cannot be fed"):
        net(X, st, free_mask=torch.ones(B, T, dtype=torch.bool))
    ws = eng.acquire(B, T, H, W, False, True)
    net._pack_weights(eng)
    with pytest.raises(ValueError, match="step 0 cannot be fed"):
        eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 0), residual=c["O"])
    # the library's own refusal, behind the host's: a fed step 0 through the _residual entry
    eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 1), residual=c["O"])
    before = ws.xs.clone()
    ws.feedback.fb.from_step = 0
    with pytest.raises(NintError, match="invalid argument"):
        eng._seq_pass(ws, False)
    torch.cuda.synchronize()
    assert torch.equal(ws.xs, before)
    with pytest.raises(ValueError, match="slot 0"):
        eng.head_forward(ws, net.conv.weight, net.conv.bias, slot=0)
    eng.release(ws)
    with pytest.raises(RuntimeError, match="back-propagation through the fed-back prediction"):
        net(X, free_from=1)
    with pytest.raises(ValueError, match="rollout_from must be a step index >= 1"):
        FusedTrainer(net, rollout_from=0)
    with pytest.raises(ValueError, match="not supported"):
        FusedTrainer(net, rollout_from=1, stateful=True)
    big = pkg.ConvLSTM(8, [16, 160], [3, 3], 2, out_channels=2, feedback=True, residual=True).cuda()
    with torch.no_grad():
        with pytest.raises(NintError, match="beyond the staged head"):
            big(torch.randn(1, 3, 8, 8, 8, device="cuda"))


# ------------------------------------------------------------------ inference
def _tracer_dataset(period="train", n_steps=17, T=4, grid=(12, 20), **kw):
    from nasa_niswan_amd.dataset import SyntheticE33OMA_CRNN
    return SyntheticE33OMA_CRNN(period, padding=None, in_channels=6, sequence_length=T, levels=1, n_steps=n_steps, grid=grid,
                                device="cuda", tracer_input=True, **kw)


def _tracer_net(pkg, dtype, seed=5, residual=True):
    from oracle import convlstm_oracle as O
    net = pkg.ConvLSTM(6, [16, 8], [5, 3], 2, out_channels=1, compute_dtype=dtype, lon_cyclic=True, feedback=True, residual=residual).cuda()
    net.load_state_dict(O.synth_params(6, [16, 8], [5, 3], 2, out_channels=1, seed=seed))
    return net


@pytest.mark.parametrize("dtype", BOTH)
def test_predict_stream_in_chunks_is_one_long_window(pkg, dtype):
    """predict_stream(closed_loop=True) over three chunks equals ONE residual closed-loop window over the period bit for bit: a
    later chunk's step 0 receives the previous chunk's last prediction through the pack and the chunk is fed from step 1; the open
    walk and predict / evaluate_skill use the residual head too"""
    from nasa_niswan_amd.dataset import SlabBatch
    from nasa_niswan_amd.inference import evaluate_skill, predict, predict_stream
    ds = _tracer_dataset()
    T = ds.seq_len
    net = _tracer_net(pkg, dtype)
    pred, steps, dropped = predict_stream(net, ds, lanes=1, halo=(0, 0), closed_loop=True, spinup=2)
    assert pred.shape[0] == 3 * T and int(steps[0]) == 1
    eng = net._engine(pred.device)
    X = SlabBatch(ds, np.asarray([int(ds.first[0])]), 3 * T)
    H, W = ds.grid
    with torch.no_grad(), eng.window(1, 3 * T, H, W, False, False) as ws:
        net._pack_weights(eng)
        eng.forward(ws, X, feedback=(net.conv.weight, net.conv.bias, 2), residual=1)
        whole = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(3 * T, 1, H, W)
        eng.forward(ws, X, residual=1)
        open_ = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(3 * T, 1, H, W)
    assert torch.equal(pred, whole) and not torch.equal(pred[3:], open_[3:]) and torch.equal(pred[:2], open_[:2])
    walk, _, _ = predict_stream(net, ds, lanes=1, halo=(0, 0))
    assert walk.shape == open_.shape and torch.equal(walk[:2], open_[:2]) and bool(torch.isfinite(walk).all())
    # predict and evaluate_skill: the residual head of the last step, against the module
    idx = [0, 3]
    gt_, pd_ = predict(net, ds, batch_size=2, halo=(0, 0), indices=idx)
    Xb, _ = ds.device_batch(idx)
    with torch.no_grad():
        want = net(Xb)
    assert np.array_equal(pd_, want.cpu().numpy() * ds.y_std + ds.y_mean)
    acc, preds = evaluate_skill(net, ds, batch_size=2, halo=(0, 0), indices=idx, return_predictions=True)
    assert torch.equal(preds, want) and acc.n_samples == 2
    plain = _tracer_net(pkg, dtype, residual=False)
    with torch.no_grad():
        assert not torch.equal(plain(Xb), want)


def test_rollout_skill_runs_with_the_residual_head(pkg):
    from nasa_niswan_amd.dataset import SlabBatch
    from nasa_niswan_amd.inference import lead_time_r2, rollout_skill
    ds = _tracer_dataset(n_steps=30)
    net = _tracer_net(pkg, "f32")
    H, W = ds.grid
    starts, horizon, spinup = [1, 4, 9, 16], 3, 2
    acc = rollout_skill(net, ds, starts, horizon, spinup, 2)
    pix, counts, sample = acc.sums()
    assert list(counts) == [len(starts)] * horizon and np.isfinite(lead_time_r2(acc)).all()
    # slot j holds the predictions of window step spinup + j of the residual closed loop: sum p of slot 0 against the engine's own pass
    eng = net._engine(torch.device("cuda", torch.cuda.current_device()))
    tot = 0.0
    for i in range(0, len(starts), 2):
        t0s = starts[i:i + 2]
        with torch.no_grad(), eng.window(len(t0s), spinup + horizon, H, W, False, False) as ws:
            net._pack_weights(eng)
            eng.forward(ws, SlabBatch(ds, np.asarray(t0s), spinup + horizon), feedback=(net.conv.weight, net.conv.bias, spinup), residual=1)
            seq = eng.head_forward_seq(ws, net.conv.weight, net.conv.bias).view(len(t0s), spinup + horizon, 1, H, W)
        tot += float(seq[:, spinup].double().sum())
    assert abs(float(pix[0, 1].sum()) - tot) <= 1e-9 * max(1.0, abs(tot))


# ------------------------------------------------------------------ train.py
def test_train_py_residual_head_end_to_end_and_reload(pkg, tmp_path, monkeypatch):
    """train.py --tracer-input --residual-head --rollout-from 1 on the synthetic record: ten short epochs write a snapshot whose
    arguments hold the flag; it reloads into a residual run, and a run without the flag is refused as its successor's origin"""
    from nasa_niswan_amd import train as T
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    snap = tmp_path / "s"
    base = ["--model", "LSTM-res", "--in-channels", "5", "--hidden-channels", "8", "4", "--kernel-size", "3", "3", "--num-layers", "2",
            "--sequence-length", "3", "--input-size", "8", "12", "--grid", "8", "12", "--batch-size", "4", "--learning-rate", "1e-4",
            "--synthetic-steps", "40", "--dtype", "f32", "--cyclic-longitude", "--tracer-input", "--residual-head", "--rollout-from", "1"]
    logger = T.main(T.get_arguments(base + ["--num-epochs", "10", "--snapshot-dir", str(snap)]))
    assert np.isfinite(logger["MSELoss"]).all() and len(logger["MSELoss"]) == 10
    assert (snap / "epoch-010" / "generator.pth.tar").is_file() and T.checkpoint_residual_head(str(snap / "epoch-010")) is True
    again = T.main(T.get_arguments(base + ["--num-epochs", "1", "--snapshot-dir", str(tmp_path / "t"), "--use-checkpoint",
                                           "--restore-from", str(snap / "epoch-010")]))
    assert np.isfinite(again["MSELoss"]).all()
    # the resumed run starts where the first one stood: its first loss is below the first run's first loss
    assert again["first_step_loss"] < logger["first_step_loss"] * 1.5
