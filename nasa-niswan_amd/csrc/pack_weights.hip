// pack_weights.hip -- a layer's f32 weights into the images the gate kernels read: the MFMA fragment-order forward and
// dgrad images, the permuted bias, and behind them the stencil rows and the dense-K image of tiny hidden widths; with the
// size rules the callers share (nint_kc, nint_xfold_pays, nint_packed_weight_bytes).
#include "nint_common.h"

// ------------------------------------------------------------------------------ weight packing
// Fragment order: Bp[s][nt][lane][e]; s = K-step; lane = 16*g + col;
// the lane's e-th element is K-channel chunk*KC + g*EPL + e and output column nt*16 + col.
//   fwd  : K-steps = x chunks x taps, then h chunks x taps; K-channel -> cat[x,h] channel (x part padded to Cxp),
//          column n' -> gate*Ch + cblock*16+col
//   dgrad: K-channel -> gate column n' of dG, column -> cat channel, taps flipped
// xfold (horizontally folded x source, nint_layer.xfold): the x chunks have k vertical taps only and their
// K-channel kc = kx*Cx + c selects W[.][c][ky][kx]; in the dgrad image the folded x columns take their weight
// at the centre-column taps (tx = k/2) and zero elsewhere.
template <int DT>
__device__ __forceinline__ void pack_weights_body(const float* __restrict__ W, const float* __restrict__ bias, void* __restrict__ Wf,
                                                  void* __restrict__ Wd, float* __restrict__ bias_p, int Cx, int Cxp, int Ch, int Ch16,
                                                  int Chp, int k, int xfold) {
  typedef Elem<DT> E;
  const int taps = k * k;
  const int Ctot = Cx + Ch;
  const int ntf = 4 * Ch16 / 16;
  const int sx = Cxp / E::KC * (xfold ? k : taps);              // K-steps of the x part
  const int sf = sx + Chp / E::KC * taps;
  const size_t nf = (size_t)sf * ntf * 64 * E::EPL;
  const int ntd = (Cxp + Chp) / 16;
  const int sd = 4 * Ch16 / E::KC * taps;
  const size_t nd = (size_t)sd * ntd * 64 * E::EPL;
  const size_t nb = 4 * Ch16;
  // stencil image (csrc/stencil.hip; tiny hidden widths): rows of 32 f32, row order = the kernel's iteration order
  //   for ky: [x source: per channel quad q: (plain) kx = 0, 1, 2 x 4 channels | (folded) 4 folded channels]  [h source: per quad: kx x 4]
  // column o = gate*8 + ch; values rounded to the storage type like the MFMA images
  const bool st = nint_stencil_shape(Cx, Ch, k, xfold);
  const int rpk = st ? nint_stencil_rows(Cx, Ch, xfold) : 0;
  const size_t ns = (size_t)3 * rpk * 32;
  float* Ws = (float*)((char*)Wf + nint_internal_stencil_offset(Cxp, Chp, Ch16, k, DT));
  // dense-K image (csrc/tiny_gemm.hip): [K-step][column tile 2][lane 64][16 B] in ET + the group table (ints) behind it
  const bool tg = nint_tiny_shape(Cx, Ch, k, xfold, DT);
  const size_t ntg = tg ? (size_t)NINT_TINY_MAXSTEPS * 2 * 64 * E::EPL : 0;
  const size_t ntt = tg ? 4 * NINT_TINY_MAXSTEPS : 0;
  char* Wt = (char*)Wf + nint_internal_tiny_offset(Cx, Cxp, Ch, Chp, Ch16, k, xfold, DT);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nf + nd + nb + ns + ntg + ntt; i += (size_t)gridDim.x * blockDim.x) {
    if (i >= nf + nd + nb + ns) {
      const size_t ii = i - nf - nd - nb - ns;
      const int xg = nint_tiny_xg(Cx, xfold, DT), hg = nint_tiny_hg(Ch, DT), ngx = nint_tiny_ngx(Cx, xfold, DT), ng = ngx + 9 * hg;
      // group gi -> (source, tap, 16-byte piece q of the pixel)
      auto group = [&](int gi, int& ky, int& kx, int& q, bool& isx) {
        isx = gi < ngx;
        if (isx) {
          if (xfold) { ky = gi / xg; kx = 1; q = gi % xg; }
          else { const int tp = gi / xg; q = gi % xg; ky = tp / 3; kx = tp % 3; }
        } else {
          const int gj = gi - ngx, tp = gj / hg; q = gj % hg; ky = tp / 3; kx = tp % 3;
        }
      };
      if (ii < ntg) {
        const int e = ii % E::EPL;
        size_t r = ii / E::EPL;
        const int lane = r % 64; r /= 64;
        const int tl = r % 2;
        const int s = (int)(r / 2);
        const int gi = 4 * s + (lane >> 4), m = lane & 15;          // the lane's K group; output row m of column tile tl
        const int gate = m % 4, ch = 2 * (m / 4) + tl;               // row = 4 c + gate, channel = 2 c + tile
        float v = 0.f;
        if (gi < ng && ch < Ch) {
          int ky, kx, q; bool isx;
          group(gi, ky, kx, q, isx);
          const int c = q * E::EPL + e;                             // channel inside the pixel's (real) channels of that source
          int ic = -1;
          if (isx) {
            if (xfold) { if (c < 3 * Cx) { kx = c / Cx; ic = c % Cx; } }
            else if (c < Cx) ic = c;
          } else if (c < Ch) {
            ic = Cx + c;
          }
          if (ic >= 0) v = W[(((size_t)(gate * Ch + ch)) * Ctot + ic) * taps + ky * k + kx];
        }
        store_elem<DT>(Wt, ii, v);
      } else {
        // table[gi]: byte offset of the group inside its source's LDS halo image, relative to the lane's own pixel at tap (0, 0)
        const int gi = (int)(ii - ntg);
        int off = 0;
        if (gi < ng) {
          int ky, kx, q; bool isx;
          group(gi, ky, kx, q, isx);
          off = (ky * NINT_TINY_HW + kx) * (isx ? xg : hg) * 16 + q * 16;
        }
        ((int*)(Wt + (size_t)NINT_TINY_MAXSTEPS * 2 * 1024))[gi] = off;
      }
    } else if (i >= nf + nd + nb) {
      const size_t ii = i - nf - nd - nb;
      const int o = ii % 32, gate = o >> 3, ch = o & 7;
      int r = (int)(ii / 32);
      const int ky = r / rpk; r -= ky * rpk;
      const int rx = xfold ? 4 * nint_cdiv(3 * Cx, 4) : 12 * nint_cdiv(Cx, 4);
      int ic = -1, kx = 0;
      if (r < rx) {
        if (xfold) { if (r < 3 * Cx) { kx = r / Cx; ic = r % Cx; } }
        else { const int q = r / 12, kk = (r % 12) / 4, e = r % 4; kx = kk; if (4 * q + e < Cx) ic = 4 * q + e; }
      } else {
        const int rh = r - rx, q = rh / 12, e = rh % 4;
        kx = (rh % 12) / 4;
        if (4 * q + e < Ch) ic = Cx + 4 * q + e;
      }
      float v = 0.f;
      if (ic >= 0 && ch < Ch) v = W[(((size_t)(gate * Ch + ch)) * Ctot + ic) * taps + ky * k + kx];
      if (DT == NINT_BF16) v = bf2f(f2bf(v));
      Ws[ii] = v;
    } else if (i < nf) {
      const int e = i % E::EPL;
      size_t r = i / E::EPL;
      const int lane = r % 64; r /= 64;
      const int nt = r % ntf;
      const int s = r / ntf;
      const int kl = (lane >> 4) * E::EPL + e;                  // channel inside the chunk
      int ic = -1, tap = 0;
      if (s < sx) {
        if (xfold) {
          const int chunk = s / k, ky = s % k;
          const int kc = chunk * E::KC + kl;                     // folded channel kx*Cx + c
          if (kc < k * Cx) { ic = kc % Cx; tap = ky * k + kc / Cx; }
        } else {
          const int chunk = s / taps;
          tap = s % taps;
          const int kc = chunk * E::KC + kl;
          if (kc < Cx) ic = kc;
        }
      } else {
        const int sh = s - sx;
        const int chunk = sh / taps;
        tap = sh % taps;
        const int hc = chunk * E::KC + kl;
        if (hc < Ch) ic = Cx + hc;
      }
      const int cblock = nt / 4, gate = nt % 4, col = lane & 15;
      const int ch = cblock * 16 + col;
      float v = 0.f;
      if (ic >= 0 && ch < Ch) v = W[(((size_t)(gate * Ch + ch)) * Ctot + ic) * taps + tap];
      store_elem<DT>(Wf, i, v);
    } else if (i < nf + nd) {
      const size_t ii = i - nf;
      const int e = ii % E::EPL;
      size_t r = ii / E::EPL;
      const int lane = r % 64; r /= 64;
      const int nt = r % ntd;
      const int s = r / ntd;
      const int chunk = s / taps, tap = s % taps;
      const int np = chunk * E::KC + (lane >> 4) * E::EPL + e;       // gate column n' of dG
      const int cblock = np / 64, gate = (np % 64) / 16, colk = np % 16;
      const int ch = cblock * 16 + colk;
      const int j = nt * 16 + (lane & 15);                           // cat channel (padded space)
      const int ty = tap / k, tx = tap % k;
      int ic = -1;
      int ftap = (k - 1 - ty) * k + (k - 1 - tx);
      if (j < Cxp) {
        if (xfold) {
          if (j < k * Cx && tx == k / 2) { ic = j % Cx; ftap = (k - 1 - ty) * k + j / Cx; }
        } else if (j < Cx) {
          ic = j;
        }
      } else {
        const int hc = j - Cxp;
        if (hc < Ch) ic = Cx + hc;
      }
      float v = 0.f;
      if (ic >= 0 && ch < Ch) v = W[(((size_t)(gate * Ch + ch)) * Ctot + ic) * taps + ftap];
      store_elem<DT>(Wd, ii, v);
    } else {
      const int n = (int)(i - nf - nd);
      const int cblock = n / 64, gate = (n % 64) / 16, col = n % 16;
      const int ch = cblock * 16 + col;
      bias_p[n] = (ch < Ch && bias) ? bias[gate * Ch + ch] : 0.f;
    }
  }
}

template <int DT>
__global__ void pack_weights_kernel(const float* __restrict__ W, const float* __restrict__ bias, void* __restrict__ Wf,
                                    void* __restrict__ Wd, float* __restrict__ bias_p, int Cx, int Cxp, int Ch, int Ch16,
                                    int Chp, int k, int xfold) {
  pack_weights_body<DT>(W, bias, Wf, Wd, bias_p, Cx, Cxp, Ch, Ch16, Chp, k, xfold);
}

// every layer of a model in one launch: layer = blockIdx.y
struct PackEntry { const float* W; const float* bias; void* Wf; void* Wd; float* bias_p; int Cx, Cxp, Ch, Ch16, Chp, k, xfold; };
struct PackTable { PackEntry e[NINT_MAX_LAYERS]; };
template <int DT>
__global__ void pack_weights_layers_kernel(PackTable t) {
  const PackEntry& E = t.e[blockIdx.y];
  pack_weights_body<DT>(E.W, E.bias, E.Wf, E.Wd, E.bias_p, E.Cx, E.Cxp, E.Ch, E.Ch16, E.Chp, E.k, E.xfold);
}

extern "C" int nint_kc(int dtype) { return dtype == NINT_BF16 ? 32 : (dtype == NINT_F32 ? 16 : NINT_E_ARG); }

// Folding pays when it lowers the number of x K-steps: ceil(k*Cx / KC) * k  <  ceil(Cx / KC) * k * k
extern "C" int nint_xfold_pays(int Cx, int k, int dtype) {
  const int kc = nint_kc(dtype);
  if (kc < 0 || Cx <= 0 || k <= 1 || !(k & 1)) return 0;
  return nint_cdiv(k * Cx, kc) < nint_cdiv(Cx, kc) * k ? 1 : 0;
}

extern "C" size_t nint_packed_weight_bytes(int Cx, int Ch, int k, int dtype, int xfold) {
  const int kc = nint_kc(dtype);
  if (kc < 0) return 0;
  const int es = dtype == NINT_BF16 ? 2 : 4;
  const int Cxp = nint_round_up(xfold ? k * Cx : Cx, kc), Chp = nint_round_up(Ch, kc), Ch16 = nint_round_up(Ch, 16);
  // both images fit in (Cxp+Chp) x 4*Ch16 x taps elements (the folded forward image is smaller); tiny hidden widths keep the
  // stencil kernel's f32 weight rows behind them (csrc/stencil.hip)
  size_t n = (size_t)(Cxp + Chp) * 4 * Ch16 * k * k * es;
  if (nint_stencil_shape(Cx, Ch, k, xfold))       // (+ the dense-K image of csrc/tiny_gemm.hip behind the stencil rows)
    n = nint_internal_tiny_offset(Cx, Cxp, Ch, Chp, Ch16, k, xfold, dtype) + nint_tiny_bytes();
  return n;
}

extern "C" int nint_pack_weights(const float* W, const float* bias, void* Wf, void* Wd, float* bias_p, int Cx,
                                 int Ch, int k, int xfold, int dtype, void* stream) {
  if (!W || !Wf || !Wd || !bias_p || Cx <= 0 || Ch <= 0 || !(k & 1) || (xfold != 0 && xfold != 1)) return NINT_E_ARG;
  const int kc = nint_kc(dtype);
  if (kc < 0) return NINT_E_ARG;
  const int Cxp = nint_round_up(xfold ? k * Cx : Cx, kc), Chp = nint_round_up(Ch, kc), Ch16 = nint_round_up(Ch, 16);
  const size_t n = 2 * (size_t)(Cxp + Chp) * 4 * Ch16 * k * k + 4 * Ch16 + 3 * 32 * (size_t)(nint_stencil_shape(Cx, Ch, k, xfold) ? nint_stencil_rows(Cx, Ch, xfold) : 0)
                   + (nint_tiny_shape(Cx, Ch, k, xfold, dtype) ? (size_t)NINT_TINY_MAXSTEPS * 2 * 64 * (dtype == NINT_BF16 ? 8 : 4) + 4 * NINT_TINY_MAXSTEPS : 0);
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(pack_weights_kernel<decltype(dt)::value>, grid1d(n), dim3(256), 0, (hipStream_t)stream, W, bias, Wf, Wd, bias_p, Cx, Cxp, Ch, Ch16, Chp, k, xfold);
  });
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_pack_weights_layers(const float* const* W, const float* const* bias, const nint_layer* layers, int L,
                                        int dtype, void* stream) {
  if (!W || !bias || !layers || L < 1 || L > NINT_MAX_LAYERS) return NINT_E_ARG;
  const int kc = nint_kc(dtype);
  if (kc < 0) return NINT_E_ARG;
  PackTable t = {};
  size_t nmax = 0;
  for (int l = 0; l < L; ++l) {
    const nint_layer& ly = layers[l];
    if (!W[l] || !ly.Wf || !ly.Wd || !ly.bias_p || ly.Cx <= 0 || ly.Ch <= 0 || !(ly.k & 1)) return NINT_E_ARG;
    if (ly.Cxp != nint_round_up(ly.xfold ? ly.k * ly.Cx : ly.Cx, kc) || ly.Chp != nint_round_up(ly.Ch, kc) ||
        ly.Ch16 != nint_round_up(ly.Ch, 16))
      return NINT_E_ARG;
    t.e[l] = PackEntry{W[l], bias[l], (void*)ly.Wf, (void*)ly.Wd, (float*)ly.bias_p, ly.Cx, ly.Cxp, ly.Ch, ly.Ch16, ly.Chp, ly.k, ly.xfold};
    const size_t n = 2 * (size_t)(ly.Cxp + ly.Chp) * 4 * ly.Ch16 * ly.k * ly.k + 4 * ly.Ch16 +
                     3 * 32 * (size_t)(nint_stencil_shape(ly.Cx, ly.Ch, ly.k, ly.xfold) ? nint_stencil_rows(ly.Cx, ly.Ch, ly.xfold) : 0) +
                     (nint_tiny_shape(ly.Cx, ly.Ch, ly.k, ly.xfold, dtype) ? (size_t)NINT_TINY_MAXSTEPS * 2 * 64 * (dtype == NINT_BF16 ? 8 : 4) + 4 * NINT_TINY_MAXSTEPS : 0);
    if (n > nmax) nmax = n;
  }
  dim3 grid = grid1d(nmax);
  grid.y = L;
  nint_by_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL(pack_weights_layers_kernel<decltype(dt)::value>, grid, dim3(256), 0, (hipStream_t)stream, t); });
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}
