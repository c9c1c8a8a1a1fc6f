// pointwise.hip -- the HBM-bound kernels around the gate GEMMs: layout conversion at the
// boundary, weight packing into MFMA fragment order, the LSTM pointwise backward, the 1x1
// head, the fused crop+MSE+L1 loss, flat Adam and the fuse/z-score/halo-pad preproc.
// All of them are one-read/one-write streaming kernels; threads walk the channel axis
// fastest so that channels-last slabs are read and written in full cache lines.
#include "nint_common.h"

static inline dim3 grid1d(size_t n, int block = 256) {
  size_t g = (n + block - 1) / block;
  if (g > 256 * 32) g = 256 * 32;   // grid-stride the rest (256 CUs x 32)
  if (g < 1) g = 1;
  return dim3((unsigned)g);
}

// ------------------------------------------------------------------------------ pack / unpack
// (B,T,C,H,W) f32 -> halo slab image t*B+b, interior only (halo/slack stay zero).
// Thread order: channel fastest on the WRITE side (full 64-byte rows); the NCHW read side is
// strided by H*W floats per channel, served from L2 after the first touch of each line.
template <int DT>
__global__ void pack_btchw_kernel(const float* __restrict__ src, void* __restrict__ dst, int B, int T, int C,
                                  int Cp, int H, int W, int P, int Hh, int Wh, int kf) {
  const size_t total = (size_t)B * T * H * W * Cp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = i % Cp;
    size_t r = i / Cp;
    const int x = r % W; r /= W;
    const int y = r % H; r /= H;
    const int b = r % B;
    const int t = r / B;
    // kf > 1: horizontally folded layout, slab channel kx*C + c of pixel x = channel c of pixel x + kx - kf/2 (0 outside)
    const int kx = co / C, c = co - kx * C, xi = x + kx - (kf >> 1);
    const float v = (kx < kf && xi >= 0 && xi < W) ? src[((((size_t)b * T + t) * C + c) * H + y) * W + xi] : 0.f;
    const size_t o = ((((size_t)t * B + b) * Hh + (y + P)) * Wh + (x + P)) * Cp + co;
    store_elem<DT>(dst, o, v);
  }
}

// Stage C rows of W floats (one per channel, each contiguous along x) into the LDS tile [C][ld]: the tile is
// walked as C * (W / VW) vectors of VW floats; a thread issues the loads of U vectors BEFORE the first LDS store, so
// U * 256 independent loads are in flight per workgroup (the rows are read once, from HBM: latency, not issue,
// bounds this loop).  rowfn(c) -> (pointer to the row, mean, std, output channel); ZS = z-score the values.
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
template <int VW> struct RowVec;
template <> struct RowVec<1> { typedef float type; };
template <> struct RowVec<2> { typedef f32x2_t type; };
template <> struct RowVec<4> { typedef f32x4_t type; };
struct RowDesc { const float* p; float mean, sd; int co; };

template <int VW, bool ZS, class RowFn>
__device__ __forceinline__ void stage_rows(float* __restrict__ tile, int ld, int C, int W, RowFn rowfn) {
  typedef typename RowVec<VW>::type V;
  constexpr int U = VW == 4 ? 4 : 8;
  const int WV = W / VW, total = C * WV;
  const unsigned magic = (unsigned)(((1ull << 32) + WV - 1) / WV);   // idx / WV by multiply-high: exact for idx < 65536, WV <= 4096
  const bool small = total < 65536 && WV <= 4096 && WV > 1;           // (a divisor of 1 has no 32-bit magic number: 2^32)
  for (int base = threadIdx.x; base < total; base += 256 * U) {
    V v[U];
    RowDesc d[U];
    int q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * 256;
      if (idx < total) {
        const int c = small ? (int)__umulhi((unsigned)idx, magic) : idx / WV;
        q[u] = idx - c * WV;
        d[u] = rowfn(c);
        v[u] = *(const V*)(d[u].p + q[u] * VW);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (base + u * 256 < total) {
        float* trow = tile + d[u].co * ld + q[u] * VW;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          float f;
          if constexpr (VW == 1) f = v[u]; else f = v[u][e];
          trow[e] = ZS ? (f - d[u].mean) / d[u].sd : f;
        }
      }
    }
  }
}

// write one row of Wo pixels from the tile as 16-byte vectors of 8 (bf16) / 4 (f32) consecutive channels;
// xmap(xo) = tile column of output pixel xo.  kf > 1: HORIZONTALLY FOLDED output (nint_layer.xfold): output channel
// kx*C + c of pixel xo is input channel c of pixel xo + kx - kf/2, zero outside [0, Wo) (the conv's zero padding).
template <int DT, class XMap>
__device__ __forceinline__ void write_row_channels_last(const float* __restrict__ tile, int ld, int C, int Cp, int Wo, char* __restrict__ d,
                                                        XMap xmap, int kf = 1) {
  constexpr int V = 16 / Elem<DT>::ES;         // channels per 16-byte vector
  const int nv = Cp / V;
  const unsigned magic_c = (unsigned)(((1ull << 32) + C - 1) / C);    // co / C by multiply-high (co < 65536)
  for (int i = threadIdx.x; i < Wo * nv; i += 256) {
    const int xo = i / nv, v = i - xo * nv;
    float f[V];
    if (kf <= 1) {
      const int xs = xmap(xo);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int c = v * V + j;
        f[j] = c < C ? tile[c * ld + xs] : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int co = v * V + j;
        const int kx = C == 1 ? co : (int)__umulhi((unsigned)co, magic_c), c = co - kx * C;   // (C = 1: the magic number would be 2^32)
        const int xi = xo + kx - (kf >> 1);
        f[j] = (kx < kf && xi >= 0 && xi < Wo) ? tile[c * ld + xmap(xi)] : 0.f;
      }
    }
    u32x4_t o;
    if constexpr (DT == NINT_BF16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(f[2 * j], f[2 * j + 1]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __builtin_bit_cast(uint32_t, f[j]);
    }
    *(u32x4_t*)(d + ((size_t)xo * Cp + v * V) * Elem<DT>::ES) = o;
  }
}

// Tiled variant: one workgroup per (b, t, y) row.  The NCHW side is read along x (full cache
// lines per channel row), transposed through LDS, and the channels-last side is written as
// 16-byte vectors of 8 (bf16) / 4 (f32) consecutive channels, i.e. whole 64-byte-chunk rows.
template <int DT, int VW>
__global__ __launch_bounds__(256) void pack_btchw_rows_kernel(const float* __restrict__ src, void* __restrict__ dst,
                                                             int B, int T, int C, int Cp, int H, int W, int P, int Hh,
                                                             int Wh, int kf) {
  extern __shared__ float tile[];              // [C][W + 1]
  const int ld = W + 1;
  int r = blockIdx.x;
  const int y = r % H; r /= H;
  const int t = r % T;
  const int b = r / T;
  const float* s = src + (((size_t)b * T + t) * C) * H * W + (size_t)y * W;
  const size_t HW = (size_t)H * W;
  stage_rows<VW, false>(tile, ld, C, W, [&](int c) { return RowDesc{s + c * HW, 0.f, 1.f, c}; });
  __syncthreads();
  char* d = (char*)dst + ((((size_t)t * B + b) * Hh + (y + P)) * Wh + P) * (size_t)Cp * Elem<DT>::ES;
  write_row_channels_last<DT>(tile, ld, C, Cp, W, d, [](int x) { return x; }, kf);
}

template <int DT>
__global__ void unpack_halo_kernel(const void* __restrict__ src, float* __restrict__ dst, int n0, int N, int C,
                                   int Cp, int H, int W, int P, int Hh, int Wh) {
  const size_t total = (size_t)N * C * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int y = r % H; r /= H;
    const int c = r % C;
    const int n = r / C;
    const size_t s = ((((size_t)(n0 + n)) * Hh + (y + P)) * Wh + (x + P)) * Cp + c;
    dst[i] = load_elem<DT>(src, s);
  }
}

template <int DT>
__global__ void pack_compact_kernel(const float* __restrict__ src, void* __restrict__ dst, int N, int C, int Cp,
                                    int H, int W) {
  const size_t total = (size_t)N * H * W * Cp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = i % Cp;
    size_t r = i / Cp;
    const int x = r % W; r /= W;
    const int y = r % H;
    const int n = r / H;
    store_elem<DT>(dst, i, c < C ? src[(((size_t)n * C + c) * H + y) * W + x] : 0.f);
  }
}

template <int DT>
__global__ void unpack_compact_kernel(const void* __restrict__ src, float* __restrict__ dst, int N, int C, int Cp,
                                      int H, int W) {
  const size_t total = (size_t)N * C * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int y = r % H; r /= H;
    const int c = r % C;
    const int n = r / C;
    dst[i] = load_elem<DT>(src, (((size_t)n * H + y) * W + x) * Cp + c);
  }
}

static int pack_btchw_impl(const float* src, void* dst, int B, int T, int C, int kf, int Cp, const nint_geom* g, int dtype,
                           void* stream) {
  if (!src || !dst || !g || B <= 0 || T <= 0 || C <= 0 || Cp < C * kf) return NINT_E_ARG;
  const size_t total = (size_t)B * T * g->H * g->W * Cp;
  hipStream_t st = (hipStream_t)stream;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  const size_t tile_bytes = (size_t)C * (g->W + 1) * sizeof(float);
  if (tile_bytes <= 160 * 1024 && Cp % (dtype == NINT_BF16 ? 8 : 4) == 0) {
    const dim3 grid((unsigned)((size_t)B * T * g->H));
    // widest row vector the alignment of every channel row allows (rows start at multiples of W floats)
    const int vw = ((((uintptr_t)src) & 15) == 0 && g->W % 4 == 0) ? 4 : (((((uintptr_t)src) & 7) == 0 && g->W % 2 == 0) ? 2 : 1);
    // (row tiles above 64 KiB -- 65+ channels on a 1-degree grid -- need the opt-in, as the slab preproc kernel does)
#define NINT_PACK(DT_, VW_) { auto kern = pack_btchw_rows_kernel<DT_, VW_>;                                                                     \
    if (tile_bytes > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes)); \
    hipLaunchKernelGGL(kern, grid, dim3(256), tile_bytes, st, src, dst, B, T, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh, kf); }
    if (dtype == NINT_BF16) { if (vw == 4) NINT_PACK(NINT_BF16, 4) else if (vw == 2) NINT_PACK(NINT_BF16, 2) else NINT_PACK(NINT_BF16, 1) }
    else { if (vw == 4) NINT_PACK(NINT_F32, 4) else if (vw == 2) NINT_PACK(NINT_F32, 2) else NINT_PACK(NINT_F32, 1) }
#undef NINT_PACK
    NINT_LAUNCH_CHECK();
    return NINT_OK;
  }
  // rows that do not fit the LDS tile (or an odd channel padding): one thread per slab element, plain or folded
  if (dtype == NINT_BF16)
    hipLaunchKernelGGL(pack_btchw_kernel<NINT_BF16>, grid1d(total), dim3(256), 0, st, src, dst, B, T, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh, kf);
  else
    hipLaunchKernelGGL(pack_btchw_kernel<NINT_F32>, grid1d(total), dim3(256), 0, st, src, dst, B, T, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh, kf);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_pack_btchw(const float* src, void* dst, int B, int T, int C, int Cp, const nint_geom* g,
                               int dtype, void* stream) {
  return pack_btchw_impl(src, dst, B, T, C, 1, Cp, g, dtype, stream);
}

extern "C" int nint_pack_btchw_xfold(const float* src, void* dst, int B, int T, int C, int k, int Cp, const nint_geom* g,
                                     int dtype, void* stream) {
  if (k < 1 || !(k & 1)) return NINT_E_ARG;
  return pack_btchw_impl(src, dst, B, T, C, k, Cp, g, dtype, stream);
}

// d/dx from the gradient of a horizontally folded input: dx[n][c][y][x] = sum_kx dfold[n][y][x - kx + k/2][kx*C + c]
template <int DT>
__global__ void unfold_dx_kernel(const void* __restrict__ src, float* __restrict__ dst, int N, int C, int k, int Cp, int H, int W) {
  const size_t total = (size_t)N * C * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int y = r % H; r /= H;
    const int c = r % C;
    const int n = r / C;
    float acc = 0.f;
    for (int kx = 0; kx < k; ++kx) {
      const int xs = x - kx + k / 2;
      if (xs >= 0 && xs < W) acc += load_elem<DT>(src, (((size_t)n * H + y) * W + xs) * Cp + kx * C + c);
    }
    dst[i] = acc;
  }
}

extern "C" int nint_unfold_dx(const void* src, float* dst, int N, int C, int k, int Cp, int H, int W, int dtype, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0 || k < 1 || !(k & 1) || Cp < k * C || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  if (dtype == NINT_BF16)
    hipLaunchKernelGGL(unfold_dx_kernel<NINT_BF16>, grid1d((size_t)N * C * H * W), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, k, Cp, H, W);
  else
    hipLaunchKernelGGL(unfold_dx_kernel<NINT_F32>, grid1d((size_t)N * C * H * W), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, k, Cp, H, W);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_unpack_halo(const void* src, float* dst, int n0, int N, int C, int Cp, const nint_geom* g,
                                int dtype, void* stream) {
  if (!src || !dst || !g || N <= 0 || C <= 0 || Cp < C || n0 < 0) return NINT_E_ARG;
  const size_t total = (size_t)N * C * g->H * g->W;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == NINT_BF16)
    hipLaunchKernelGGL(unpack_halo_kernel<NINT_BF16>, grid1d(total), dim3(256), 0, st, src, dst, n0, N, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh);
  else if (dtype == NINT_F32)
    hipLaunchKernelGGL(unpack_halo_kernel<NINT_F32>, grid1d(total), dim3(256), 0, st, src, dst, n0, N, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh);
  else
    return NINT_E_ARG;
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_pack_compact(const float* src, void* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0 || Cp < C || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  if (dtype == NINT_BF16)
    hipLaunchKernelGGL(pack_compact_kernel<NINT_BF16>, grid1d((size_t)N * H * W * Cp), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, Cp, H, W);
  else
    hipLaunchKernelGGL(pack_compact_kernel<NINT_F32>, grid1d((size_t)N * H * W * Cp), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, Cp, H, W);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_unpack_compact(const void* src, float* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0 || Cp < C || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  if (dtype == NINT_BF16)
    hipLaunchKernelGGL(unpack_compact_kernel<NINT_BF16>, grid1d((size_t)N * C * H * W), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, Cp, H, W);
  else
    hipLaunchKernelGGL(unpack_compact_kernel<NINT_F32>, grid1d((size_t)N * C * H * W), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, Cp, H, W);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

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
  hipStream_t st = (hipStream_t)stream;
  if (dtype == NINT_BF16)
    hipLaunchKernelGGL(pack_weights_kernel<NINT_BF16>, grid1d(n), dim3(256), 0, st, W, bias, Wf, Wd, bias_p, Cx, Cxp, Ch, Ch16, Chp, k, xfold);
  else
    hipLaunchKernelGGL(pack_weights_kernel<NINT_F32>, grid1d(n), dim3(256), 0, st, W, bias, Wf, Wd, bias_p, Cx, Cxp, Ch, Ch16, Chp, k, xfold);
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
  if (dtype == NINT_BF16) hipLaunchKernelGGL(pack_weights_layers_kernel<NINT_BF16>, grid, dim3(256), 0, (hipStream_t)stream, t);
  else hipLaunchKernelGGL(pack_weights_layers_kernel<NINT_F32>, grid, dim3(256), 0, (hipStream_t)stream, t);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// ------------------------------------------------------------------------------ LSTM pointwise backward
// Per (pixel, hidden channel), SURVEY.md section 8 a-5 / autograd of model.py:223-229:
//   tc = tanh(c'), do = dh*tc, dc += dh*o*(1-tc^2), di = dc*g, df = dc*c, dg = dc*i, dc_prev = dc*f
//   dGi = di*i*(1-i), dGf = df*f*(1-f), dGg = dg*(1-g^2), dGo = do*o*(1-o)
// Reads the gate stash and dh (ET), c_prev / c_new / dc (f32); writes dG into its halo slab (ET,
// interior only) and dc_prev in place.  One thread per (pixel, channel), channel fastest.
// 4 consecutive elements as f32 (16-byte f32 / 8-byte bf16 vector load); i must be a multiple of 4
// One thread per (pixel, 4 consecutive hidden channels): every access is a 16-byte (f32) or 8-byte
// (bf16) vector.  (The bias gradient, the column sums of dG, is produced by the weight-gradient kernel, which has the
// dG fragments in registers anyway: wgrad.hip.)
template <int DT>
__global__ __launch_bounds__(256) void lstm_bwd_pointwise_kernel(PwArgs a) {
  lstm_bwd_pointwise_body<DT>(a, blockIdx.x, gridDim.x);       // (nint_common.h: the body is also a problem of conv_bwd_multi_kernel)
}

int nint_internal_pointwise_plan(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* gates,
                                 const float* c_prev, const float* c_new, const void* dh, float* dc, void* dG,
                                 bool dc_zero, const void* dh2, PwArgs* plan) {
  if (!ly || !g || !gates || !c_new || !dh || !dc || !dG || N <= 0) return NINT_E_ARG;
  if (dtype != NINT_F32 && dtype != NINT_BF16) return NINT_E_ARG;
  *plan = PwArgs{gates, c_prev, c_new, dh, dh2, dc, dG, N, g->H, g->W, g->P, g->Hh, g->Wh, ly->Ch16, ly->Chp, dc_zero ? 1 : 0};
  return NINT_OK;
}

int nint_internal_pointwise_enqueue(const PwArgs* a, int dtype, void* stream) {
  const size_t total = (size_t)a->N * a->H * a->W * (a->Ch16 / 4);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = grid1d(total);
  if (dtype == NINT_BF16) hipLaunchKernelGGL((lstm_bwd_pointwise_kernel<NINT_BF16>), grid, dim3(256), 0, st, *a);
  else hipLaunchKernelGGL((lstm_bwd_pointwise_kernel<NINT_F32>), grid, dim3(256), 0, st, *a);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_cell_bwd_pointwise(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* gates,
                                       const float* c_prev, const float* c_new, const void* dh, float* dc, void* dG,
                                       void* stream) {
  PwArgs a;
  const int rc = nint_internal_pointwise_plan(ly, g, dtype, N, gates, c_prev, c_new, dh, dc, dG, false, nullptr, &a);
  return rc != NINT_OK ? rc : nint_internal_pointwise_enqueue(&a, dtype, stream);
}

// ------------------------------------------------------------------------------ 1x1 head
// pred[n][o][y][x] = b[o] + sum_c w[o][c] * h[n][y][x][c]     (model.py:251,274)
// One thread per pixel: the channel vector is read once (16-byte loads), the weights are wave-uniform
// (scalar loads), and every output plane is written coalesced along x.  CHV = channels held in registers.
// The weights are staged once per workgroup in LDS, zero-padded to [O][CHV]: the inner loop is then broadcast LDS reads and
// FMAs with no bounds test (a predicate on the run-time channel count made every FMA a branch and a scalar load with its
// own wait: 176 s_load_dword / 364 branches in the 32-channel instance).  The padding terms add +0.
template <int CHV>
__device__ __forceinline__ void head_stage_weights(float* w_s, const float* __restrict__ w, int O, int Ch) {
  for (int i = threadIdx.x; i < O * CHV; i += blockDim.x) {
    const int o = i / CHV, c = i - o * CHV;
    w_s[i] = c < Ch ? w[o * Ch + c] : 0.f;
  }
  __syncthreads();
}

// The sequence entries (nint_head_fwd_seq and its kin) run the same bodies over all T*B images of the top layer's slab; only the
// plane index of the (B, T*O, H, W) tensors differs: image n = t*B + b (time-major, as everywhere inside the library) owns the
// O planes from (b*T + t)*O.  SEQ = false (Bs unused): plane block n, the (N, O, H, W) tensors of the one-step entries.
template <bool SEQ>
__device__ __forceinline__ size_t head_image(size_t n, int Bs, int T) {
  if constexpr (SEQ) return (n % (size_t)Bs) * T + n / (size_t)Bs;
  else return n;
}

template <int DT, int CHV, bool SEQ>
__device__ __forceinline__ void head_fwd_body(float* w_s, const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                              const float* __restrict__ w, const float* __restrict__ b,
                                              float* __restrict__ pred, int H, int W, int P, int Hh, int Wh, int Bs) {
  head_stage_weights<CHV>(w_s, w, O, Ch);
  const size_t npix = (size_t)N * H * W;
  const size_t pix = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const int x = pix % W;
  size_t r = pix / W;
  const int y = r % H;
  const int n = r / H;
  const size_t hb = ((((size_t)(n0 + n)) * Hh + (y + P)) * Wh + (x + P)) * Chp;
  float hv[CHV];
#pragma unroll
  for (int c = 0; c < CHV; c += 4) {
    const f32x4_t v = (c < Chp) ? load_vec4<DT>(h, hb + c) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
    hv[c] = v[0]; hv[c + 1] = v[1]; hv[c + 2] = v[2]; hv[c + 3] = v[3];
  }
  float* out = pred + (head_image<SEQ>(n, Bs, N / (SEQ ? Bs : 1)) * O * H + y) * W + x;
  for (int o = 0; o < O; ++o) {
    float acc = b ? b[o] : 0.f;
    const f32x4_t* wr = (const f32x4_t*)(w_s + o * CHV);
#pragma unroll
    for (int c = 0; c < CHV; c += 4) {
      const f32x4_t wv = wr[c / 4];
      acc += wv[0] * hv[c]; acc += wv[1] * hv[c + 1]; acc += wv[2] * hv[c + 2]; acc += wv[3] * hv[c + 3];
    }
    out[(size_t)o * H * W] = acc;
  }
}

template <int DT, int CHV>
__global__ __launch_bounds__(256) void head_fwd_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ pred, int H, int W, int P, int Hh, int Wh) {
  extern __shared__ __attribute__((aligned(16))) char smem_hf[];
  head_fwd_body<DT, CHV, false>((float*)smem_hf, h, n0, N, Ch, Chp, O, w, b, pred, H, W, P, Hh, Wh, 0);
}

template <int DT, int CHV>
__global__ __launch_bounds__(256) void head_fwd_seq_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                           const float* __restrict__ w, const float* __restrict__ b,
                                                           float* __restrict__ seq, int H, int W, int P, int Hh, int Wh, int Bs) {
  extern __shared__ __attribute__((aligned(16))) char smem_hfs[];
  head_fwd_body<DT, CHV, true>((float*)smem_hfs, h, n0, N, Ch, Chp, O, w, b, seq, H, W, P, Hh, Wh, Bs);
}

// generic widths: one thread per output element
template <int DT, bool SEQ>
__device__ __forceinline__ void head_fwd_wide_body(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                   const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ pred,
                                                   int H, int W, int P, int Hh, int Wh, int Bs) {
  const size_t total = (size_t)N * O * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int y = r % H; r /= H;
    const int o = r % O;
    const int n = r / O;
    const size_t hb = ((((size_t)(n0 + n)) * Hh + (y + P)) * Wh + (x + P)) * Chp;
    float acc = b ? b[o] : 0.f;
    for (int c = 0; c < Ch; ++c) acc += w[o * Ch + c] * load_elem<DT>(h, hb + c);
    if constexpr (SEQ) pred[((head_image<true>(n, Bs, N / Bs) * O + o) * H + y) * W + x] = acc;
    else pred[i] = acc;
  }
}

template <int DT>
__global__ void head_fwd_wide_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                     const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ pred,
                                     int H, int W, int P, int Hh, int Wh) {
  head_fwd_wide_body<DT, false>(h, n0, N, Ch, Chp, O, w, b, pred, H, W, P, Hh, Wh, 0);
}

template <int DT>
__global__ void head_fwd_wide_seq_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                         const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ seq,
                                         int H, int W, int P, int Hh, int Wh, int Bs) {
  head_fwd_wide_body<DT, true>(h, n0, N, Ch, Chp, O, w, b, seq, H, W, P, Hh, Wh, Bs);
}

// d loss / d (head output) of image n (time-major), output o, pixel yx, for the backward kernels below.  DpPlain: the (N, O, H, W)
// tensor of the one-step entries.  DpSeq: dseq (B, T*O, H, W) and / or the cotangent of pred = head(h_{T-1}) (B, O, H, W), which
// joins step T-1 here; either may be nullptr.
struct DpPlain {
  const float* __restrict__ p; int O; size_t HW;
  __device__ __forceinline__ float operator()(size_t n, int o, size_t yx) const { return p[(n * O + o) * HW + yx]; }
};
struct DpSeq {
  const float* __restrict__ dseq; const float* __restrict__ dlast; int O, B, T; size_t HW;
  __device__ __forceinline__ float operator()(size_t n, int o, size_t yx) const {
    const size_t t = n / (size_t)B, b = n - t * B;
    float d = dseq ? dseq[((b * T + t) * O + o) * HW + yx] : 0.f;
    if (dlast && t == (size_t)(T - 1)) d += dlast[(b * O + o) * HW + yx];
    return d;
  }
};

// dh[n][y][x][c] = sum_o w[o][c] * dpred[n][o][y][x].  One thread per pixel (dpred planes read coalesced
// along x, weights wave-uniform), the padded channel vector is written with 16-byte stores.
template <int DT, int CHV, class Dp>
__device__ __forceinline__ void head_bwd_dh_body(float* w_s, const float* __restrict__ w, const Dp dpred,
                                                 void* __restrict__ dh, int N, int Ch, int Chp, int O, int H, int W) {
  head_stage_weights<CHV>(w_s, w, O, Ch);
  const size_t npix = (size_t)N * H * W;
  const size_t pix = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const size_t yx = pix % ((size_t)H * W);
  const size_t n = pix / ((size_t)H * W);
  float acc[CHV];
#pragma unroll
  for (int c = 0; c < CHV; ++c) acc[c] = 0.f;
  for (int o = 0; o < O; ++o) {
    const float d = dpred(n, o, yx);
    const f32x4_t* wr = (const f32x4_t*)(w_s + o * CHV);
#pragma unroll
    for (int c = 0; c < CHV; c += 4) {
      const f32x4_t wv = wr[c / 4];
      acc[c] += wv[0] * d; acc[c + 1] += wv[1] * d; acc[c + 2] += wv[2] * d; acc[c + 3] += wv[3] * d;
    }
  }
#pragma unroll
  for (int c = 0; c < CHV; c += 4)
    if (c < Chp) store_vec4<DT>(dh, pix * Chp + c, (f32x4_t){acc[c], acc[c + 1], acc[c + 2], acc[c + 3]});
}

template <int DT, int CHV>
__global__ __launch_bounds__(256) void head_bwd_dh_kernel(const float* __restrict__ w, const float* __restrict__ dpred,
                                                          void* __restrict__ dh, int N, int Ch, int Chp, int O, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) char smem_hd[];
  head_bwd_dh_body<DT, CHV>((float*)smem_hd, w, DpPlain{dpred, O, (size_t)H * W}, dh, N, Ch, Chp, O, H, W);
}

template <int DT, int CHV>
__global__ __launch_bounds__(256) void head_bwd_dh_seq_kernel(const float* __restrict__ w, DpSeq dpred, void* __restrict__ dh,
                                                              int N, int Ch, int Chp, int O, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) char smem_hds[];
  head_bwd_dh_body<DT, CHV>((float*)smem_hds, w, dpred, dh, N, Ch, Chp, O, H, W);
}

template <int DT, class Dp>
__device__ __forceinline__ void head_bwd_dh_wide_body(const float* __restrict__ w, const Dp dpred, void* __restrict__ dh,
                                                      int N, int Ch, int Chp, int O, int H, int W) {
  const size_t total = (size_t)N * H * W * Chp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = i % Chp;
    const size_t pix = i / Chp;
    const size_t yx = pix % ((size_t)H * W);
    const int n = pix / ((size_t)H * W);
    float acc = 0.f;
    if (c < Ch)
      for (int o = 0; o < O; ++o) acc += w[o * Ch + c] * dpred((size_t)n, o, yx);
    store_elem<DT>(dh, i, acc);
  }
}

template <int DT>
__global__ void head_bwd_dh_wide_kernel(const float* __restrict__ w, const float* __restrict__ dpred, void* __restrict__ dh,
                                        int N, int Ch, int Chp, int O, int H, int W) {
  head_bwd_dh_wide_body<DT>(w, DpPlain{dpred, O, (size_t)H * W}, dh, N, Ch, Chp, O, H, W);
}

template <int DT>
__global__ void head_bwd_dh_wide_seq_kernel(const float* __restrict__ w, DpSeq dpred, void* __restrict__ dh,
                                            int N, int Ch, int Chp, int O, int H, int W) {
  head_bwd_dh_wide_body<DT>(w, dpred, dh, N, Ch, Chp, O, H, W);
}

// dw[o][c] = sum_pixels dpred*h ; db[o] = sum dpred.  One workgroup per (o, c-or-bias) output,
// fixed-order tree reduction -> bitwise reproducible.
template <int DT, class Dp>
__device__ __forceinline__ void head_bwd_dw_body(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                 int O, const Dp dpred,
                                                 float* __restrict__ dw, float* __restrict__ db, int H, int W,
                                                 int P, int Hh, int Wh) {
  const int o = blockIdx.x / (Ch + 1);
  const int c = blockIdx.x % (Ch + 1);   // c == Ch -> bias
  const size_t npix = (size_t)N * H * W;
  float acc = 0.f;
  for (size_t i = threadIdx.x; i < npix; i += blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int y = r % H;
    const int n = r / H;
    const float d = dpred((size_t)n, o, (size_t)y * W + x);
    if (c < Ch) {
      const size_t hb = ((((size_t)(n0 + n)) * Hh + (y + P)) * Wh + (x + P)) * Chp + c;
      acc += d * load_elem<DT>(h, hb);
    } else {
      acc += d;
    }
  }
  __shared__ float red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (c < Ch) dw[o * Ch + c] = red[0];
    else db[o] = red[0];
  }
}

template <int DT>
__global__ __launch_bounds__(256) void head_bwd_dw_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                          int O, const float* __restrict__ dpred,
                                                          float* __restrict__ dw, float* __restrict__ db, int H, int W,
                                                          int P, int Hh, int Wh) {
  head_bwd_dw_body<DT>(h, n0, N, Ch, Chp, O, DpPlain{dpred, O, (size_t)H * W}, dw, db, H, W, P, Hh, Wh);
}

template <int DT>
__global__ __launch_bounds__(256) void head_bwd_dw_seq_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                              int O, DpSeq dpred, float* __restrict__ dw, float* __restrict__ db,
                                                              int H, int W, int P, int Hh, int Wh) {
  head_bwd_dw_body<DT>(h, n0, N, Ch, Chp, O, dpred, dw, db, H, W, P, Hh, Wh);
}

// Tiled path (O*(Ch+1) <= HEAD_DW_NK*512 outputs): every workgroup owns a pixel range, stages `stage` pixels of dpred and
// h in LDS at a time (ONE HBM round trip per stage: the launch is latency-bound, 14 MB in all for the bench's head), thread
// i accumulates the outputs i, i+512, ... over the range; per-workgroup partials are folded in fixed order by
// head_bwd_dw_final_kernel.  The grid is one workgroup per HEAD_DW_PIX pixels, as far as the caller's scratch goes.
// (Wide heads -- 128 hidden channels, or 200 outputs -- used to fall to head_bwd_dw_kernel: one workgroup per output walking
// every pixel with a 4-byte strided read, 2.5 ms per step for configs[3].)
#define HEAD_DW_PIX 240
#define HEAD_DW_NK 8
#define HEAD_DW_LDS_FLOATS (15 * 1024)
template <int DT, class Dp>
__device__ __forceinline__ void head_bwd_dw_tiled_body(float* smem_dw, const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                       int O, const Dp dpred,
                                                       float* __restrict__ partial, int H, int W, int P, int Hh,
                                                       int Wh, int stage) {
  const int SO = O | 1, SC = (Ch + 1) | 1;     // odd row strides: the staging writes walk pixels without bank conflicts
  float* sd = smem_dw;                         // [pixel][o]
  float* sh = smem_dw + stage * SO;            // [pixel][c] + a constant 1 for the bias column
  const int nout = O * (Ch + 1);
  int oo_[HEAD_DW_NK], cc_[HEAD_DW_NK];
  float acc[HEAD_DW_NK];
#pragma unroll
  for (int k = 0; k < HEAD_DW_NK; ++k) {
    const int i = min((int)threadIdx.x + 512 * k, nout - 1);
    oo_[k] = i / (Ch + 1); cc_[k] = i % (Ch + 1); acc[k] = 0.f;
  }
  const int nk = (nout + 511) / 512;
  const size_t npix = (size_t)N * H * W;
  const size_t per = (npix + gridDim.x - 1) / gridDim.x;
  const size_t p0 = blockIdx.x * per, p1 = min(npix, p0 + per);
  const int nq = (Ch + 3) / 4;                 // channel quads of a pixel (Chp is a multiple of 16: the vector load stays inside)
  for (size_t base = p0; base < p1; base += stage) {
    const int cnt = (int)min((size_t)stage, p1 - base);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * O; i += 512) {        // dpred planes: consecutive threads walk consecutive pixels
      const int oo = i / cnt, pp = i - oo * cnt;
      const size_t pix = base + pp;
      const size_t yx = pix % ((size_t)H * W);
      const size_t n = pix / ((size_t)H * W);
      sd[pp * SO + oo] = dpred(n, oo, yx);
    }
    for (int i = threadIdx.x; i < cnt * nq; i += 512) {       // h: one 4-channel vector per thread
      const int pp = i / nq, q = i - pp * nq;
      const size_t pix = base + pp;
      const int x = pix % W;
      size_t r = pix / W;
      const int y = r % H;
      const int n = r / H;
      const f32x4_t v = load_vec4<DT>(h, ((((size_t)(n0 + n)) * Hh + (y + P)) * Wh + (x + P)) * Chp + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < Ch) sh[pp * SC + 4 * q + e] = v[e];
      if (q == 0) sh[pp * SC + Ch] = 1.f;
    }
    __syncthreads();
    if (nk == 1) {
      if ((int)threadIdx.x < nout) {
#pragma unroll 8
        for (int pp = 0; pp < cnt; ++pp) acc[0] += sd[pp * SO + oo_[0]] * sh[pp * SC + cc_[0]];
      }
    } else {
      for (int pp = 0; pp < cnt; ++pp) {
#pragma unroll
        for (int k = 0; k < HEAD_DW_NK; ++k)
          if (k < nk) acc[k] += sd[pp * SO + oo_[k]] * sh[pp * SC + cc_[k]];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < HEAD_DW_NK; ++k)
    if ((int)threadIdx.x + 512 * k < nout) partial[(size_t)blockIdx.x * nout + threadIdx.x + 512 * k] = acc[k];
}

template <int DT>
__global__ __launch_bounds__(512) void head_bwd_dw_tiled_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                              int O, const float* __restrict__ dpred,
                                                              float* __restrict__ partial, int H, int W, int P, int Hh,
                                                              int Wh, int stage) {
  extern __shared__ __attribute__((aligned(16))) float smem_dw[];
  head_bwd_dw_tiled_body<DT>(smem_dw, h, n0, N, Ch, Chp, O, DpPlain{dpred, O, (size_t)H * W}, partial, H, W, P, Hh, Wh, stage);
}

template <int DT>
__global__ __launch_bounds__(512) void head_bwd_dw_tiled_seq_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                                  int O, DpSeq dpred, float* __restrict__ partial, int H, int W,
                                                                  int P, int Hh, int Wh, int stage) {
  extern __shared__ __attribute__((aligned(16))) float smem_dw[];
  head_bwd_dw_tiled_body<DT>(smem_dw, h, n0, N, Ch, Chp, O, dpred, partial, H, W, P, Hh, Wh, stage);
}

// Larger heads (more than 512 outputs, and the smaller of O and Ch + 1 at most 32 -- 200 outputs x 16 channels, or 20 x
// 128): REGISTER-tiled.  The smaller dimension ("R") lives in registers, a thread owns one index of the larger one ("T")
// and NH = 512 / T pixel strides: per staged pixel it reads its own T value once and the R values as broadcast 16-byte reads
// -- 1 + R/4 LDS instructions per R FMAs instead of 2 per FMA.  The NH partial sums of an output are folded through LDS in
// fixed order; the slab layout is head_bwd_dw_tiled_kernel's.
template <int DT, class Dp>
__device__ __forceinline__ void head_bwd_dw_rtile_body(float* smem_dw, const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                       int O, const Dp dpred,
                                                       float* __restrict__ partial, int H, int W, int P, int Hh,
                                                       int Wh, int stage) {
  const int C1 = Ch + 1;
  const bool r_is_c = C1 <= O;                 // registers over the channels (+ bias), threads over the outputs -- or the other way round
  const int R = r_is_c ? C1 : O, T = r_is_c ? O : C1;
  const int SR = (R + 3) & ~3, ST = T | 1;     // row strides: 16-byte rows for the broadcast reads, odd for the per-thread ones
  float* sr = smem_dw;                         // [pixel][R]
  float* st = smem_dw + stage * SR;            // [pixel][T]
  float* sd = r_is_c ? st : sr;                // dpred [pixel][o]
  float* sh = r_is_c ? sr : st;                // h     [pixel][c] + 1
  const int SD = r_is_c ? ST : SR, SH = r_is_c ? SR : ST;
  const int nout = O * C1;
  const int NH = min(8, 512 / T);
  const int ti = threadIdx.x % T, hf = threadIdx.x / T;
  const bool act = hf < NH;
  float acc[32];
#pragma unroll
  for (int r = 0; r < 32; ++r) acc[r] = 0.f;
  const size_t npix = (size_t)N * H * W;
  const size_t per = (npix + gridDim.x - 1) / gridDim.x;
  const size_t p0 = blockIdx.x * per, p1 = min(npix, p0 + per);
  const int nq = (Ch + 3) / 4;
  for (size_t base = p0; base < p1; base += stage) {
    const int cnt = (int)min((size_t)stage, p1 - base);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * O; i += 512) {        // dpred planes: consecutive threads walk consecutive pixels
      const int oo = i / cnt, pp = i - oo * cnt;
      const size_t pix = base + pp;
      const size_t yx = pix % ((size_t)H * W);
      const size_t n = pix / ((size_t)H * W);
      sd[pp * SD + oo] = dpred(n, oo, yx);
    }
    for (int i = threadIdx.x; i < cnt * nq; i += 512) {       // h: one 4-channel vector per thread
      const int pp = i / nq, q = i - pp * nq;
      const size_t pix = base + pp;
      const int x = pix % W;
      size_t r = pix / W;
      const int y = r % H;
      const int n = r / H;
      const f32x4_t v = load_vec4<DT>(h, ((((size_t)(n0 + n)) * Hh + (y + P)) * Wh + (x + P)) * Chp + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < Ch) sh[pp * SH + 4 * q + e] = v[e];
      if (q == 0) sh[pp * SH + Ch] = 1.f;
    }
    if (SR > R) for (int i = threadIdx.x; i < cnt; i += 512)   // the tail of the 16-byte rows feeds accumulators that are never stored: keep it finite
      for (int r = R; r < SR; ++r) sr[i * SR + r] = 0.f;
    __syncthreads();
    if (act) {
      for (int pp = hf; pp < cnt; pp += NH) {
        const float tv = st[pp * ST + ti];
        const f32x4_t* rr = (const f32x4_t*)(sr + pp * SR);
#pragma unroll
        for (int r4 = 0; r4 < 8; ++r4) {
          if (4 * r4 < SR) {
            const f32x4_t rv = rr[r4];
            acc[4 * r4] += tv * rv[0]; acc[4 * r4 + 1] += tv * rv[1]; acc[4 * r4 + 2] += tv * rv[2]; acc[4 * r4 + 3] += tv * rv[3];
          }
        }
      }
    }
  }
  // fold the NH pixel strides of every output (fixed order) through LDS: red[hf][ti][r]
  __syncthreads();
  float* red = smem_dw;                        // NH * T * SR floats (the launch reserves the larger of this and the staging buffers)
  if (act) {
#pragma unroll
    for (int r = 0; r < 32; ++r)
      if (r < R) red[((size_t)hf * T + ti) * SR + r] = acc[r];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nout; i += 512) {
    const int o = i / C1, c = i - o * C1;
    const int t2 = r_is_c ? o : c, r2 = r_is_c ? c : o;
    float s = 0.f;
    for (int q = 0; q < NH; ++q) s += red[((size_t)q * T + t2) * SR + r2];
    partial[(size_t)blockIdx.x * nout + i] = s;
  }
}

template <int DT>
__global__ __launch_bounds__(512) void head_bwd_dw_rtile_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                              int O, const float* __restrict__ dpred,
                                                              float* __restrict__ partial, int H, int W, int P, int Hh,
                                                              int Wh, int stage) {
  extern __shared__ __attribute__((aligned(16))) float smem_dw[];
  head_bwd_dw_rtile_body<DT>(smem_dw, h, n0, N, Ch, Chp, O, DpPlain{dpred, O, (size_t)H * W}, partial, H, W, P, Hh, Wh, stage);
}

template <int DT>
__global__ __launch_bounds__(512) void head_bwd_dw_rtile_seq_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                                  int O, DpSeq dpred, float* __restrict__ partial, int H, int W,
                                                                  int P, int Hh, int Wh, int stage) {
  extern __shared__ __attribute__((aligned(16))) float smem_dw[];
  head_bwd_dw_rtile_body<DT>(smem_dw, h, n0, N, Ch, Chp, O, dpred, partial, H, W, P, Hh, Wh, stage);
}

// block = 64 outputs x blockDim/64 lanes over the per-workgroup partials; fixed order
__global__ void head_bwd_dw_final_kernel(const float* __restrict__ partial, int nblocks, int Ch, int O,
                                         float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[1024];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6, G = blockDim.x >> 6;
  const int nout = O * (Ch + 1);
  float s = 0.f;
  if (i < nout) {
#pragma unroll 4
    for (int b = sub; b < nblocks; b += G) s += partial[(size_t)b * nout + i];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (sub != 0 || i >= nout) return;
  for (int q = 1; q < G; ++q) s += red[q * 64 + (threadIdx.x & 63)];
  const int o = i / (Ch + 1), c = i % (Ch + 1);
  if (c < Ch) dw[o * Ch + c] = s;
  else db[o] = s;
}

// sq != nullptr: the sequence entry (n0 = B, N = T*B, plane blocks b*T + t)
static int head_fwd_impl(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b, float* pred,
                         const nint_geom* g, int dtype, int Bs, void* stream) {
  const size_t total = (size_t)N * O * g->H * g->W, npix = (size_t)N * g->H * g->W;
  hipStream_t st = (hipStream_t)stream;
  const dim3 gp((unsigned)((npix + 255) / 256));
  const size_t w_lds = (size_t)O * (Chp <= 32 ? 32 : (Chp <= 64 ? 64 : 128)) * sizeof(float);      // staged weights [O][CHV]
  if (Chp <= 128 && Chp % 4 == 0 && w_lds <= 64 * 1024) {
#define NINT_HF(DT_, CHV_) { if (Bs) hipLaunchKernelGGL((head_fwd_seq_kernel<DT_, CHV_>), gp, dim3(256), w_lds, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh, Bs); \
                             else hipLaunchKernelGGL((head_fwd_kernel<DT_, CHV_>), gp, dim3(256), w_lds, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh); }
    if (dtype == NINT_BF16) { if (Chp <= 32) NINT_HF(NINT_BF16, 32) else if (Chp <= 64) NINT_HF(NINT_BF16, 64) else NINT_HF(NINT_BF16, 128) }
    else { if (Chp <= 32) NINT_HF(NINT_F32, 32) else if (Chp <= 64) NINT_HF(NINT_F32, 64) else NINT_HF(NINT_F32, 128) }
#undef NINT_HF
  } else if (dtype == NINT_BF16) {
    if (Bs) hipLaunchKernelGGL(head_fwd_wide_seq_kernel<NINT_BF16>, grid1d(total), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh, Bs);
    else hipLaunchKernelGGL(head_fwd_wide_kernel<NINT_BF16>, grid1d(total), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh);
  } else {
    if (Bs) hipLaunchKernelGGL(head_fwd_wide_seq_kernel<NINT_F32>, grid1d(total), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh, Bs);
    else hipLaunchKernelGGL(head_fwd_wide_kernel<NINT_F32>, grid1d(total), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh);
  }
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_head_fwd(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                             const float* b, float* pred, const nint_geom* g, int dtype, void* stream) {
  if (!h_slab || !w || !pred || !g || N <= 0 || O <= 0 || Ch <= 0) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  return head_fwd_impl(h_slab, n0, N, Ch, Chp, O, w, b, pred, g, dtype, 0, stream);
}

// channel padding of a slab the head reads: KC of the storage type (nint.h), so every 16-byte channel vector stays inside
static bool head_seq_args_ok(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const nint_geom* g, int dtype) {
  if (!h_slab || !w || !g || B <= 0 || T <= 0 || O <= 0 || Ch <= 0 || Chp < Ch) return false;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return false;
  if (g->H <= 0 || g->W <= 0 || g->P < 0 || g->Hh < g->H + 2 * g->P || g->Wh < g->W + 2 * g->P) return false;
  return Chp % (dtype == NINT_BF16 ? 32 : 16) == 0;
}

extern "C" int nint_head_fwd_seq(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                 float* seq, const nint_geom* g, int dtype, void* stream) {
  if (!seq || !head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if ((((uintptr_t)h_slab) & 15) != 0) return NINT_E_ALIGN;
  return head_fwd_impl(h_slab, B, T * B, Ch, Chp, O, w, b, seq, g, dtype, B, stream);     // h_t = slot t + 1: images from B
}

// sq != nullptr: d loss / d (head output) comes from the sequence tensors (DpSeq) instead of dpred
static int head_bwd_impl(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                         const float* dpred, const DpSeq* sq, void* dh, float* dw, float* db, const nint_geom* g, int dtype,
                         float* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t npix = (size_t)N * g->H * g->W;
  const bool b16 = dtype == NINT_BF16;
  if (dh) {
    const dim3 gp((unsigned)((npix + 255) / 256));
    const size_t w_lds = (size_t)O * (Chp <= 32 ? 32 : (Chp <= 64 ? 64 : 128)) * sizeof(float);    // staged weights [O][CHV]
#define NINT_HD(DT_, CHV_) { if (sq) hipLaunchKernelGGL((head_bwd_dh_seq_kernel<DT_, CHV_>), gp, dim3(256), w_lds, st, w, *sq, dh, N, Ch, Chp, O, g->H, g->W); \
                             else hipLaunchKernelGGL((head_bwd_dh_kernel<DT_, CHV_>), gp, dim3(256), w_lds, st, w, dpred, dh, N, Ch, Chp, O, g->H, g->W); }
#define NINT_HDW(DT_) { if (sq) hipLaunchKernelGGL(head_bwd_dh_wide_seq_kernel<DT_>, grid1d(npix * Chp), dim3(256), 0, st, w, *sq, dh, N, Ch, Chp, O, g->H, g->W); \
                        else hipLaunchKernelGGL(head_bwd_dh_wide_kernel<DT_>, grid1d(npix * Chp), dim3(256), 0, st, w, dpred, dh, N, Ch, Chp, O, g->H, g->W); }
    if (w_lds > 64 * 1024) {
      if (b16) NINT_HDW(NINT_BF16) else NINT_HDW(NINT_F32)
    } else if (Chp <= 32 && Chp % 4 == 0) {
      if (b16) NINT_HD(NINT_BF16, 32) else NINT_HD(NINT_F32, 32)
    } else if (Chp <= 64 && Chp % 4 == 0) {
      if (b16) NINT_HD(NINT_BF16, 64) else NINT_HD(NINT_F32, 64)
    } else if (Chp <= 128 && Chp % 4 == 0) {
      if (b16) NINT_HD(NINT_BF16, 128) else NINT_HD(NINT_F32, 128)
    } else {
      if (b16) NINT_HDW(NINT_BF16) else NINT_HDW(NINT_F32)
    }
#undef NINT_HD
#undef NINT_HDW
    NINT_LAUNCH_CHECK();
  }
  const int nout = O * (Ch + 1);
  const int row_floats = (O | 1) + ((Ch + 1) | 1);
  const int Rd = O < Ch + 1 ? O : Ch + 1, Td = O < Ch + 1 ? Ch + 1 : O;      // register / thread dimension of the register-tiled kernel
  // the two-stage kernels: KERN_ for the one-step entry, KERN_##seq for the sequence one
#define NINT_DW2(PLAIN_, SEQ_, NBLK_, LDS_, STAGE_) {                                                                                            \
    if (sq) { if (b16) hipLaunchKernelGGL(SEQ_<NINT_BF16>, dim3(NBLK_), dim3(512), LDS_, st, h_slab, n0, N, Ch, Chp, O, *sq, scratch, g->H, g->W, g->P, g->Hh, g->Wh, STAGE_);  \
              else hipLaunchKernelGGL(SEQ_<NINT_F32>, dim3(NBLK_), dim3(512), LDS_, st, h_slab, n0, N, Ch, Chp, O, *sq, scratch, g->H, g->W, g->P, g->Hh, g->Wh, STAGE_); }      \
    else { if (b16) hipLaunchKernelGGL(PLAIN_<NINT_BF16>, dim3(NBLK_), dim3(512), LDS_, st, h_slab, n0, N, Ch, Chp, O, dpred, scratch, g->H, g->W, g->P, g->Hh, g->Wh, STAGE_); \
           else hipLaunchKernelGGL(PLAIN_<NINT_F32>, dim3(NBLK_), dim3(512), LDS_, st, h_slab, n0, N, Ch, Chp, O, dpred, scratch, g->H, g->W, g->P, g->Hh, g->Wh, STAGE_); } }
  if (dw && db && scratch && nout > 512 && Rd <= 32 && Td <= 512 && scratch_bytes >= (size_t)256 * nout * sizeof(float)) {
    const int SR = (Rd + 3) & ~3, ST = Td | 1, NH = 512 / Td < 8 ? 512 / Td : 8;
    int stage = HEAD_DW_LDS_FLOATS / (SR + ST);
    if (stage > HEAD_DW_PIX) stage = HEAD_DW_PIX;
    size_t lds_f = (size_t)stage * (SR + ST);
    if ((size_t)NH * Td * SR > lds_f) lds_f = (size_t)NH * Td * SR;            // the closing fold's buffer
    const size_t lds = lds_f * sizeof(float);
    if (stage >= 8 && lds <= 64 * 1024) {
      const size_t cap = scratch_bytes / ((size_t)nout * sizeof(float));
      const size_t want = (npix + HEAD_DW_PIX - 1) / HEAD_DW_PIX;
      const int nblk = (int)(want < cap ? want : cap);
      NINT_DW2(head_bwd_dw_rtile_kernel, head_bwd_dw_rtile_seq_kernel, nblk, lds, stage)
      NINT_LAUNCH_CHECK();
      hipLaunchKernelGGL(head_bwd_dw_final_kernel, dim3(nint_cdiv(nout, 64)), dim3(1024), 0, st, scratch, nblk, Ch, O, dw, db);
      NINT_LAUNCH_CHECK();
      return NINT_OK;
    }
  }
  if (dw && db && scratch && nout <= HEAD_DW_NK * 512 && 8 * row_floats <= HEAD_DW_LDS_FLOATS &&
      scratch_bytes >= (size_t)256 * nout * sizeof(float)) {
    int stage = HEAD_DW_LDS_FLOATS / row_floats;               // pixels staged at a time (60 KiB of LDS)
    if (stage > HEAD_DW_PIX) stage = HEAD_DW_PIX;
    const size_t lds = (size_t)stage * row_floats * sizeof(float);
    const size_t cap = scratch_bytes / ((size_t)nout * sizeof(float));
    const size_t want = (npix + HEAD_DW_PIX - 1) / HEAD_DW_PIX;
    const int nblk = (int)(want < cap ? want : cap);
    NINT_DW2(head_bwd_dw_tiled_kernel, head_bwd_dw_tiled_seq_kernel, nblk, lds, stage)
    NINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_bwd_dw_final_kernel, dim3(nint_cdiv(nout, 64)), dim3(1024), 0, st, scratch, nblk, Ch, O, dw, db);
    NINT_LAUNCH_CHECK();
  } else if (dw && db) {
    if (sq) {
      if (b16) hipLaunchKernelGGL(head_bwd_dw_seq_kernel<NINT_BF16>, dim3(O * (Ch + 1)), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, *sq, dw, db, g->H, g->W, g->P, g->Hh, g->Wh);
      else hipLaunchKernelGGL(head_bwd_dw_seq_kernel<NINT_F32>, dim3(O * (Ch + 1)), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, *sq, dw, db, g->H, g->W, g->P, g->Hh, g->Wh);
    } else if (b16) {
      hipLaunchKernelGGL(head_bwd_dw_kernel<NINT_BF16>, dim3(O * (Ch + 1)), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, dpred, dw, db, g->H, g->W, g->P, g->Hh, g->Wh);
    } else {
      hipLaunchKernelGGL(head_bwd_dw_kernel<NINT_F32>, dim3(O * (Ch + 1)), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, dpred, dw, db, g->H, g->W, g->P, g->Hh, g->Wh);
    }
    NINT_LAUNCH_CHECK();
  }
#undef NINT_DW2
  return NINT_OK;
}

extern "C" int nint_head_bwd(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                             const float* dpred, void* dh, float* dw, float* db, const nint_geom* g, int dtype,
                             float* scratch, size_t scratch_bytes, void* stream) {
  if (!h_slab || !w || !dpred || !g || N <= 0 || O <= 0 || Ch <= 0) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  return head_bwd_impl(h_slab, n0, N, Ch, Chp, O, w, dpred, nullptr, dh, dw, db, g, dtype, scratch, scratch_bytes, stream);
}

extern "C" int nint_head_bwd_seq(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* dseq,
                                 const float* dpred_last, void* dh_seq, float* dw, float* db, const nint_geom* g, int dtype,
                                 float* scratch, size_t scratch_bytes, void* stream) {
  if (!head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if ((!dseq && !dpred_last) || (!dw) != (!db) || (!dh_seq && !dw)) return NINT_E_ARG;
  if (((((uintptr_t)h_slab) | ((uintptr_t)dh_seq)) & 15) != 0) return NINT_E_ALIGN;
  const DpSeq sq = {dseq, dpred_last, O, B, T, (size_t)g->H * g->W};
  return head_bwd_impl(h_slab, B, T * B, Ch, Chp, O, w, nullptr, &sq, dh_seq, dw, db, g, dtype, scratch, scratch_bytes, stream);
}

// ------------------------------------------------------------------------------ loss
// train.py:102,105: crop, MSELoss + L1Loss (mean).  Two launches on the same stream:
//  (1) per-block partial sums in double (fixed order), (2) one block folds them, writes
//  the loss and adds to the 5 running statistics.  dpred = (2(p-y) + sign(p-y)) / n on the crop.
__global__ __launch_bounds__(1024) void loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                           float* __restrict__ dpred, double* __restrict__ partial,
                                                           int N, int O, int H, int W, int oy, int ox, int Hc, int Wc) {
  const size_t total = (size_t)N * O * H * W;
  const double inv_n = 1.0 / ((double)N * O * Hc * Wc);
  double s2 = 0, s1 = 0, sy = 0, syy = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int yy = r % H;
    const size_t no = r / H;
    const int cy = yy - oy, cx = x - ox;
    float g = 0.f;
    if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) {
      const float t = y[(no * Hc + cy) * Wc + cx];
      const float d = pred[i] - t;
      s2 += (double)d * d;
      s1 += fabs((double)d);
      sy += t;
      syy += (double)t * t;
      g = (float)((2.0 * d + (d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0))) * inv_n);
    }
    if (dpred) dpred[i] = g;
  }
  __shared__ double red[4][1024];
  red[0][threadIdx.x] = s2; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = sy; red[3][threadIdx.x] = syy;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 4) partial[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ loss_out,
                                                         double* __restrict__ stats, double count) {
  // thread (b, q) = one partial; fixed-order tree over the blocks
  __shared__ double red[4][256];
  for (int q = 0; q < 4; ++q) {
    double s = 0;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += partial[b * 4 + q];
    red[q][threadIdx.x] = s;
  }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st)
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double s0 = red[0][0], s1 = red[1][0], s2 = red[2][0], s3 = red[3][0];
    const double loss = s0 / count + s1 / count;
    if (loss_out) loss_out[0] = (float)loss;
    if (stats) {
      stats[0] += s0; stats[1] += s1; stats[2] += s2; stats[3] += s3; stats[4] += count;
      // the reference's per-batch statistics (train.py:113-117, utils.py:73-75): it sums loss.item() and
      // sklearn r2_score(y, pred) of every batch and divides by the number of batches
      const double ss_tot = s3 - s2 * s2 / count;
      const double r2 = ss_tot > 0.0 ? 1.0 - s0 / ss_tot : (s0 == 0.0 ? 1.0 : 0.0);   // sklearn's constant-target convention
      stats[5] += loss; stats[6] += r2; stats[7] += 1.0;
    }
  }
}

// partial sums live in a small static device buffer per call site: the caller passes it as the
// tail of `stats` would complicate the ABI, so the kernel pair uses dpred-independent scratch
// carved from loss_out[1..]: loss_out must have room for 1 + 2*LOSS_BLOCKS*4 floats.
#define LOSS_BLOCKS 256
#define LOSS_BLOCKS_MAX ((NINT_LOSS_SCRATCH_FLOATS - 2) / 8)     // what the caller's scratch holds: 4 doubles per workgroup
extern "C" int nint_loss_mse_l1_crop(const float* pred, const float* y, float* dpred, float* loss_out, double* stats,
                                     int N, int O, int H, int W, int oy, int ox, int Hc, int Wc, void* stream) {
  if (!pred || !y || !loss_out || N <= 0 || O <= 0 || oy < 0 || ox < 0 || oy + Hc > H || ox + Wc > W) return NINT_E_ARG;
  if ((((uintptr_t)loss_out) & 7) != 0) return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)(loss_out + 2);   // loss_out: [0]=loss, [1]=pad, [2..] = 256*4 doubles
  hipLaunchKernelGGL(loss_partial_kernel, dim3(LOSS_BLOCKS), dim3(1024), 0, st, pred, y, dpred, partial, N, O, H, W, oy, ox, Hc, Wc);
  NINT_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, partial, LOSS_BLOCKS, loss_out, stats, (double)N * O * Hc * Wc);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// ------------------------------------------------------------------------------ head + loss, fused (training)
// train.py:96-109 around the 1x1 head in ONE pass over the pixels: pred = w . h + b (model.py:274), crop, the MSE+L1
// partial sums (train.py:102,105), d loss / d pred, and dL/dh = w^T . dpred.  One thread per pixel (grid-stride):
// the channel vector is read once, pred never goes to memory, dpred is written for the head's weight gradient.
// Same arithmetic, in the same order, as head_fwd_kernel -> loss_partial_kernel -> head_bwd_dh_kernel.
#define HEAD_OCH 64
// SEQ (nint_head_loss_seq_fused): the images are all T*B steps of the slab, image n = t*B + b; the targets are (B, T, O, Hc, Wc),
// plane block b*T + t (head_image); dpred and dh stay in image order, which is what the weight-gradient stage and BPTT read.
template <int DT, int CHV, bool SEQ>
__device__ __forceinline__ void head_loss_fused_body(char* smem_hl, const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                     const float* __restrict__ w, const float* __restrict__ b,
                                                     const float* __restrict__ y, float* __restrict__ dpred,
                                                     void* __restrict__ dh, double* __restrict__ partial, int H, int W,
                                                     int P, int Hh, int Wh, int oy, int ox, int Hc, int Wc, int Bs) {
  // A workgroup takes 64 pixels per pass (grid-stride).  Phase 1: wave q runs the outputs [q*OG, (q+1)*OG) of every pixel
  // (lane = pixel): pred, loss terms, d loss / d pred -> dpred and, through LDS, to phase 2: wave q accumulates the
  // channels [q*CHV/4, (q+1)*CHV/4) of dL/dh over ALL outputs in output order.  (One thread per pixel for all outputs --
  // the first version -- is a chain of O dependent round trips on 1/4 of the threads: 50 us at B = 8, 44 us at B = 1.)
  float* w_s = (float*)smem_hl;                  // [O][CHV], zero padded (head_stage_weights)
  float* gq_s = w_s + O * CHV;                   // [min(O, HEAD_OCH)][64]
  head_stage_weights<CHV>(w_s, w, O, Ch);
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar: the weight reads below stay scalar loads)
  const size_t npix = (size_t)N * H * W;
  const double inv_n = 1.0 / ((double)N * O * Hc * Wc);
  constexpr int CQ = CHV / 4;                    // channels per wave in phase 2
  double s2 = 0, s1 = 0, sy = 0, syy = 0;
  for (size_t p0 = (size_t)blockIdx.x * 64; p0 < npix; p0 += (size_t)gridDim.x * 64) {
    const size_t pix = p0 + lane;
    const bool live = pix < npix;
    const size_t pc = live ? pix : npix - 1;
    const int x = pc % W;
    size_t r = pc / W;
    const int yy = r % H;
    const int n = r / H;
    const size_t hb = ((((size_t)(n0 + n)) * Hh + (yy + P)) * Wh + (x + P)) * Chp;
    float hv[CHV];
#pragma unroll
    for (int c = 0; c < CHV; c += 4) {
      const f32x4_t v = (c < Chp) ? load_vec4<DT>(h, hb + c) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
      hv[c] = v[0]; hv[c + 1] = v[1]; hv[c + 2] = v[2]; hv[c + 3] = v[3];
    }
    const int cy = yy - oy, cx = x - ox;
    const bool in = live && cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
    float* dp = dpred + ((size_t)n * O * H + yy) * W + x;
    const float* yp = y + (head_image<SEQ>(n, Bs, N / (SEQ ? Bs : 1)) * O * Hc + cy) * Wc + cx;
    float acc[CQ];
#pragma unroll
    for (int c = 0; c < CQ; ++c) acc[c] = 0.f;
    const int c0 = q * CQ;
    // the outputs in chunks of HEAD_OCH (d loss / d pred of one chunk in LDS at a time: 200 outputs would otherwise pin the
    // workgroup count per CU at one); phase 2 keeps accumulating in output order across the chunks
    for (int oc = 0; oc < O; oc += HEAD_OCH) {
      const int on = min(HEAD_OCH, O - oc);
      const int OG = (on + 3) / 4, ob = oc + q * OG, oe = min(oc + on, ob + OG);
      if (oc > 0) __syncthreads();               // the previous chunk is consumed
      constexpr int OU = 5;                      // targets fetched ahead of their use: one HBM round trip per OU outputs
      for (int o0 = ob; o0 < oe; o0 += OU) {
        float tq[OU];
#pragma unroll
        for (int u = 0; u < OU; ++u) tq[u] = (in && o0 + u < oe) ? yp[(size_t)(o0 + u) * Hc * Wc] : 0.f;
#pragma unroll
        for (int u = 0; u < OU; ++u) {
          const int o = o0 + u;
          if (o >= oe) break;
          float p = b ? b[o] : 0.f;
          const f32x4_t* wr = (const f32x4_t*)(w_s + o * CHV);
#pragma unroll
          for (int c = 0; c < CHV; c += 4) {
            const f32x4_t wv = wr[c / 4];
            p += wv[0] * hv[c]; p += wv[1] * hv[c + 1]; p += wv[2] * hv[c + 2]; p += wv[3] * hv[c + 3];
          }
          float gq = 0.f;
          if (in) {
            const float t = tq[u];
            const float d = p - t;
            s2 += (double)d * d;
            s1 += fabs((double)d);
            sy += t;
            syy += (double)t * t;
            gq = (float)((2.0 * d + (d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0))) * inv_n);
          }
          if (live) dp[(size_t)o * H * W] = gq;
          gq_s[(o - oc) * 64 + lane] = gq;
        }
      }
      __syncthreads();
      // phase 2: dL/dh[c] = sum_o w[o][c] * gq[o], in output order (the order of head_bwd_dh_kernel)
      for (int o = oc; o < oc + on; ++o) {
        const float gq = gq_s[(o - oc) * 64 + lane];
        const f32x4_t* wr = (const f32x4_t*)(w_s + o * CHV + c0);
#pragma unroll
        for (int c = 0; c < CQ; c += 4) {
          const f32x4_t wv = wr[c / 4];
          acc[c] += wv[0] * gq; acc[c + 1] += wv[1] * gq; acc[c + 2] += wv[2] * gq; acc[c + 3] += wv[3] * gq;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < CQ; c += 4)
        if (c0 + c < Chp) store_vec4<DT>(dh, pix * Chp + c0 + c, (f32x4_t){acc[c], acc[c + 1], acc[c + 2], acc[c + 3]});
    }
    __syncthreads();                             // gq_s is rewritten by the next pass
  }
  __shared__ double red[4][256];
  red[0][threadIdx.x] = s2; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = sy; red[3][threadIdx.x] = syy;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int q2 = 0; q2 < 4; ++q2) red[q2][threadIdx.x] += red[q2][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 4) partial[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

template <int DT, int CHV>
__global__ __launch_bounds__(256) void head_loss_fused_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                              const float* __restrict__ w, const float* __restrict__ b,
                                                              const float* __restrict__ y, float* __restrict__ dpred,
                                                              void* __restrict__ dh, double* __restrict__ partial, int H, int W,
                                                              int P, int Hh, int Wh, int oy, int ox, int Hc, int Wc) {
  extern __shared__ __attribute__((aligned(16))) char smem_hl[];
  head_loss_fused_body<DT, CHV, false>(smem_hl, h, n0, N, Ch, Chp, O, w, b, y, dpred, dh, partial, H, W, P, Hh, Wh, oy, ox, Hc, Wc, 0);
}

template <int DT, int CHV>
__global__ __launch_bounds__(256) void head_loss_seq_fused_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                                  const float* __restrict__ w, const float* __restrict__ b,
                                                                  const float* __restrict__ y, float* __restrict__ dpred,
                                                                  void* __restrict__ dh, double* __restrict__ partial, int H, int W,
                                                                  int P, int Hh, int Wh, int oy, int ox, int Hc, int Wc, int Bs) {
  extern __shared__ __attribute__((aligned(16))) char smem_hls[];
  head_loss_fused_body<DT, CHV, true>(smem_hls, h, n0, N, Ch, Chp, O, w, b, y, dpred, dh, partial, H, W, P, Hh, Wh, oy, ox, Hc, Wc, Bs);
}

static int head_loss_fused_impl(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                const float* y, float* dpred, void* dh, float* loss_out, double* stats, const nint_geom* g,
                                int oy, int ox, int Hc, int Wc, int dtype, int Bs, void* stream);

extern "C" int nint_head_loss_fused(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                    const float* y, float* dpred, void* dh, float* loss_out, double* stats, const nint_geom* g,
                                    int oy, int ox, int Hc, int Wc, int dtype, void* stream) {
  if (!h_slab || !w || !y || !dpred || !dh || !loss_out || !g || N <= 0 || O <= 0 || Ch <= 0) return NINT_E_ARG;
  if (oy < 0 || ox < 0 || oy + Hc > g->H || ox + Wc > g->W) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  if (Chp > 128 || Chp % 4) return NINT_E_SHAPE;   // wider heads: nint_head_fwd + nint_loss_mse_l1_crop + nint_head_bwd
  if ((((uintptr_t)loss_out) & 7) != 0) return NINT_E_ALIGN;
  return head_loss_fused_impl(h_slab, n0, N, Ch, Chp, O, w, b, y, dpred, dh, loss_out, stats, g, oy, ox, Hc, Wc, dtype, 0, stream);
}

extern "C" int nint_head_loss_seq_fused(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                        const float* y, float* dpred, void* dh_seq, float* loss_out, double* stats,
                                        const nint_geom* g, int oy, int ox, int Hc, int Wc, int dtype, void* stream) {
  if (!y || !dpred || !dh_seq || !loss_out || !head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if (oy < 0 || ox < 0 || Hc <= 0 || Wc <= 0 || oy + Hc > g->H || ox + Wc > g->W) return NINT_E_ARG;
  if (Chp > 128) return NINT_E_SHAPE;              // wider heads: nint_head_fwd_seq + nint_loss_mse_l1_crop + nint_head_bwd_seq
  if ((((uintptr_t)loss_out) & 7) != 0 || ((((uintptr_t)h_slab) | ((uintptr_t)dh_seq)) & 15) != 0) return NINT_E_ALIGN;
  return head_loss_fused_impl(h_slab, B, T * B, Ch, Chp, O, w, b, y, dpred, dh_seq, loss_out, stats, g, oy, ox, Hc, Wc, dtype, B, stream);
}

// Bs != 0: the sequence entry (n0 = B, N = T*B)
static int head_loss_fused_impl(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                const float* y, float* dpred, void* dh, float* loss_out, double* stats, const nint_geom* g,
                                int oy, int ox, int Hc, int Wc, int dtype, int Bs, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)(loss_out + 2);   // loss_out: [0]=loss, [1]=pad, [2..] = up to LOSS_BLOCKS_MAX*4 doubles
  // 64 pixels per workgroup and pass: up to LOSS_BLOCKS_MAX workgroups
  const size_t npix = (size_t)N * g->H * g->W;
  const int nblk = (int)((npix + 63) / 64 < LOSS_BLOCKS_MAX ? (npix + 63) / 64 : LOSS_BLOCKS_MAX);
  const dim3 grid(nblk);
  const int chv = Chp <= 32 ? 32 : (Chp <= 64 ? 64 : 128);
  const size_t lds = ((size_t)O * chv + (size_t)(O < HEAD_OCH ? O : HEAD_OCH) * 64) * sizeof(float);   // weights [O][CHV] + d loss / d pred of 64 pixels, one output chunk
  if (lds + 8192 > 160 * 1024) return NINT_E_SHAPE;
#define NINT_HL(DT_, CHV_) { if (Bs) { auto kern = head_loss_seq_fused_kernel<DT_, CHV_>;                                                       \
                               if (lds + 8192 > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                               hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, h_slab, n0, N, Ch, Chp, O, w, b,                              \
                                                  y, dpred, dh, partial, g->H, g->W, g->P, g->Hh, g->Wh, oy, ox, Hc, Wc, Bs); }                 \
                             else { auto kern = head_loss_fused_kernel<DT_, CHV_>;                                                            \
                               if (lds + 8192 > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                               hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, h_slab, n0, N, Ch, Chp, O, w, b,                              \
                                                  y, dpred, dh, partial, g->H, g->W, g->P, g->Hh, g->Wh, oy, ox, Hc, Wc); } }
  if (dtype == NINT_BF16) { if (Chp <= 32) NINT_HL(NINT_BF16, 32) else if (Chp <= 64) NINT_HL(NINT_BF16, 64) else NINT_HL(NINT_BF16, 128) }
  else { if (Chp <= 32) NINT_HL(NINT_F32, 32) else if (Chp <= 64) NINT_HL(NINT_F32, 64) else NINT_HL(NINT_F32, 128) }
#undef NINT_HL
  NINT_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, partial, nblk, loss_out, stats, (double)N * O * Hc * Wc);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// ------------------------------------------------------------------------------ Adam
// torch.optim.Adam single-tensor update order (train.py:71,110):
//   m = lerp(m, g, 1-b1) ; v = b2*v + (1-b2)*g*g ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
__global__ void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, size_t n, float step_size, float w1, float b2, float w2,
                                 float eps, float inv_sqrt_bc2_denom, float grad_scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float gr = g[i] * grad_scale;
    float mi = m[i], vi = v[i];
    // torch lerp: a + w*(b-a) for w < 0.5, else b - (b-a)*(1-w)
    mi = (w1 < 0.5f) ? __fadd_rn(mi, __fmul_rn(w1, __fsub_rn(gr, mi)))
                     : __fsub_rn(gr, __fmul_rn(__fsub_rn(gr, mi), 1.f - w1));
    vi = __fadd_rn(__fmul_rn(vi, b2), __fmul_rn(__fmul_rn(w2, gr), gr));   // addcmul: (value*t1)*t2
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vi), inv_sqrt_bc2_denom), eps);
    p[i] = __fadd_rn(p[i], __fdiv_rn(__fmul_rn(-step_size, mi), denom));          // addcdiv: (value*t1)/t2
    m[i] = mi;
    v[i] = vi;
  }
}

extern "C" int nint_adam_flat(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1,
                              double beta2, double eps, int step, float grad_scale, void* stream) {
  if (!p || !g || !m || !v || step < 1) return NINT_E_ARG;
  if (n == 0) return NINT_OK;
  // scalars in double like torch's Python floats, rounded to f32 once
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  const float step_size = (float)(lr / bc1);
  const float sqrt_bc2 = (float)sqrt(bc2);
  hipLaunchKernelGGL(adam_flat_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, step_size,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, sqrt_bc2, grad_scale);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// ------------------------------------------------------------------------------ preproc
// dataset.py:526-536 through :67-98.  Output element (t, c, yp, xp):
//   lon: cyclic, xs = (xp - pl) mod W                            (dataset.py:67-80)
//   lat: top halo row j (< pt)  <- source row 1+j      (mode 0, channel C-1-c: np.fliplr quirk, dataset.py:96)
//                                <- source row pt-j     (mode 1, true reflect, dataset.py:51 semantics)
//        bottom halo row j      <- source row H-pb-1+j  (mode 0, channel C-1-c) / H-2-j (mode 1)
//   value = (src - mean[c]) / std[c]                              (dataset.py:528), with mean/std of
//   the SOURCE channel that is actually read (the reference z-scores before it pads).
// Sources are RECORDS (n_steps, lev_i, H, W) resident in HBM; sample b of a batch reads the time steps
// [t0[b], t0[b]+T) of every source (the sliding window of dataset.py:614-616 as a pointer offset), so one
// launch serves the whole batch.  The trailing sources from first_static on are TIME-INVARIANT (the static
// attributes of dataset.py:100-122, concatenated after the dynamic channels at :531-533 / :622-624): one
// (lev_i, H, W) "time step", read at step 0 whatever t0[b] + t is.  They are ordinary fused channels otherwise,
// so the mode-0 halo of channel c still comes from channel C-1-c across the whole C.
// All index arithmetic is per row (scalar); threads only walk x.
#define PRE_MAX_SRC 16
#define PRE_MAX_B NINT_PRE_MAX_B
struct PreArgs {
  const float* src[PRE_MAX_SRC];
  int first_c[PRE_MAX_SRC + 1];   // first fused channel of each source
  int nsrc;
  int first_static;               // sources [first_static, nsrc) are time-invariant (nsrc: none)
  int t0[PRE_MAX_B];              // first time step of each sample's window
};

// time step of source s that sample b reads at window step t (0 for a time-invariant source)
__device__ __forceinline__ size_t pre_step(const PreArgs& a, int s, int b, int t) {
  return s >= a.first_static ? 0 : (size_t)(a.t0[b] + t);
}

// latitude rule: source row of padded row yp, and whether the row comes from the channel-flipped source
__device__ __forceinline__ int pre_src_row(int yp, int H, int pt, int pb, int mode, bool* flip) {
  *flip = false;
  if (yp < pt) {
    if (mode == 0) { *flip = true; return 1 + yp; }
    return pt - yp;
  }
  if (yp < pt + H) return yp - pt;
  const int j = yp - pt - H;
  if (mode == 0) { *flip = true; return H - pb - 1 + j; }
  return H - 2 - j;
}

// (source, level) of fused channel c: wave-uniform, a handful of scalar compares
__device__ __forceinline__ void pre_find(const PreArgs& a, int c, int* s_out, int* lev_out, int* nlev_out) {
  int s = 0;
  while (s + 1 < a.nsrc && c >= a.first_c[s + 1]) ++s;
  *s_out = s;
  *lev_out = c - a.first_c[s];
  *nlev_out = a.first_c[s + 1] - a.first_c[s];
}

// f32 NCHW output (B, T, C, Hp, Wp): one workgroup per (b, t, c) plane and row group; the public
// Dataset.__getitem__ layout (dataset.py:538-539) and the target z-score.
__global__ __launch_bounds__(256) void preproc_nchw_kernel(PreArgs a, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           float* __restrict__ out, int B, int T, int C, int H, int W, int Hp,
                                                           int Wp, int mode) {
  const int pl = (Wp - W) / 2, pt = (Hp - H) / 2, pb = Hp - H - pt;
  int r = blockIdx.x;
  const int c = r % C; r /= C;
  const int t = r % T;
  const int b = r / T;
  // the two candidate source channels of this plane (interior rows: c, mode-0 halo rows: C-1-c)
  const float* base[2]; float m[2], sd[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int cs = f ? C - 1 - c : c;
    int s, lev, nlev;
    pre_find(a, cs, &s, &lev, &nlev);
    base[f] = a.src[s] + (pre_step(a, s, b, t) * nlev + lev) * H * W;
    m[f] = mean[cs]; sd[f] = stdv[cs];
  }
  float* o = out + (((size_t)b * T + t) * C + c) * Hp * Wp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int yp = blockIdx.y * 4 + wave; yp < Hp; yp += gridDim.y * 4) {      // a wave per row: row math is scalar
    bool flip;
    const int ys = pre_src_row(yp, H, pt, pb, mode, &flip);
    const float* row = base[flip ? 1 : 0] + (size_t)ys * W;
    const float mm = flip ? m[1] : m[0], ss = flip ? sd[1] : sd[0];
    for (int xp = lane; xp < Wp; xp += 64) {
      int xs = xp - pl;
      xs = xs < 0 ? xs + W : (xs >= W ? xs - W : xs);
      o[(size_t)yp * Wp + xp] = (row[xs] - mm) / ss;
    }
  }
}

// Straight into the model's input halo slab: image t*B + b0 + b, interior rows/columns [P, P+Hp) x [P, P+Wp),
// channels-last ET with the channel padding written as zeros.  One workgroup per (b, t, yp) row: the C source
// rows (each contiguous along x) are z-scored into an LDS tile [C][W+1], then written out as 16-byte vectors of
// 8 (bf16) / 4 (f32) consecutive channels -- the f32 NCHW intermediate and the separate pack pass never exist.
template <int DT, int VW>
__global__ __launch_bounds__(256) void preproc_slab_kernel(PreArgs a, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           void* __restrict__ dst, int B, int b0, int nb, int T, int C, int Cp,
                                                           int H, int W, int Hp, int Wp, int mode, int P, int Hh, int Wh, int kf) {
  extern __shared__ __attribute__((aligned(16))) char smem_pre[];
  RowDesc* rows = (RowDesc*)smem_pre;                                        // [C] source row of every fused channel
  float* tile = (float*)(smem_pre + nint_round_up(C * (int)sizeof(RowDesc), 16));   // [C][W + 1]
  const int ld = W + 1;
  const int pl = (Wp - W) / 2, pt = (Hp - H) / 2, pb = Hp - H - pt;
  int r = blockIdx.x;
  const int yp = r % Hp; r /= Hp;
  const int t = r % T;
  const int b = r / T;                         // sample inside this launch, [0, nb)
  bool flip;
  const int ys = pre_src_row(yp, H, pt, pb, mode, &flip);
  for (int cs = threadIdx.x; cs < C; cs += 256) {   // one descriptor per source channel: (source, level) found once per row block
    int s, lev, nlev;
    pre_find(a, cs, &s, &lev, &nlev);
    rows[cs] = RowDesc{a.src[s] + (pre_step(a, s, b, t) * nlev + lev) * H * W + (size_t)ys * W, mean[cs], stdv[cs],
                       flip ? C - 1 - cs : cs};
  }
  __syncthreads();
  stage_rows<VW, true>(tile, ld, C, W, [&](int c) { return rows[c]; });
  __syncthreads();
  char* d = (char*)dst + ((((size_t)t * B + b0 + b) * Hh + (yp + P)) * Wh + P) * (size_t)Cp * Elem<DT>::ES;
  write_row_channels_last<DT>(tile, ld, C, Cp, Wp, d, [&](int xp) {
    const int xs = xp - pl;                    // cyclic longitude (dataset.py:67-80)
    return xs < 0 ? xs + W : (xs >= W ? xs - W : xs);
  }, kf);
}

static int pre_args(PreArgs* a, const float* const* srcs, const int* lev, int nsrc, int nstatic, int H, int W, int Hp, int Wp,
                    int mode) {
  if (!srcs || !lev || nsrc <= 0 || nsrc > PRE_MAX_SRC || nstatic < 0 || nstatic > nsrc) return NINT_E_ARG;
  if (Hp < H || Wp < W || (mode != 0 && mode != 1)) return NINT_E_ARG;
  const int pl = (Wp - W) / 2, pr = Wp - W - pl, pt = (Hp - H) / 2, pb = Hp - H - pt;
  // the reference raises AttributeError for oversize padding (dataset.py:80,98)
  if (pl > W || pr > W || pt + 1 > H || pb + 1 > H) return NINT_E_SHAPE;
  a->nsrc = nsrc;
  a->first_static = nsrc - nstatic;
  int c = 0;
  for (int i = 0; i < nsrc; ++i) {
    if (!srcs[i] || lev[i] <= 0) return NINT_E_ARG;
    a->src[i] = srcs[i];
    a->first_c[i] = c;
    c += lev[i];
  }
  a->first_c[nsrc] = c;
  return c;
}

extern "C" int nint_preproc_fuse_pad_static_batch(const float* const* srcs, const int* lev, int nsrc, int nstatic,
                                                  const float* mean, const float* stdv, const int* t0, int B, float* out,
                                                  int T, int H, int W, int Hp, int Wp, int mode, void* stream) {
  if (!mean || !stdv || !out || !t0 || T <= 0 || B <= 0) return NINT_E_ARG;
  PreArgs a;
  const int C = pre_args(&a, srcs, lev, nsrc, nstatic, H, W, Hp, Wp, mode);
  if (C < 0) return C;
  for (int b0 = 0; b0 < B; b0 += PRE_MAX_B) {
    const int nb = B - b0 < PRE_MAX_B ? B - b0 : PRE_MAX_B;
    for (int i = 0; i < nb; ++i) {
      if (t0[b0 + i] < 0) return NINT_E_ARG;
      a.t0[i] = t0[b0 + i];
    }
    const int planes = nb * T * C;
    // enough row groups per plane to put a few thousand workgroups in flight on small batches
    int gy = planes >= 2048 ? 1 : nint_cdiv(2048, planes);
    if (gy > nint_cdiv(Hp, 4)) gy = nint_cdiv(Hp, 4);
    hipLaunchKernelGGL(preproc_nchw_kernel, dim3(planes, gy), dim3(256), 0, (hipStream_t)stream, a, mean, stdv,
                       out + (size_t)b0 * T * C * Hp * Wp, nb, T, C, H, W, Hp, Wp, mode);
    NINT_LAUNCH_CHECK();
  }
  return NINT_OK;
}

extern "C" int nint_preproc_fuse_pad_batch(const float* const* srcs, const int* lev, int nsrc, const float* mean,
                                           const float* stdv, const int* t0, int B, float* out, int T, int H, int W,
                                           int Hp, int Wp, int mode, void* stream) {
  return nint_preproc_fuse_pad_static_batch(srcs, lev, nsrc, 0, mean, stdv, t0, B, out, T, H, W, Hp, Wp, mode, stream);
}

extern "C" int nint_preproc_fuse_pad_static(const float* const* srcs, const int* lev, int nsrc, int nstatic,
                                            const float* mean, const float* stdv, float* out, int T, int H, int W, int Hp,
                                            int Wp, int mode, void* stream) {
  const int t0 = 0;     // srcs already point at the window's first time step (static sources: at their only step)
  return nint_preproc_fuse_pad_static_batch(srcs, lev, nsrc, nstatic, mean, stdv, &t0, 1, out, T, H, W, Hp, Wp, mode, stream);
}

extern "C" int nint_preproc_fuse_pad(const float* const* srcs, const int* lev, int nsrc, const float* mean,
                                     const float* stdv, float* out, int T, int H, int W, int Hp, int Wp, int mode,
                                     void* stream) {
  return nint_preproc_fuse_pad_static(srcs, lev, nsrc, 0, mean, stdv, out, T, H, W, Hp, Wp, mode, stream);
}

extern "C" int nint_preproc_fuse_pad_static_slab(const float* const* srcs, const int* lev, int nsrc, int nstatic,
                                                 const float* mean, const float* stdv, const int* t0, int B, void* xs_slab,
                                                 int Cxp, int xfold_k, int T, int H, int W, const nint_geom* g, int mode,
                                                 int dtype, void* stream) {
  if (!mean || !stdv || !xs_slab || !t0 || !g || T <= 0 || B <= 0) return NINT_E_ARG;
  if (xfold_k < 0 || (xfold_k > 1 && !(xfold_k & 1))) return NINT_E_ARG;
  const int kf = xfold_k > 1 ? xfold_k : 1;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  const int Hp = g->H, Wp = g->W;               // the model runs on the padded grid (launcher.sh:24)
  PreArgs a;
  const int C = pre_args(&a, srcs, lev, nsrc, nstatic, H, W, Hp, Wp, mode);   // C counts the static channels too
  if (C < 0) return C;
  if (Cxp < C * kf || Cxp % (dtype == NINT_BF16 ? 8 : 4)) return NINT_E_ARG;
  if ((((uintptr_t)xs_slab) & 15) != 0) return NINT_E_ALIGN;
  const size_t tile_bytes = nint_round_up(C * (int)sizeof(RowDesc), 16) + (size_t)C * (W + 1) * sizeof(float);
  if (tile_bytes > 160 * 1024) return NINT_E_LDS;
  // widest row vector every source row's alignment allows (rows start at multiples of W floats from the record base,
  // static sources included)
  int vw = W % 4 == 0 ? 4 : (W % 2 == 0 ? 2 : 1);
  for (int i = 0; i < nsrc; ++i) {
    const uintptr_t p = (uintptr_t)srcs[i];
    while (vw > 1 && (p & (4 * vw - 1))) vw >>= 1;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += PRE_MAX_B) {
    const int nb = B - b0 < PRE_MAX_B ? B - b0 : PRE_MAX_B;
    for (int i = 0; i < nb; ++i) {
      if (t0[b0 + i] < 0) return NINT_E_ARG;
      a.t0[i] = t0[b0 + i];
    }
    const dim3 grid((unsigned)((size_t)nb * T * Hp));
#define NINT_PRE_V(DT_, VW_)                                                                                              \
    {                                                                                                                     \
      auto kern = preproc_slab_kernel<DT_, VW_>;                                                                          \
      if (tile_bytes > 64 * 1024)                                                                                         \
        NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes)); \
      hipLaunchKernelGGL(kern, grid, dim3(256), tile_bytes, st, a, mean, stdv, xs_slab, B, b0, nb, T, C, Cxp, H, W, Hp, Wp, \
                         mode, g->P, g->Hh, g->Wh, kf);                                                                    \
    }
#define NINT_PRE(DT_) { if (vw == 4) NINT_PRE_V(DT_, 4) else if (vw == 2) NINT_PRE_V(DT_, 2) else NINT_PRE_V(DT_, 1) }
    if (dtype == NINT_BF16) NINT_PRE(NINT_BF16) else NINT_PRE(NINT_F32)
#undef NINT_PRE
#undef NINT_PRE_V
    NINT_LAUNCH_CHECK();
  }
  return NINT_OK;
}

extern "C" int nint_preproc_fuse_pad_slab(const float* const* srcs, const int* lev, int nsrc, const float* mean,
                                          const float* stdv, const int* t0, int B, void* xs_slab, int Cxp, int xfold_k,
                                          int T, int H, int W, const nint_geom* g, int mode, int dtype, void* stream) {
  return nint_preproc_fuse_pad_static_slab(srcs, lev, nsrc, 0, mean, stdv, t0, B, xs_slab, Cxp, xfold_k, T, H, W, g, mode,
                                           dtype, stream);
}
