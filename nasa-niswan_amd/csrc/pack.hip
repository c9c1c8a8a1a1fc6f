// pack.hip -- activation layout at the library's boundary: (B,T,C,H,W) f32 <-> channels-last halo slabs and compact
// tensors (pack_btchw*, unpack_halo, pack/unpack_compact, unfold_dx), and the fuse/z-score/halo-pad preproc, whose slab
// kernel shares stage_rows / write_row_channels_last with the row-tiled pack.  One-read/one-write streaming kernels;
// threads walk the channel axis fastest so that channels-last slabs are read and written in full cache lines.
#include "nint_common.h"

// ------------------------------------------------------------------------------ pack / unpack
// (B,T,C,H,W) f32 -> halo slab image t*B+b, interior only (halo/slack stay zero).
// Thread order: channel fastest on the WRITE side (full 64-byte rows); the NCHW read side is
// strided by H*W floats per channel, served from L2 after the first touch of each line.
template <int DT>
__global__ void pack_btchw_kernel(const float* __restrict__ src, void* __restrict__ dst, int B, int T, int C,
                                  int Cp, int H, int W, int P, int Hh, int Wh, int kf, int cyc) {
  const size_t total = (size_t)B * T * H * W * Cp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = i % Cp;
    size_t r = i / Cp;
    const int x = r % W; r /= W;
    const int y = r % H; r /= H;
    const int b = r % B;
    const int t = r / B;
    // kf > 1: horizontally folded layout, slab channel kx*C + c of pixel x = channel c of pixel x + kx - kf/2 (0 outside;
    // cyc: of that pixel mod W -- cyclic longitude, kf/2 <= W)
    const int kx = co / C, c = co - kx * C;
    int xi = x + kx - (kf >> 1);
    if (cyc) xi = xi < 0 ? xi + W : (xi >= W ? xi - W : xi);
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
// host side: f(std::integral_constant<int, VW>) for the row-vector width vw = 4 / 2 / 1 floats
template <class F> static inline auto by_row_vec(int vw, F&& f) {
  if (vw == 4) return f(std::integral_constant<int, 4>{});
  if (vw == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 1>{});
}

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
// kx*C + c of pixel xo is input channel c of pixel xo + kx - kf/2, zero outside [0, Wo) (the conv's zero padding); cyc: that
// pixel mod Wo instead (cyclic longitude, nint_seq.lon_cyclic; kf/2 <= Wo).
template <int DT, class XMap>
__device__ __forceinline__ void write_row_channels_last(const float* __restrict__ tile, int ld, int C, int Cp, int Wo, char* __restrict__ d,
                                                        XMap xmap, int kf = 1, int cyc = 0) {
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
        int xi = xo + kx - (kf >> 1);
        if (cyc) xi = xi < 0 ? xi + Wo : (xi >= Wo ? xi - Wo : xi);
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
                                                             int Wh, int kf, int cyc) {
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
  write_row_channels_last<DT>(tile, ld, C, Cp, W, d, [](int x) { return x; }, kf, cyc);
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
                           void* stream, int cyc = 0) {
  if (!src || !dst || !g || B <= 0 || T <= 0 || C <= 0 || Cp < C * kf) return NINT_E_ARG;
  if (cyc && g->W < kf / 2) return NINT_E_ARG;
  const size_t total = (size_t)B * T * g->H * g->W * Cp;
  hipStream_t st = (hipStream_t)stream;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  const size_t tile_bytes = (size_t)C * (g->W + 1) * sizeof(float);
  if (tile_bytes <= 160 * 1024 && Cp % (dtype == NINT_BF16 ? 8 : 4) == 0) {
    const dim3 grid((unsigned)((size_t)B * T * g->H));
    // widest row vector the alignment of every channel row allows (rows start at multiples of W floats)
    const int vw = ((((uintptr_t)src) & 15) == 0 && g->W % 4 == 0) ? 4 : (((((uintptr_t)src) & 7) == 0 && g->W % 2 == 0) ? 2 : 1);
    // (row tiles above 64 KiB -- 65+ channels on a 1-degree grid -- need the opt-in, as the slab preproc kernel does)
    const int rc = nint_by_dtype(dtype, [&](auto dt) { return by_row_vec(vw, [&](auto v) -> int {
      auto kern = pack_btchw_rows_kernel<decltype(dt)::value, decltype(v)::value>;
      if (tile_bytes > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
      hipLaunchKernelGGL(kern, grid, dim3(256), tile_bytes, st, src, dst, B, T, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh, kf, cyc);
      return NINT_OK; }); });
    if (rc != NINT_OK) return rc;
    NINT_LAUNCH_CHECK();
    return NINT_OK;
  }
  // rows that do not fit the LDS tile (or an odd channel padding): one thread per slab element, plain or folded
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(pack_btchw_kernel<decltype(dt)::value>, grid1d(total), dim3(256), 0, st, src, dst, B, T, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh, kf, cyc);
  });
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

extern "C" int nint_pack_btchw_xfold_cyclic(const float* src, void* dst, int B, int T, int C, int k, int Cp, const nint_geom* g,
                                            int dtype, void* stream) {
  if (k < 1 || !(k & 1)) return NINT_E_ARG;
  return pack_btchw_impl(src, dst, B, T, C, k, Cp, g, dtype, stream, 1);
}

// d/dx from the gradient of a horizontally folded input: dx[n][c][y][x] = sum_kx dfold[n][y][x - kx + k/2][kx*C + c]
// (cyc: the source pixel taken mod W, the adjoint of the cyclic fold)
template <int DT>
__global__ void unfold_dx_kernel(const void* __restrict__ src, float* __restrict__ dst, int N, int C, int k, int Cp, int H, int W,
                                 int cyc) {
  const size_t total = (size_t)N * C * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int y = r % H; r /= H;
    const int c = r % C;
    const int n = r / C;
    float acc = 0.f;
    for (int kx = 0; kx < k; ++kx) {
      int xs = x - kx + k / 2;
      if (cyc) xs = xs < 0 ? xs + W : (xs >= W ? xs - W : xs);
      if (xs >= 0 && xs < W) acc += load_elem<DT>(src, (((size_t)n * H + y) * W + xs) * Cp + kx * C + c);
    }
    dst[i] = acc;
  }
}

static int unfold_dx_impl(const void* src, float* dst, int N, int C, int k, int Cp, int H, int W, int dtype, void* stream, int cyc) {
  if (!src || !dst || N <= 0 || C <= 0 || k < 1 || !(k & 1) || Cp < k * C || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  if (cyc && W < k / 2) return NINT_E_ARG;
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(unfold_dx_kernel<decltype(dt)::value>, grid1d((size_t)N * C * H * W), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, k, Cp, H, W, cyc);
  });
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_unfold_dx(const void* src, float* dst, int N, int C, int k, int Cp, int H, int W, int dtype, void* stream) {
  return unfold_dx_impl(src, dst, N, C, k, Cp, H, W, dtype, stream, 0);
}

extern "C" int nint_unfold_dx_cyclic(const void* src, float* dst, int N, int C, int k, int Cp, int H, int W, int dtype, void* stream) {
  return unfold_dx_impl(src, dst, N, C, k, Cp, H, W, dtype, stream, 1);
}

extern "C" int nint_unpack_halo(const void* src, float* dst, int n0, int N, int C, int Cp, const nint_geom* g,
                                int dtype, void* stream) {
  if (!src || !dst || !g || N <= 0 || C <= 0 || Cp < C || n0 < 0 || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  const size_t total = (size_t)N * C * g->H * g->W;
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(unpack_halo_kernel<decltype(dt)::value>, grid1d(total), dim3(256), 0, (hipStream_t)stream, src, dst, n0, N, C, Cp, g->H, g->W, g->P, g->Hh, g->Wh);
  });
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_pack_compact(const float* src, void* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0 || Cp < C || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(pack_compact_kernel<decltype(dt)::value>, grid1d((size_t)N * H * W * Cp), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, Cp, H, W);
  });
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_unpack_compact(const void* src, float* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0 || Cp < C || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(unpack_compact_kernel<decltype(dt)::value>, grid1d((size_t)N * C * H * W), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, Cp, H, W);
  });
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// dst += src: a cotangent that arrives as an (N,C,H,W) f32 tensor joins a gradient already in slab form (the final hidden
// state's cotangent on top of the head's dL/dh_{T-1}).  Channel padding is left as it is.
template <int DT>
__global__ void pack_compact_add_kernel(const float* __restrict__ src, void* __restrict__ dst, int N, int C, int Cp,
                                        int H, int W) {
  const size_t total = (size_t)N * H * W * Cp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = i % Cp;
    size_t r = i / Cp;
    const int x = r % W; r /= W;
    const int y = r % H;
    const int n = r / H;
    if (c < C) store_elem<DT>(dst, i, load_elem<DT>(dst, i) + src[(((size_t)n * C + c) * H + y) * W + x]);
  }
}

extern "C" int nint_pack_compact_add(const float* src, void* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0 || Cp < C || H <= 0 || W <= 0 || (dtype != NINT_F32 && dtype != NINT_BF16)) return NINT_E_ARG;
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(pack_compact_add_kernel<decltype(dt)::value>, grid1d((size_t)N * H * W * Cp), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, Cp, H, W);
  });
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// ------------------------------------------------------------------------------ recurrent state hand-off
// (h, c) of every layer from one place to another IN SLAB FORM: slot T of a workspace's stacks -> a stand-alone state, a state
// -> slot 0 of a workspace, a state -> a state through a lane map.  Region r = 2l is layer l's h (ET halo slab images), r = 2l + 1
// its c (f32 compact images); an image is a whole number of 64-byte rows in both layouts, so every region moves as 16-byte
// vectors, and halo-slab images move WHOLE: the source's halo and slack are zero (the slab invariant), so the destination's are
// zero afterwards without a separate fill.  Destination sample b takes source sample lane[b]; lane[b] < 0: zeros (a reset).
// One grid for all of it: z = region, y = destination sample, x strides the image.
struct StateCopyTable {
  const u32x4_t* src[2 * NINT_MAX_LAYERS];
  u32x4_t* dst[2 * NINT_MAX_LAYERS];        // first image of THIS launch's samples
  unsigned nvec[2 * NINT_MAX_LAYERS];       // 16-byte vectors per image
  int lane[NINT_PRE_MAX_B];
};

__global__ __launch_bounds__(256) void state_copy_kernel(StateCopyTable t) {
  const int r = blockIdx.z, b = blockIdx.y;
  const size_t nv = t.nvec[r];
  const int ls = t.lane[b];
  u32x4_t* __restrict__ d = t.dst[r] + (size_t)b * nv;
  const size_t step = (size_t)gridDim.x * 256;
  if (ls < 0) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < nv; i += step) d[i] = (u32x4_t){0u, 0u, 0u, 0u};
    return;
  }
  const u32x4_t* __restrict__ s = t.src[r] + (size_t)ls * nv;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < nv; i += step) d[i] = s[i];
}

extern "C" int nint_state_copy(void* const* h_dst, float* const* c_dst, const void* const* h_src, const float* const* c_src,
                               const int32_t* Chp, int L, int B_dst, int B_src, const int32_t* lane, const nint_geom* g,
                               int dtype, void* stream) {
  if (!h_dst || !c_dst || !h_src || !c_src || !Chp || !g || L < 1 || L > NINT_MAX_LAYERS || B_dst < 1 || B_src < 1) return NINT_E_ARG;
  if (dtype != NINT_F32 && dtype != NINT_BF16) return NINT_E_ARG;
  if (g->H < 1 || g->W < 1 || g->Hh < g->H || g->Wh < g->W) return NINT_E_ARG;
  if (!lane && B_dst != B_src) return NINT_E_ARG;
  for (int b = 0; lane && b < B_dst; ++b)
    if (lane[b] < -1 || lane[b] >= B_src) return NINT_E_ARG;
  const size_t es = dtype == NINT_BF16 ? 2 : 4;
  const int kc = dtype == NINT_BF16 ? 32 : 16;
  StateCopyTable t = {};
  size_t img[2 * NINT_MAX_LAYERS], max_nv = 0;
  for (int l = 0; l < L; ++l) {
    if (Chp[l] < 1 || Chp[l] % kc) return NINT_E_ARG;
    if (!h_dst[l] || !c_dst[l] || !h_src[l] || !c_src[l]) return NINT_E_ARG;
    img[2 * l] = (size_t)g->Hh * g->Wh * Chp[l] * es;
    img[2 * l + 1] = (size_t)g->H * g->W * Chp[l] * sizeof(float);
    t.src[2 * l] = (const u32x4_t*)h_src[l]; t.src[2 * l + 1] = (const u32x4_t*)c_src[l];
    t.dst[2 * l] = (u32x4_t*)h_dst[l]; t.dst[2 * l + 1] = (u32x4_t*)c_dst[l];
  }
  for (int r = 0; r < 2 * L; ++r) {
    if (img[r] / 16 > 0xffffffffu) return NINT_E_SHAPE;
    t.nvec[r] = (unsigned)(img[r] / 16);
    if (t.nvec[r] > max_nv) max_nv = t.nvec[r];
  }
  for (int r = 0; r < 2 * L; ++r)
    if ((((uintptr_t)t.src[r]) | ((uintptr_t)t.dst[r])) & 15) return NINT_E_ALIGN;
  for (int r = 0; r < 2 * L; ++r) {      // a block read while another sample's workgroups write it: refused
    const uintptr_t s0 = (uintptr_t)t.src[r], s1 = s0 + (size_t)B_src * img[r], d0 = (uintptr_t)t.dst[r], d1 = d0 + (size_t)B_dst * img[r];
    if (s0 < d1 && d0 < s1) return NINT_E_ARG;
  }
  // enough workgroups per image to keep every CU's memory pipe busy on one sample, eight vectors per thread at the most
  unsigned gx = (unsigned)((max_nv + 256 * 8 - 1) / (256 * 8));
  if (gx > 64) gx = 64;
  if (gx < 1) gx = 1;
  u32x4_t* dst0[2 * NINT_MAX_LAYERS];
  for (int r = 0; r < 2 * L; ++r) dst0[r] = t.dst[r];
  for (int b0 = 0; b0 < B_dst; b0 += NINT_PRE_MAX_B) {
    const int nb = B_dst - b0 < NINT_PRE_MAX_B ? B_dst - b0 : NINT_PRE_MAX_B;
    for (int i = 0; i < NINT_PRE_MAX_B; ++i) t.lane[i] = i < nb ? (lane ? lane[b0 + i] : b0 + i) : -1;
    for (int r = 0; r < 2 * L; ++r) t.dst[r] = dst0[r] + (size_t)b0 * t.nvec[r];
    hipLaunchKernelGGL(state_copy_kernel, dim3(gx, (unsigned)nb, (unsigned)(2 * L)), dim3(256), 0, (hipStream_t)stream, t);
    NINT_LAUNCH_CHECK();
  }
  return NINT_OK;
}

// ------------------------------------------------------------------------------ cyclic longitude: halo columns
// nint_seq.lon_cyclic.  For every image of a job and every INTERIOR row y in [P, P + H): slab columns [0, P)
// take slab columns [W, W + P) (the last P interior columns) and slab columns [P + W, P + W + P) take [P, 2P) (the first P) --
// or all 2P of them take zeros (CLEAR).  Halo ROWS are not touched: latitude keeps its zero padding.  With W >= P the columns
// read are interior columns and the columns written are halo columns: no lane reads what another writes.  16 bytes per lane;
// blockIdx.y = job, x strides its (image, row, halo pixel, 16-byte vector) items.
__global__ __launch_bounds__(256) void halo_wrap_kernel(WrapTable t) {
  const WrapJob j = t.job[blockIdx.y];
  const size_t nv = (size_t)j.px_bytes >> 4, per_row = 2 * (size_t)t.P * nv;
  const size_t total = (size_t)j.nimg * t.H * per_row;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t v = i % nv, r = i / per_row;
    const int q = (int)((i % per_row) / nv);                     // halo pixel of the row: [0, P) left, [P, 2P) right
    const int y = (int)(r % t.H);
    const size_t img = r / t.H;
    const int dcol = q < t.P ? q : t.W + q, scol = q < t.P ? t.W + q : q;
    char* row = j.base + ((img * t.Hh + (size_t)(y + t.P)) * t.Wh) * j.px_bytes;
    u32x4_t val = {0u, 0u, 0u, 0u};
    if (j.op == NINT_WRAP_COPY) val = *(const u32x4_t*)(row + (size_t)scol * j.px_bytes + v * 16);
    *(u32x4_t*)(row + (size_t)dcol * j.px_bytes + v * 16) = val;
  }
}

int nint_internal_wrap_check(const WrapTable* t) {
  if (!t || t->n < 1 || t->n > NINT_WRAP_MAX_JOBS) return NINT_E_ARG;
  if (t->H < 1 || t->P < 1 || t->W < t->P || t->Hh < t->H + 2 * t->P || t->Wh < t->W + 2 * t->P) return NINT_E_ARG;
  for (int q = 0; q < t->n; ++q) {
    const WrapJob& j = t->job[q];
    if (!j.base || j.nimg < 1 || j.px_bytes < 16 || j.px_bytes % 16 || (j.op != NINT_WRAP_COPY && j.op != NINT_WRAP_CLEAR)) return NINT_E_ARG;
    if (((uintptr_t)j.base) & 15) return NINT_E_ALIGN;
  }
  return NINT_OK;
}

int nint_internal_wrap_enqueue(const WrapTable* t, void* stream) {
  const int rc = nint_internal_wrap_check(t);
  if (rc != NINT_OK) return rc;
  size_t most = 0;
  for (int q = 0; q < t->n; ++q) {
    const size_t items = (size_t)t->job[q].nimg * t->H * 2 * t->P * (t->job[q].px_bytes >> 4);
    if (items > most) most = items;
  }
  unsigned gx = (unsigned)((most + 255) / 256);
  if (gx > 2048) gx = 2048;                    // (the rest by the stride)
  hipLaunchKernelGGL(halo_wrap_kernel, dim3(gx, (unsigned)t->n), dim3(256), 0, (hipStream_t)stream, *t);
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
                                                           int H, int W, int Hp, int Wp, int mode, int P, int Hh, int Wh, int kf,
                                                           int cyc) {
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
  }, kf, cyc);
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

static int preproc_slab_impl(const float* const* srcs, const int* lev, int nsrc, int nstatic,
                             const float* mean, const float* stdv, const int* t0, int B, void* xs_slab,
                             int Cxp, int xfold_k, int T, int H, int W, const nint_geom* g, int mode,
                             int dtype, void* stream, int cyc) {
  if (!mean || !stdv || !xs_slab || !t0 || !g || T <= 0 || B <= 0) return NINT_E_ARG;
  if (cyc && (g->W != W || W < xfold_k / 2)) return NINT_E_ARG;      // (the model wraps at its own edge: no longitude halo in between)
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
    const int rc = nint_by_dtype(dtype, [&](auto dt) { return by_row_vec(vw, [&](auto v) -> int {
      auto kern = preproc_slab_kernel<decltype(dt)::value, decltype(v)::value>;
      if (tile_bytes > 64 * 1024)
        NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
      hipLaunchKernelGGL(kern, grid, dim3(256), tile_bytes, st, a, mean, stdv, xs_slab, B, b0, nb, T, C, Cxp, H, W, Hp, Wp,
                         mode, g->P, g->Hh, g->Wh, kf, cyc);
      return NINT_OK; }); });
    if (rc != NINT_OK) return rc;
    NINT_LAUNCH_CHECK();
  }
  return NINT_OK;
}

extern "C" int nint_preproc_fuse_pad_static_slab(const float* const* srcs, const int* lev, int nsrc, int nstatic,
                                                 const float* mean, const float* stdv, const int* t0, int B, void* xs_slab,
                                                 int Cxp, int xfold_k, int T, int H, int W, const nint_geom* g, int mode,
                                                 int dtype, void* stream) {
  return preproc_slab_impl(srcs, lev, nsrc, nstatic, mean, stdv, t0, B, xs_slab, Cxp, xfold_k, T, H, W, g, mode, dtype, stream, 0);
}

extern "C" int nint_preproc_fuse_pad_static_slab_cyclic(const float* const* srcs, const int* lev, int nsrc, int nstatic,
                                                        const float* mean, const float* stdv, const int* t0, int B, void* xs_slab,
                                                        int Cxp, int xfold_k, int T, int H, int W, const nint_geom* g, int mode,
                                                        int dtype, void* stream) {
  return preproc_slab_impl(srcs, lev, nsrc, nstatic, mean, stdv, t0, B, xs_slab, Cxp, xfold_k, T, H, W, g, mode, dtype, stream, 1);
}

extern "C" int nint_preproc_fuse_pad_slab_cyclic(const float* const* srcs, const int* lev, int nsrc, const float* mean,
                                                 const float* stdv, const int* t0, int B, void* xs_slab, int Cxp, int xfold_k,
                                                 int T, int H, int W, const nint_geom* g, int mode, int dtype, void* stream) {
  return preproc_slab_impl(srcs, lev, nsrc, 0, mean, stdv, t0, B, xs_slab, Cxp, xfold_k, T, H, W, g, mode, dtype, stream, 1);
}

extern "C" int nint_preproc_fuse_pad_slab(const float* const* srcs, const int* lev, int nsrc, const float* mean,
                                          const float* stdv, const int* t0, int B, void* xs_slab, int Cxp, int xfold_k,
                                          int T, int H, int W, const nint_geom* g, int mode, int dtype, void* stream) {
  return nint_preproc_fuse_pad_static_slab(srcs, lev, nsrc, 0, mean, stdv, t0, B, xs_slab, Cxp, xfold_k, T, H, W, g, mode,
                                           dtype, stream);
}
