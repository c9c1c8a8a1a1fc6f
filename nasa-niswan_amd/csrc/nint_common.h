// nint_common.h -- shared device/host helpers for the gfx950 ConvLSTM kernels.
// Written for CDNA4 only: 64-wide waves, MFMA 16x16 tiles, 160 KiB LDS, no other targets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "nint.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;

#define NINT_CHECK_HIP(expr)                      \
  do {                                            \
    hipError_t _e = (expr);                       \
    if (_e != hipSuccess) return (int)_e;         \
  } while (0)

#define NINT_LAUNCH_CHECK()                       \
  do {                                            \
    hipError_t _e = hipGetLastError();            \
    if (_e != hipSuccess) return (int)_e;         \
  } while (0)

// Element-type traits. One K-step of the implicit GEMMs always covers 64 BYTES of channels
// per pixel: 32 bf16 (one v_mfma_f32_16x16x32_bf16) or 16 f32 (four v_mfma_f32_16x16x4_f32).
template <int DT> struct Elem;
template <> struct Elem<NINT_F32> {
  typedef float type;
  static constexpr int ES = 4;    // bytes per element
  static constexpr int KC = 16;   // channels per K-step
  static constexpr int EPL = 4;   // elements per lane per K-step (16 bytes)
};
template <> struct Elem<NINT_BF16> {
  typedef __bf16 type;
  static constexpr int ES = 2;
  static constexpr int KC = 32;
  static constexpr int EPL = 8;
};

__host__ __device__ inline int nint_round_up(int a, int b) { return (a + b - 1) / b * b; }
__host__ __device__ inline int nint_cdiv(int a, int b) { return (a + b - 1) / b; }

// Host side: pick a kernel's DT instance.  f is a generic lambda called with std::integral_constant<int, NINT_BF16 | NINT_F32>
// (decltype(dt)::value is the template argument); the caller has checked dtype.
template <class F> static inline auto nint_by_dtype(int dtype, F&& f) {
  if (dtype == NINT_BF16) return f(std::integral_constant<int, NINT_BF16>{});
  return f(std::integral_constant<int, NINT_F32>{});
}

// grid of a grid-stride kernel over n items
static inline dim3 grid1d(size_t n, int block = 256) {
  size_t g = (n + block - 1) / block;
  if (g > 256 * 32) g = 256 * 32;   // grid-stride the rest (256 CUs x 32)
  if (g < 1) g = 1;
  return dim3((unsigned)g);
}

// float -> bf16 round-to-nearest-even; the plain cast lowers to v_cvt_pk_bf16_f32 on gfx950
// and keeps NaN a NaN (MI355X_MICROARCH.md, correctness boundaries).
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(uint16_t, h);
}
// two floats -> one dword of two bf16 (low half = first): a single v_cvt_pk_bf16_f32
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  bf16x2_t v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float bf2f(uint16_t u) { return __builtin_bit_cast(float, (uint32_t)u << 16); }

template <int DT> __device__ __forceinline__ float load_elem(const void* p, size_t i);
template <> __device__ __forceinline__ float load_elem<NINT_F32>(const void* p, size_t i) { return ((const float*)p)[i]; }
template <> __device__ __forceinline__ float load_elem<NINT_BF16>(const void* p, size_t i) { return bf2f(((const uint16_t*)p)[i]); }
template <int DT> __device__ __forceinline__ void store_elem(void* p, size_t i, float v);
template <> __device__ __forceinline__ void store_elem<NINT_F32>(void* p, size_t i, float v) { ((float*)p)[i] = v; }
template <> __device__ __forceinline__ void store_elem<NINT_BF16>(void* p, size_t i, float v) { ((uint16_t*)p)[i] = f2bf(v); }

// 4 consecutive elements (16-byte f32 / 8-byte bf16 vector store); i must be a multiple of 4
template <int DT> __device__ __forceinline__ void store_vec4(void* p, size_t i, f32x4_t v);
template <> __device__ __forceinline__ void store_vec4<NINT_F32>(void* p, size_t i, f32x4_t v) {
  *(f32x4_t*)((float*)p + i) = v;
}
template <> __device__ __forceinline__ void store_vec4<NINT_BF16>(void* p, size_t i, f32x4_t v) {
  u32x2_t w;
  w[0] = pack_bf16x2(v[0], v[1]);
  w[1] = pack_bf16x2(v[2], v[3]);
  *(u32x2_t*)((uint16_t*)p + i) = w;
}

// 4 consecutive elements as f32 (16-byte f32 / 8-byte bf16 vector load); i must be a multiple of 4
template <int DT> __device__ __forceinline__ f32x4_t load_vec4(const void* p, size_t i);
template <> __device__ __forceinline__ f32x4_t load_vec4<NINT_F32>(const void* p, size_t i) { return *(const f32x4_t*)((const float*)p + i); }
template <> __device__ __forceinline__ f32x4_t load_vec4<NINT_BF16>(const void* p, size_t i) {
  const u32x2_t w = *(const u32x2_t*)((const uint16_t*)p + i);
  return (f32x4_t){__builtin_bit_cast(float, w[0] << 16), __builtin_bit_cast(float, w[0] & 0xffff0000u),
                   __builtin_bit_cast(float, w[1] << 16), __builtin_bit_cast(float, w[1] & 0xffff0000u)};
}

// One K-step of D += A*B on a 16x16 tile from two 16-byte fragments.
//   bf16: lane l holds A[row l&15][k = 8*(l>>4)+j], B[k = 8*(l>>4)+j][col l&15], j=0..7
//   f32 : four MFMAs; in MFMA j lane l supplies A[row l&15][k = l>>4] = element j of its fragment,
//         i.e. channel 4*(l>>4)+j of the K-step -- the same bytes-per-lane geometry as bf16.
template <int DT> __device__ __forceinline__ f32x4_t mma_step(u32x4_t a, u32x4_t b, f32x4_t c);
template <> __device__ __forceinline__ f32x4_t mma_step<NINT_BF16>(u32x4_t a, u32x4_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4_t mma_step<NINT_F32>(u32x4_t a, u32x4_t b, f32x4_t c) {
  f32x4_t af = __builtin_bit_cast(f32x4_t, a), bf = __builtin_bit_cast(f32x4_t, b);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[0], bf[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[1], bf[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[2], bf[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[3], bf[3], c, 0, 0, 0);
  return c;
}

// Reciprocal by v_rcp_f32 (1 ulp): an IEEE division costs ~10 VALU instructions (div_scale x2, rcp, 4 fma,
// div_fmas, div_fixup) and the LSTM epilogue does five per element -- it was half of the epilogue's VALU work.
__device__ __forceinline__ float rcpf_(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sigmoidf_(float x) { return rcpf_(1.0f + __expf(-x)); }
// tanh(x) = 2*sigmoid(2x) - 1: five instructions (mul, exp, add, rcp, fma); saturates cleanly (exp overflow ->
// inf -> rcp 0 -> -1; underflow -> 0 -> rcp(1) -> 1); absolute error ~1e-7 (cancellation near 0 is absolute, not relative)
__device__ __forceinline__ float tanhf_(float x) { return fmaf(2.0f, rcpf_(1.0f + __expf(-2.0f * x)), -1.0f); }

// One element of the LSTM cell (model.py:223-229) from its four pre-activations (bias included) and c_{t-1}.  The ONE definition:
// the MFMA epilogue (conv_igemm.hip: epi_lstm), stencil.hip and tiny_gemm.hip call it, so every kernel family agrees bit for bit
// (oracle/stored_audit.py relies on that).  The association of c is pinned: fmaf(c_prev, f, i * g).  A padding channel's
// `pad ? 0.f : acc` select stays at the caller.
struct LstmCell { float i, f, g, o, c, h; };
__device__ __forceinline__ LstmCell lstm_cell_elem(float ai, float af, float ag, float ao, float c_prev) {
  LstmCell e;
  e.i = sigmoidf_(ai);
  e.f = sigmoidf_(af);
  e.g = tanhf_(ag);
  e.o = sigmoidf_(ao);
  e.c = fmaf(c_prev, e.f, e.i * e.g);        // model.py:228
  e.h = e.o * tanhf_(e.c);                   // model.py:229
  return e;
}
// What the gate stash holds for a channel with zero weights and zero bias (pre-activation 0): i, f, g, o = 0.5, 0.5, 0, 0.5
constexpr float lstm_stash_zero_w(int gate) { return gate == 2 ? 0.f : 0.5f; }

// One element of the pointwise LSTM backward (autograd of model.py:222-229) from the stashed gates, c_{t-1}, c_t, d/dh_t and d/dc_t:
//   dct = dc + dh*o*(1 - tanh(c_t)^2);  dG = (dct*g*i(1-i), dct*c_{t-1}*f(1-f), dct*i*(1-g^2), dh*tanh(c_t)*o(1-o));  dc_{t-1} = dct*f
// Called by lstm_bwd_pointwise_body below and by the fused dgrad epilogue (conv_igemm.hip: epi_dgrad_pw).
struct LstmBwd { float d_i, d_f, d_g, d_o, dc_prev; };
__device__ __forceinline__ LstmBwd lstm_bwd_elem(float i, float f, float g, float o, float c_prev, float c, float dh, float dc) {
  const float tc = tanhf_(c);
  const float dct = dc + dh * o * (1.f - tc * tc);
  const float d_o = dh * tc;
  return {dct * g * i * (1.f - i), dct * c_prev * f * (1.f - f), dct * i * (1.f - g * g), d_o * o * (1.f - o), dct * f};
}

// LSTM pointwise backward (pointwise.hip: lstm_bwd_pointwise_kernel; also a problem of conv_bwd_multi_kernel, nint_seq.wave = 4):
// block `blk` of `nblk` 256-thread blocks, grid-stride over (pixel, 4 consecutive hidden channels).
struct PwArgs {
  const void* gates; const float* c_prev; const float* c_new; const void* dh; const void* dh2; float* dc; void* dG;
  int N, H, W, P, Hh, Wh, Ch16, Chp, dc_zero;
};
template <int DT, int U = 1>
__device__ __forceinline__ void lstm_bwd_pointwise_body(const PwArgs& a, size_t blk, size_t nblk) {
  // U items per thread and loop turn, all loads of a turn issued before the first store (U = 2 inside conv_bwd_multi_kernel, where
  // the pass runs at that kernel's occupancy -- 4 workgroups per CU instead of 8 -- and needs the loads in flight per thread instead)
  const int nq = a.Ch16 >> 2;
  const size_t total = (size_t)a.N * a.H * a.W * nq;
  const int Gc = 4 * a.Ch16;
  const size_t stride = nblk * 256;
  for (size_t i0 = blk * 256 + threadIdx.x; i0 < total; i0 += stride * U) {
    f32x4_t gi[U], gf[U], gg[U], go[U], cp[U], cn[U], dhv[U], dcv[U];
    size_t ci[U], ob[U];
    bool on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + (size_t)u * stride;
      on[u] = i < total;
      if (!on[u]) continue;
      const int q = i % nq;
      const size_t pix = i / nq;
      const int x = pix % a.W;
      size_t r = pix / a.W;
      const int y = r % a.H;
      const int n = r / a.H;
      const int ch = 4 * q;
      const int cblock = ch >> 4, col = ch & 15;
      const size_t gb = pix * Gc + (size_t)cblock * 64 + col;
      gi[u] = load_vec4<DT>(a.gates, gb);
      gf[u] = load_vec4<DT>(a.gates, gb + 16);
      gg[u] = load_vec4<DT>(a.gates, gb + 32);
      go[u] = load_vec4<DT>(a.gates, gb + 48);
      ci[u] = pix * a.Chp + ch;
      cp[u] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      if (a.c_prev) cp[u] = *(const f32x4_t*)(a.c_prev + ci[u]);
      cn[u] = *(const f32x4_t*)(a.c_new + ci[u]);
      dhv[u] = load_vec4<DT>(a.dh, ci[u]);
      if (a.dh2) dhv[u] += load_vec4<DT>(a.dh2, ci[u]);  // d/dh in two pieces (nint_seq.wave = 4: the x columns of the layer above + the layer's own h columns)
      dcv[u] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      if (!a.dc_zero) dcv[u] = *(const f32x4_t*)(a.dc + ci[u]);
      ob[u] = ((((size_t)n * a.Hh) + (y + a.P)) * a.Wh + (x + a.P)) * Gc + (size_t)cblock * 64 + col;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!on[u]) continue;
      f32x4_t o_i, o_f, o_g, o_o, dcp;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const LstmBwd b = lstm_bwd_elem(gi[u][e], gf[u][e], gg[u][e], go[u][e], cp[u][e], cn[u][e], dhv[u][e], dcv[u][e]);
        o_i[e] = b.d_i; o_f[e] = b.d_f; o_g[e] = b.d_g; o_o[e] = b.d_o; dcp[e] = b.dc_prev;
      }
      store_vec4<DT>(a.dG, ob[u], o_i);
      store_vec4<DT>(a.dG, ob[u] + 16, o_f);
      store_vec4<DT>(a.dG, ob[u] + 32, o_g);
      store_vec4<DT>(a.dG, ob[u] + 48, o_o);
      *(f32x4_t*)(a.dc + ci[u]) = dcp;
    }
  }
}

// Sum of v[k] over the wave's 64 lanes for k = 0..7 at once: three halving exchanges (each lane keeps half of its values and
// takes the partner's for them), then three plain ones.  Lane 8*k ends with the total of v[k] (every lane of 8k..8k+7 does).
// (head.hip: the skill sums' sample rows; ensemble.hip: the ensemble sums'.)
__device__ __forceinline__ double skill_wave_fold(const double (&v)[8], int lane) {
  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
  double a[4], c[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = (b5 ? v[j + 4] : v[j]) + __shfl_xor(b5 ? v[j] : v[j + 4], 32);
#pragma unroll
  for (int j = 0; j < 2; ++j) c[j] = (b4 ? a[j + 2] : a[j]) + __shfl_xor(b4 ? a[j] : a[j + 2], 16);
  double s = (b3 ? c[1] : c[0]) + __shfl_xor(b3 ? c[0] : c[1], 8);   // the value k = lane >> 3 over the 8 lanes that share lane & 7
  s += __shfl_xor(s, 4);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  return s;
}

// ---- the noise generator: noise.hip (nint_input_noise, nint_noise_normal) and head.hip (the noise on the
// fed-back value, nint_feedback_noise) inline these, so a value is the same number whichever kernel draws it
// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
__device__ __forceinline__ u32x4_t philox4x32_10(u32x4_t c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
    c = (u32x4_t){h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0};
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}

// one word pair -> two normals (Box-Muller): u in [2^-24, 1 - 2^-24] and a in [0, 2) are exact in f32; precise logf / sqrtf /
// sincospif (no file of the library is built with fast-math forms)
__device__ __forceinline__ void noise_pair(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float u = ((float)(wa >> 9) + 0.5f) * 0x1p-23f;
  const float a = (float)(wb >> 8) * 0x1p-23f;
  const float r = sqrtf(-2.f * logf(u));
  float s, c;
  sincospif(a, &s, &c);
  z0 = r * c; z1 = r * s;
}

// THE device function every kernel inlines: the four normals of channel offsets 4q .. 4q + 3 of one pixel
__device__ __forceinline__ f32x4_t noise_quad(uint32_t pix, uint32_t q, uint32_t step, uint32_t lane, uint32_t seed, uint32_t draw) {
  const u32x4_t w = philox4x32_10((u32x4_t){pix, q, step, lane}, seed, draw);
  f32x4_t z;
  float z0, z1;
  noise_pair(w[0], w[1], z0, z1); z[0] = z0; z[1] = z1;
  noise_pair(w[2], w[3], z0, z1); z[2] = z0; z[3] = z1;
  return z;
}

// launcher-side descriptors -----------------------------------------------------------------
struct ConvArgs {
  const char* src0;      // halo slab (x for fwd, dG for dgrad)
  const char* src1;      // second halo slab (h_prev) or nullptr
  int nchunk0, nchunk1;  // 64-byte channel chunks taken from src0 / src1
  long img_stride0, img_stride1;  // bytes per image
  int pix_stride0, pix_stride1;   // bytes per pixel
  const char* Bp;        // packed weights [S][NTt][64 lanes][16 B]
  int NTt;               // n-tiles per K-step in Bp
  int nt_begin;          // first n-tile this launch computes
  int k, p, taps;
  int kx0;               // horizontal taps of src0: k, or 1 for a horizontally folded x source (nint_layer.xfold)
  int H, W, P, Hh, Wh;
  int tiles_x, tiles_y;
  int tiles_full_y, tiles_x2, n_full;   // full tile rows, merged tiles per image (0: none), number of full tiles in the launch
  int nhp_pad2;                         // halo-tile pixels of a merged tile (MT/2 rows x 32 pixels), rounded up to 16
  unsigned magic_nhpp2, magic_hwt2;
  int tile_rows;         // 0 = per launch shape, 4 / 8 = forced tile height
  int cpf;               // channel chunks per LDS A fill
  int a_bytes;           // bytes reserved for the A image
  int nhp_pad;           // halo-tile pixels rounded up to 16 (one g-plane of the A image)
  unsigned magic_nhpp, magic_hwt;   // ceil(2^32 / nhp_pad), ceil(2^32 / (16 + 2p)): division by multiply-high in the fill
  // LSTM epilogue
  const float* bias;     // [4*Ch16] permuted
  const float* c_prev;   // compact [N][H][W][Chp] or nullptr (= 0)
  float* c_out;
  char* h_out;           // halo slab, ET
  char* gates_out;       // stash [N][H][W][4*Ch16] ET or nullptr
  int Chp, Ch16;
  int Ch;                // LSTM epilogue: real hidden channels; the gate columns of channels [Ch, Ch16) are padding (zero weights)
  // DGRAD epilogue
  char* out0;            // += columns [0, C0p)  (ET compact)
  char* out1;            // =  columns [C0p, C0p+C1p)  (ET compact)
  int C0p, C1p;
  int out0_overwrite;    // 1: columns [0, C0p) are stored, not accumulated (the destination is known to be zero)
  // DGRAD_PW epilogue: the pointwise LSTM backward of the previous time step on the h columns (Chp / Ch16 as above)
  const char* pw_gates;  // gate stash of that step [N][H][W][4*Ch16] ET
  const float* pw_c_prev;// c_{t-1} compact f32 or nullptr (= 0)
  const float* pw_c_new; // c_t
  float* pw_dc;          // d/dc, read and overwritten in place
  const char* pw_old;    // the x columns the layer above left for this step (ET compact [N][H][W][Chp]) or nullptr
  char* pw_dG;           // dG halo slab of that step
  // ... and of the layer BELOW at this launch's own time step, on the x columns (lo_gates == nullptr: x columns stored)
  const char* lo_gates; const float* lo_c_prev; const float* lo_c_new; float* lo_dc; char* lo_dG;
  int lo_Ch16, lo_dc_zero;
};

// internal entry points shared between translation units (not part of the C ABI).  Every launch of a sequence pass has a PLANNED
// form: a pure function checks the arguments and fills the record (host arithmetic only), an enqueue function does nothing but launch
// (planned, then enqueued: the first checks the arguments and fills *plan, the second launches lstm_bwd_pointwise_kernel)
int nint_internal_pointwise_plan(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* gates,
                                 const float* c_prev, const float* c_new, const void* dh, float* dc, void* dG,
                                 bool dc_zero, const void* dh2, PwArgs* plan);                 // dh2: a second piece of d/dh, added (or nullptr)
int nint_internal_pointwise_enqueue(const PwArgs* plan, int dtype, void* stream);
struct WgJob {           // one layer's weight / bias gradient
  const nint_layer* ly; int N;
  const void* dG; const void* x_slab; const void* h_slab;
  float* dW; float* db;
  int h_skip;                                // leading images whose h source is identically zero
};
// wgrad.hip: the argument blocks of wgrad_kernel / wgrad_wide_kernel (WgradArgs) and of wgrad_reduce_kernel (ReduceTable)
struct WgSrc {           // one source (x or h) of a launch
  const char* dG;        // first image of this source's reduction (the h source may skip the zero-state time step)
  const char* src; long src_img_stride; int src_pix_stride;
  float* partial;
  int CB, JG;            // channel blocks; columns per block slab (the x source's slabs carry the bias-gradient column)
  int nblk;              // workgroup columns of this source: NB * CB * TG
  int ntiles, tiles_per_split;
  int want_db;           // 1: the slab's last column (JG-1) carries the bias gradient (column sums of dG; wgrad.hip)
};
struct WgradArgs {
  long dG_img_stride; int dG_pix_stride;
  WgSrc s[2];
  int nparts;            // 1, or 2: BOTH sources in one launch (same kernel shape), their workgroups interleaved per gate block so
                         // that the x and h workgroups of a pixel range run together and share the dG tiles in L2
  int NTC, J;            // channel tiles per block, (tap, channel-tile) columns in all
  int TG;                // column groups of 4*JW columns (49 taps of a 7x7 kernel: 2)
  int k, p, taps;
  int P, Wh;
  int tiles_x, tiles_y;
};
struct ReduceEntry {
  const float* part; float* dW;
  int Cx, Ch, Ch16, k, NB, CB, NTC, J, splits, is_h, xfold;
  int TG, JG;                               // column groups per block column, columns per block slab (incl. the db column)
  float* db;                                // non-NULL: slab column JG-1 of (channel block 0, last group) is the bias gradient
  int waves;                                // waves that share the splits of one 64-element line (the others exit)
  unsigned blk_begin;                       // first workgroup of this (layer, source) in the merged launch
};
struct ReduceTable { ReduceEntry e[2 * NINT_MAX_LAYERS]; int n; int acc; };   // acc (nint_seq.accumulate): 1 = dW / db += the sum
// The weight / bias gradients of jobs[0..n), planned: per job ONE launch (both sources merged) or two (x, then h) into consecutive
// regions of `partial`, and one fold of every split-K slab of every job into its dW and db.
struct WgLaunch { const void* kern; int gx, gy, block; size_t lds; WgradArgs a; };   // kern: host handle of the wgrad[_wide]_kernel<...> instantiation
struct WgJobPlan { WgLaunch launch[2]; int n; };
struct WgFoldPlan { ReduceTable t; unsigned grid; int block; };
// pure: every check (job pointers, h_skip, shape, LDS, workspace room) is made here; nothing is enqueued
int nint_internal_wgrad_plan(const WgJob* jobs, int njobs, const nint_geom* g, int dtype, float* partial, size_t partial_bytes,
                             int n_cu, WgJobPlan* plans, WgFoldPlan* fold);
int nint_internal_wgrad_enqueue(const WgJobPlan* plan, void* stream);
int nint_internal_wgrad_fold_enqueue(const WgFoldPlan* fold, void* stream);
// stencil.hip: the gate step of tiny hidden widths (Ch <= 8, 3x3) on the vector ALU.  Its weight image -- one row of 32 f32 per
// (tap, channel) in the kernel's iteration order -- sits behind the MFMA images in the Wf buffer (nint_pack_weights).
__host__ __device__ inline bool nint_stencil_shape(int Cx, int Ch, int k, int xfold) {
  return k == 3 && Ch <= 8 && (xfold ? 3 * Cx <= 64 : Cx <= 16);
}
__host__ __device__ inline int nint_stencil_rows(int Cx, int Ch, int xfold) {     // rows per vertical tap: x part + h part
  return (xfold ? 4 * nint_cdiv(3 * Cx, 4) : 12 * nint_cdiv(Cx, 4)) + 12 * nint_cdiv(Ch, 4);
}
__host__ __device__ inline size_t nint_internal_stencil_offset(int Cxp, int Chp, int Ch16, int k, int dtype) {
  const size_t img = (size_t)(Cxp + Chp) * 4 * Ch16 * k * k * (dtype == NINT_BF16 ? 2 : 4);    // both MFMA images fit in this
  return (img + 255) / 256 * 256;
}
// tiny_gemm.hip: the same layers on the matrix pipe with a DENSE K: K is a list of 16-byte groups (8 bf16 / 4 f32 channels of one
// halo pixel of one source), four groups per K-step.  Group order: the x source's groups (folded: per vertical tap the centre
// pixel's xg groups; plain: per tap (ky, kx) the pixel's xg groups), then the h source's (per tap, hg groups).
constexpr int NINT_TINY_MAXSTEPS = 12, NINT_TINY_HW = 34;      // K-steps a wave keeps in registers; halo tile width (32 + 2)
__host__ __device__ inline int nint_tiny_xg(int Cx, int xfold, int dtype) { return nint_cdiv((xfold ? 3 * Cx : Cx) * (dtype == NINT_BF16 ? 2 : 4), 16); }
__host__ __device__ inline int nint_tiny_hg(int Ch, int dtype) { return nint_cdiv(Ch * (dtype == NINT_BF16 ? 2 : 4), 16); }
__host__ __device__ inline int nint_tiny_ngx(int Cx, int xfold, int dtype) { return (xfold ? 3 : 9) * nint_tiny_xg(Cx, xfold, dtype); }
__host__ __device__ inline bool nint_tiny_shape(int Cx, int Ch, int k, int xfold, int dtype) {
  return nint_stencil_shape(Cx, Ch, k, xfold) &&
         nint_cdiv(nint_tiny_ngx(Cx, xfold, dtype) + 9 * nint_tiny_hg(Ch, dtype), 4) <= NINT_TINY_MAXSTEPS;
}
__host__ __device__ inline size_t nint_tiny_bytes() { return (size_t)NINT_TINY_MAXSTEPS * 2 * 1024 + 4 * NINT_TINY_MAXSTEPS * sizeof(int) + 64; }
__host__ __device__ inline size_t nint_internal_tiny_offset(int Cx, int Cxp, int Ch, int Chp, int Ch16, int k, int xfold, int dtype) {
  const size_t o = nint_internal_stencil_offset(Cxp, Chp, Ch16, k, dtype) + ((size_t)3 * nint_stencil_rows(Cx, Ch, xfold) + 1) * 128;
  return (o + 255) / 256 * 256;
}
int nint_internal_tiny_lstm(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* x_slab,
                            const void* h_prev, const float* c_prev, void* h_out, float* c_out, void* gates_out,
                            void* stream);
bool nint_internal_stencil_holds(const nint_layer* ly);
int nint_internal_stencil_lstm(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* x_slab,
                               const void* h_prev, const float* c_prev, void* h_out, float* c_out, void* gates_out,
                               void* stream);
// pack.hip: cyclic longitude (nint_seq.lon_cyclic).  One launch of halo_wrap_kernel serves a table of jobs; a job is a block of halo
// slab images whose halo COLUMNS, on the interior rows, receive the wrapped interior columns (WRAP) or zeros (CLEAR).
enum { NINT_WRAP_COPY = 0, NINT_WRAP_CLEAR = 1 };
#define NINT_WRAP_MAX_JOBS 12
struct WrapJob { char* base; int nimg; int px_bytes; int op; };       // first image, images, bytes per pixel (a multiple of 16)
struct WrapTable { WrapJob job[NINT_WRAP_MAX_JOBS]; int n; int H, W, P, Hh, Wh; };
// pure: the geometry and every job are checked (W >= P, 16-byte pixels and bases) -- NINT_E_ARG / NINT_E_ALIGN, nothing enqueued
int nint_internal_wrap_check(const WrapTable* t);
int nint_internal_wrap_enqueue(const WrapTable* t, void* stream);
// head.hip: the feedback step of the closed-loop forward (nint_seq.fb_O; nint_head_feedback's arguments)
struct FbPlan {
  const void* h; const float* w; const float* b; void* xs;       // h, xs: the FIRST image read / written
  int N, Ch, Chp, O, Cx, Cxp, c0, kf, cyc, dtype;                // kf: 1 = plain slab, k = folded
  int H, W, P, Hh, Wh;
  size_t lds;
  // SCHEDULED SAMPLING.  sel = 1: the masked instantiation, which feeds image i only where bit i of `mask` is set
  // (N <= 64).  sel = 0, what every plan function below leaves: the unmasked kernels, which never read the word.
  unsigned long long mask; int sel;
  // RESIDUAL HEAD.  res = 1: the instantiation that adds the base -- the value stored in the feedback channels of
  // the images from xb on, the pixel's own copy in a folded slab -- to the dot product before the rounding.  res = 0, what every
  // plan function below leaves: the kernels without it, which never read the pointer.
  const void* xb; int res;
};
// NOISE ON THE FED-BACK VALUE: the plan with the noise's fields behind it.  nz = 1: the instantiation that adds
// __fmul_rn(sigma[o], z) to the f32 value before the rounding, z = noise_quad's normal of (pixel, o, nz_step, nz_lane0 + image), and
// takes this whole structure.  nz = 0, what every plan function below leaves: the kernels without it, whose argument stays the FbPlan
// above -- so they are, byte for byte, the kernels they were.
struct FbPlanNz : FbPlan {
  const float* nz_sigma; uint32_t nz_seed, nz_draw, nz_step, nz_lane0; int nz;
};
// The mask word of N images from N HOST bytes, each 0 or 1 (nint_feedback_mask, nint_head_feedback_sel): NINT_E_ARG for a NULL
// pointer or any other byte, then NINT_E_SHAPE for more images than the word has bits.
static inline int nint_internal_mask_word(const unsigned char* fed, int N, unsigned long long* word) {
  if (!fed || N < 0) return NINT_E_ARG;
  unsigned long long m = 0;
  for (int i = 0; i < N; ++i) {
    if (fed[i] > 1) return NINT_E_ARG;
    if (i < 64 && fed[i]) m |= 1ull << i;
  }
  if (N > 64) return NINT_E_SHAPE;
  *word = m;
  return NINT_OK;
}
// pure: every check of nint_head_feedback (NINT_E_ARG / NINT_E_ALIGN / NINT_E_SHAPE) is made here and *plan filled; nothing is enqueued
int nint_internal_feedback_plan(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g,
                                int dtype, FbPlan* plan);
int nint_internal_feedback_enqueue(const FbPlanNz* plan, void* stream);
// residual head: the planned launch reads its base from images [base_n0, base_n0 + N) of the slab it writes [x_n0, x_n0 + N) of
int nint_internal_feedback_base(FbPlan* plan, const void* xs_slab, int x_n0, int base_n0, int N);
// noise on the stored value: the planned launch draws for step `step`; fn == nullptr or fn->sigma == nullptr leaves the plan as it is
int nint_internal_feedback_noise(FbPlanNz* plan, const nint_feedback_noise* fn, uint32_t step);
// ... and its adjoint, the feedback step of the roll-out backward (nint_head_feedback_bwd's arguments)
struct FbBwdPlan {
  const void* dx; float* dpred; void* dh; const float* w;        // dx, dpred, dh: the FIRST image read / written
  int N, Ch, Chp, O, Cx, Cxp, c0, kf, cyc, dtype;                // kf: 1 = plain slab, k = folded
  int H, W;
  size_t lds;
  unsigned long long mask; int sel;                              // as in FbPlan; per thread here: a workgroup straddles images
  const float* pnext; int res;                                   // residual head: g += dpred of the fed step itself, images from pnext on (res = 1)
};
int nint_internal_feedback_bwd_plan(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch, int Chp,
                                    int O, const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g,
                                    int dtype, FbBwdPlan* plan);
int nint_internal_feedback_bwd_enqueue(const FbBwdPlan* plan, void* stream);
// head.hip: skill_fold_kernel, the fixed-order fold of NP partial rows of eight f64 per pair into sample[pair][8] -- the second
// launch of nint_skill_accum / nint_head_skill_accum and of nint_ens_accum (ensemble.hip)
int nint_internal_skill_fold_enqueue(const double* part, double* sample, int npair, int NP, void* stream);
#define NINT_MULTI_MAX 4  // problems per merged grid (the kernels of NINT_MULTI_KERNELS, csrc/conv_igemm.hip)
struct CellFwdJob {      // one gate launch (nint_cell_fwd's arguments)
  const nint_layer* ly; const void* x_slab; const void* h_prev; const float* c_prev; void* h_out; float* c_out; void* gates_out;
};
// A conv_igemm launch, planned: every conv launch is planned first (cell_fwd / nint_internal_conv_dgrad) and enqueued from its
// plan (nint_internal_conv_enqueue), by itself or with other independent ones as ONE grid (nint_internal_multi_*).
struct ConvPlan {
  ConvArgs a; int gx, gy; size_t lds; int variant;   // grid (gx == 0: nothing to launch), dynamic LDS, kernel shape (conv_variant)
  const void* kern;                                  // host handle of the conv_igemm_kernel<...> instantiation
  int carrier;                                       // NINT_K_CONV_IGEMM; NINT_K_STENCIL / NINT_K_TINY with NINT_E_SHAPE: no planned form
};
constexpr int conv_variant(int EPI, int WN, int WK, int NTW, int MT) { return EPI * 10000 + WN * 1000 + WK * 100 + NTW * 10 + MT / 4; }
struct ConvShape { int epi, wn, wk, ntw, mt; };      // ... and its inverse (the bodies and their carriers: csrc/conv_igemm.hip, "the shape table")
constexpr ConvShape conv_shape(int v) { return {v / 10000, v / 1000 % 10, v / 100 % 10, v / 10 % 10, 4 * (v % 10)}; }
int nint_internal_n_cu();                            // CUs of the current device; 256 where the lookup fails
// n_cu: the CU count the launch-shape rules use (<= 0: looked up here)
int nint_internal_cell_fwd_plan(const CellFwdJob* j, const nint_geom* g, int dtype, int N, int n_cu, ConvPlan* plan);
int nint_internal_conv_enqueue(const ConvPlan* plan, void* stream);
// Independent planned launches in ONE grid: the argument block of conv_lstm_multi[8]_kernel / conv_bwd_multi[8]_kernel /
// conv_dgrad_multi8_kernel (csrc/conv_igemm.hip).
struct ConvMulti {
  ConvArgs a[NINT_MULTI_MAX];
  int n;
  int begin[NINT_MULTI_MAX + 1];     // first workgroup of each problem (multiples of 8); begin[n] = grid size
  int nbx[NINT_MULTI_MAX];           // pixel-tile workgroups of each problem (its launch's gridDim.x); column group = (b - begin) / nbx
  int nwg[NINT_MULTI_MAX];           // nbx * column groups: workgroups past it are padding
  int variant[NINT_MULTI_MAX];
  PwArgs pw;                         // conv_bwd_multi_kernel only: workgroups [begin[n], begin[n] + pw_blocks) run a pointwise LSTM backward pass
  int pw_blocks;
};
struct MultiPlan { ConvMulti m; int carrier, grid; size_t lds; };     // carrier: NINT_K_CONV_LSTM_MULTI ... NINT_K_CONV_DGRAD_MULTI8
// pure: the merged kernel that holds plans[0..n) (pw: plus one pointwise backward pass), its argument block, grid and LDS -- or
// NINT_E_SHAPE: one of them has a shape the merged kernels do not hold, or they are of both kinds (the caller enqueues them one by one)
int nint_internal_multi_plan(const ConvPlan* plans, int n, const PwArgs* pw, MultiPlan* out);
int nint_internal_multi_enqueue(const MultiPlan* mp, int dtype, void* stream);
struct DgradPw {         // fused pointwise backward of the previous time step (EPI_DGRAD_PW)
  const void* gates; const float* c_prev; const float* c_new; float* dc; const void* old; void* dG_out;
  // optional: the layer below's pointwise backward of THIS time step, run on the x columns (the layer's dh buffer is only read)
  const void* lo_gates; const float* lo_c_prev; const float* lo_c_new; float* lo_dc; void* lo_dG_out; int lo_Ch16; bool lo_dc_zero;
  int tile_rows;          // 0 = the layer's choice, 4 / 8 = this launch's tile height
};
// *plan describes the launch (plan->gx == 0: there is nothing to launch); nothing is enqueued
int nint_internal_conv_dgrad(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* dG, void* dx_accum,
                             void* dh_prev, bool overwrite_dx, const DgradPw* pw, int n_cu, ConvPlan* plan);
