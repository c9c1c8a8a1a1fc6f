// head.hip -- the 1x1 head on the top layer's hidden state (forward, d/dh, weight / bias gradient), the crop loss (the
// reference's MSE + L1, with a weight map, or the configurable mix: one kernel pair over a compile-time "loss element"), and
// the two fused into one pass over the pixels; each for one step's images or for every step of a sequence.  They share
// head_stage_weights, head_dot, the loss elements, LOSS_WG_FOLD, LOSS_BLOCKS_MAX and loss_final_kernel.  Every kernel body is
// a __forceinline__ device function under ONE __global__ wrapper templated on SEQ: the register allocation depends on that
// function boundary.  So does all compiled code on what stands behind a call before the inliner runs: the early passes see
// the kernel without it.  Whatever the loss elements' functions hold is therefore plain arithmetic on values -- no index
// arithmetic, no object with a constructor, sums in and out by value -- and the instances that existed before the elements
// compile to the instruction streams they had (profiles/head_refactor_asm.txt).
#include "nint_common.h"
#include <algorithm>
#include <cfloat>
#include <climits>

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

// THE dot product of the staged head (normative; restated in nint.h and DESIGN.md 4.14):
//   the accumulator starts from the bias (0 without one); the CHV staged channels join it in order; the first CHV - 12 by
//   fused multiply-add (one rounding), the last 12 as a rounded product, then a rounded add.
// (What the compiler made of `acc += w * h` in head_fwd_kernel when the goldens pinned these bits: the vectoriser packs the
// last products, v_pk_mul_f32 + v_add_f32.)  head_fwd_body, SkillPredHead and head_loss_body<LossSpec> call this function, so
// they agree by construction.  The unfused tail -- the part an optimiser decided differently from one body to the next -- is
// written out with contraction off.  The fused part is `acc += w * h` with contraction on, NOT __builtin_fmaf: the builtin
// gives the same instructions in another schedule, which costs head_skill_accum_kernel a wave per SIMD at every CHV and
// head_fwd_kernel up to 14 VGPRs, while this form compiles head_fwd_kernel to the instruction stream it had.  The fused
// pass of LossPlain and LossMap still holds the plain loop (Elem::HEAD_DOT = false): either form of this function costs its
// bf16 CHV = 32 instances -- the default step's -- a wave per SIMD (96 -> 108 VGPRs).  profiles/EXPERIMENTS.md has the
// numbers.  So the SOURCE enforces the unfused tail only, and only where this function is called; the fused part here, and the
// whole chain in that loop, are what the optimiser forms, held to the definition by the fused-vs-launches and skill bit tests,
// whose tables have data in the last 12 staged channels (Ch > CHV - 12) at every CHV in f32 and bf16 (the "tail" cases of
// tests/test_gpu_small_branches.py FUSED_CASES and the Ch = CHV cases beside them).
#define HEAD_DOT_UNFUSED_TAIL 12
template <int CHV>
__device__ __forceinline__ float head_dot(float acc, const float* w_row, const float (&hv)[CHV]) {
  const f32x4_t* wr = (const f32x4_t*)w_row;
#pragma unroll
  for (int c = 0; c < CHV - HEAD_DOT_UNFUSED_TAIL; c += 4) {
#pragma clang fp contract(fast)
    const f32x4_t wv = wr[c / 4];
    acc += wv[0] * hv[c]; acc += wv[1] * hv[c + 1]; acc += wv[2] * hv[c + 2]; acc += wv[3] * hv[c + 3];
  }
#pragma unroll
  for (int c = CHV - HEAD_DOT_UNFUSED_TAIL; c < CHV; c += 4) {
#pragma clang fp contract(off)
    const f32x4_t wv = wr[c / 4];
    const float m0 = wv[0] * hv[c], m1 = wv[1] * hv[c + 1], m2 = wv[2] * hv[c + 2], m3 = wv[3] * hv[c + 3];
    acc = m0 + acc; acc = m1 + acc; acc = m2 + acc; acc = m3 + acc;
  }
  return acc;
}

// CHV of a padded channel count (<= 128), and the host's pick of that instance: f(std::integral_constant<int, CHV>)
static inline int head_chv(int Chp) { return Chp <= 32 ? 32 : (Chp <= 64 ? 64 : 128); }
template <class F> static inline auto head_by_chv(int Chp, F&& f) {
  if (Chp <= 32) return f(std::integral_constant<int, 32>{});
  if (Chp <= 64) return f(std::integral_constant<int, 64>{});
  return f(std::integral_constant<int, 128>{});
}
// The ONE limit of the staged head arithmetic, for every entry that runs it: at most 128 padded channels in 4-channel vectors,
// and the weight image [O][CHV] plus what the fused passes keep beside it -- one chunk of HEAD_OCH outputs' d loss / d pred of
// 64 pixels, 8 KiB of static LDS -- within the 160 KiB of a CU.  nint_head_fwd[_seq] and the dh pass of nint_head_bwd[_seq]
// keep nothing beside the weights, but take the same rule: wherever a fused pass runs, its separate launches run the SAME
// bodies and give the same bits (the trainer and the skill path switch between the two silently).  Beyond it: the wide kernels.
#define HEAD_OCH 64
static inline size_t head_loss_lds(int Chp, int O) {                  // the dynamic LDS of the fused head + loss pass
  return ((size_t)O * head_chv(Chp) + (size_t)(O < HEAD_OCH ? O : HEAD_OCH) * 64) * sizeof(float);
}
static inline bool head_staged_holds(int Chp, int O) {
  if (Chp > 128 || Chp % 4 != 0) return false;
  return head_loss_lds(Chp, O) + 8192 <= 160 * 1024;
}

// The sequence entries (nint_head_fwd_seq and its kin) run the same bodies over all T*B images of the top layer's slab; only the
// plane index of the (B, T*O, H, W) tensors differs: image n = t*B + b (time-major, as everywhere inside the library) owns the
// O planes from (b*T + t)*O.  SEQ = false: plane block n, the (N, O, H, W) tensors of the one-step entries, whose kernel
// instances receive the sequence arguments (Bs, dlast, T) without reading them.
template <bool SEQ>
__device__ __forceinline__ size_t head_image(size_t n, int Bs, int T) {
  if constexpr (SEQ) return (n % (size_t)Bs) * T + n / (size_t)Bs;
  else return n;
}

// RESIDUAL HEAD (nint_head_base, nint.h): p = fl32(d + base), d the staged dot product above and base the value
// STORED in the input slab xs at the pixel's feedback channel c0 + o (a folded slab: the pixel's own copy, slab channel
// (k/2)*Cx + c0 + o), converted to f32 exactly.  One rounded add behind the dot product: the base never enters the accumulator.
// The bodies below take the operand as a trailing pack `Base...` that is empty (the kernel as it was: same arguments, same
// instruction stream) or one HeadBaseK; the loss body finds it in its element (LossSpecRes).  The base of a pixel is read where
// the pixel's h record is: interior pixels only, the O channels from `c`, nothing else of xs.
struct HeadBaseK { const void* xs; int n0, Cxp, c; };     // image n0 of xs pairs with the body's first image; c: first slab channel read
__device__ __forceinline__ size_t head_base_at(const HeadBaseK& k, size_t n, int y, int x, int P, int Hh, int Wh) {
  return ((((size_t)k.n0 + n) * Hh + (y + P)) * Wh + (x + P)) * k.Cxp + k.c;
}
__device__ __forceinline__ float head_add_base(float d, float base) {
#pragma clang fp contract(off)
  return d + base;
}

template <int DT, int CHV, bool SEQ, class... Base>
__device__ __forceinline__ void head_fwd_body(float* w_s, const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                              const float* __restrict__ w, const float* __restrict__ b,
                                              float* __restrict__ pred, int H, int W, int P, int Hh, int Wh, int Bs, const Base... base) {
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
  if constexpr (sizeof...(Base) > 0) {
    const HeadBaseK k = (base, ...);
    const size_t xb = head_base_at(k, (size_t)n, y, x, P, Hh, Wh);
    for (int o = 0; o < O; ++o)
      out[(size_t)o * H * W] = head_add_base(head_dot<CHV>(b ? b[o] : 0.f, w_s + o * CHV, hv), load_elem<DT>(k.xs, xb + o));
  } else {
    for (int o = 0; o < O; ++o) out[(size_t)o * H * W] = head_dot<CHV>(b ? b[o] : 0.f, w_s + o * CHV, hv);
  }
}

template <int DT, int CHV, bool SEQ, class... Base>
__global__ __launch_bounds__(256) void head_fwd_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ pred, int H, int W, int P, int Hh, int Wh, int Bs,
                                                       const Base... base) {
  extern __shared__ __attribute__((aligned(16))) char smem_hf[];
  head_fwd_body<DT, CHV, SEQ>((float*)smem_hf, h, n0, N, Ch, Chp, O, w, b, pred, H, W, P, Hh, Wh, Bs, base...);
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

template <int DT, bool SEQ>
__global__ void head_fwd_wide_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                     const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ pred,
                                     int H, int W, int P, int Hh, int Wh, int Bs) {
  head_fwd_wide_body<DT, SEQ>(h, n0, N, Ch, Chp, O, w, b, pred, H, W, P, Hh, Wh, Bs);
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
// the functor of a backward kernel instance, built inside the kernel from its __restrict__ pointer arguments
template <bool SEQ>
__device__ __forceinline__ auto head_dp(const float* __restrict__ dpred, const float* __restrict__ dlast, int O, int Bs, int T, size_t HW) {
  if constexpr (SEQ) return DpSeq{dpred, dlast, O, Bs, T, HW};
  else return DpPlain{dpred, O, HW};
}

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

template <int DT, int CHV, bool SEQ>
__global__ __launch_bounds__(256) void head_bwd_dh_kernel(const float* __restrict__ w, const float* __restrict__ dpred,
                                                          const float* __restrict__ dlast, int Bs, int T,
                                                          void* __restrict__ dh, int N, int Ch, int Chp, int O, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) char smem_hd[];
  head_bwd_dh_body<DT, CHV>((float*)smem_hd, w, head_dp<SEQ>(dpred, dlast, O, Bs, T, (size_t)H * W), dh, N, Ch, Chp, O, H, W);
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

template <int DT, bool SEQ>
__global__ void head_bwd_dh_wide_kernel(const float* __restrict__ w, const float* __restrict__ dpred,
                                        const float* __restrict__ dlast, int Bs, int T, void* __restrict__ dh,
                                        int N, int Ch, int Chp, int O, int H, int W) {
  head_bwd_dh_wide_body<DT>(w, head_dp<SEQ>(dpred, dlast, O, Bs, T, (size_t)H * W), dh, N, Ch, Chp, O, H, W);
}

// dw[o][c] = sum_pixels dpred*h ; db[o] = sum dpred.  One workgroup per (o, c-or-bias) output,
// fixed-order tree reduction -> bitwise reproducible.
template <int DT, class Dp>
__device__ __forceinline__ void head_bwd_dw_body(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                 int O, const Dp dpred,
                                                 float* __restrict__ dw, float* __restrict__ db, int H, int W,
                                                 int P, int Hh, int Wh, int acc_out) {
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
    float* dst = c < Ch ? dw + o * Ch + c : db + o;
    *dst = acc_out ? *dst + red[0] : red[0];      // (nint_head_bwd_acc: stored, or added by the output's only writer)
  }
}

template <int DT, bool SEQ>
__global__ __launch_bounds__(256) void head_bwd_dw_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                          int O, const float* __restrict__ dpred,
                                                          const float* __restrict__ dlast, int Bs, int T,
                                                          float* __restrict__ dw, float* __restrict__ db, int H, int W,
                                                          int P, int Hh, int Wh, int acc_out) {
  head_bwd_dw_body<DT>(h, n0, N, Ch, Chp, O, head_dp<SEQ>(dpred, dlast, O, Bs, T, (size_t)H * W), dw, db, H, W, P, Hh, Wh, acc_out);
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

template <int DT, bool SEQ>
__global__ __launch_bounds__(512) void head_bwd_dw_tiled_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                              int O, const float* __restrict__ dpred,
                                                              const float* __restrict__ dlast, int Bs, int T,
                                                              float* __restrict__ partial, int H, int W, int P, int Hh,
                                                              int Wh, int stage) {
  extern __shared__ __attribute__((aligned(16))) float smem_dw[];
  head_bwd_dw_tiled_body<DT>(smem_dw, h, n0, N, Ch, Chp, O, head_dp<SEQ>(dpred, dlast, O, Bs, T, (size_t)H * W), partial, H, W, P, Hh, Wh, stage);
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

template <int DT, bool SEQ>
__global__ __launch_bounds__(512) void head_bwd_dw_rtile_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp,
                                                              int O, const float* __restrict__ dpred,
                                                              const float* __restrict__ dlast, int Bs, int T,
                                                              float* __restrict__ partial, int H, int W, int P, int Hh,
                                                              int Wh, int stage) {
  extern __shared__ __attribute__((aligned(16))) float smem_dw[];
  head_bwd_dw_rtile_body<DT>(smem_dw, h, n0, N, Ch, Chp, O, head_dp<SEQ>(dpred, dlast, O, Bs, T, (size_t)H * W), partial, H, W, P, Hh, Wh, stage);
}

// block = 64 outputs x blockDim/64 lanes over the per-workgroup partials; fixed order
__global__ void head_bwd_dw_final_kernel(const float* __restrict__ partial, int nblocks, int Ch, int O,
                                         float* __restrict__ dw, float* __restrict__ db, int acc_out) {
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
  float* dst = c < Ch ? dw + o * Ch + c : db + o;
  *dst = acc_out ? *dst + s : s;                  // (nint_head_bwd_acc: stored, or added by the output's only writer)
}

// The base operand of the _res entries (nint_head_base, nint.h), checked behind the twin's own checks: NINT_OK with *k filled and
// *on = whether there is a base at all (a NULL structure or a NULL xs: the twin entry).  NINT_E_ARG: a negative x_n0, Cx < 1, the
// O feedback channels [c0, c0 + O) outside [0, Cx), xfold_k negative or even, Cxp below the (folded) channel count, or a pixel of
// Cxp elements that is no multiple of 16 bytes; NINT_E_ALIGN: xs not 16-byte aligned.
static int head_base_check(const nint_head_base* hb, int O, int dtype, HeadBaseK* k, bool* on) {
  *on = hb && hb->xs;
  if (!*on) return NINT_OK;
  const int es = dtype == NINT_BF16 ? 2 : 4;
  if (hb->x_n0 < 0 || hb->Cx <= 0 || hb->c0 < 0 || (long long)hb->c0 + O > hb->Cx) return NINT_E_ARG;
  if (hb->xfold_k < 0 || (hb->xfold_k > 0 && !(hb->xfold_k & 1))) return NINT_E_ARG;
  const int kf = hb->xfold_k > 1 ? hb->xfold_k : 1;
  if ((long long)hb->Cxp < (long long)kf * hb->Cx || ((long long)hb->Cxp * es) % 16 != 0) return NINT_E_ARG;
  if ((((uintptr_t)hb->xs) & 15) != 0) return NINT_E_ALIGN;
  *k = HeadBaseK{hb->xs, hb->x_n0, hb->Cxp, (kf >> 1) * hb->Cx + hb->c0};
  return NINT_OK;
}

// SEQ: the sequence entry (n0 = Bs = B, N = T*B, plane blocks b*T + t).  hb: the residual head's base (nullptr: none); the generic
// wide kernels have no residual form: NINT_E_SHAPE beyond the staged rule.
template <bool SEQ>
static int head_fwd_impl(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b, float* pred,
                         const nint_geom* g, int dtype, int Bs, void* stream, const HeadBaseK* hb = nullptr) {
  const size_t total = (size_t)N * O * g->H * g->W, npix = (size_t)N * g->H * g->W;
  hipStream_t st = (hipStream_t)stream;
  const dim3 gp((unsigned)((npix + 255) / 256));
  const size_t w_lds = (size_t)O * head_chv(Chp) * sizeof(float);      // staged weights [O][CHV]
  const int rc = nint_by_dtype(dtype, [&](auto dt) -> int {
    constexpr int DT = decltype(dt)::value;
    if (head_staged_holds(Chp, O))
      return head_by_chv(Chp, [&](auto chv) -> int {
        if (hb) {
          auto kern = head_fwd_kernel<DT, decltype(chv)::value, SEQ, HeadBaseK>;
          if (w_lds > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w_lds));
          hipLaunchKernelGGL(kern, gp, dim3(256), w_lds, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh, Bs, *hb);
          return NINT_OK;
        }
        auto kern = head_fwd_kernel<DT, decltype(chv)::value, SEQ>;
        if (w_lds > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w_lds));
        hipLaunchKernelGGL(kern, gp, dim3(256), w_lds, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh, Bs);
        return NINT_OK;
      });
    if (hb) return NINT_E_SHAPE;
    hipLaunchKernelGGL((head_fwd_wide_kernel<DT, SEQ>), grid1d(total), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, w, b, pred, g->H, g->W, g->P, g->Hh, g->Wh, Bs);
    return NINT_OK;
  });
  if (rc != NINT_OK) return rc;
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_head_fwd_res(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                 float* pred, const nint_geom* g, int dtype, const nint_head_base* base, void* stream) {
  if (!h_slab || !w || !pred || !g || N <= 0 || O <= 0 || Ch <= 0) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  HeadBaseK k; bool on;
  const int rc = head_base_check(base, O, dtype, &k, &on);
  if (rc != NINT_OK) return rc;
  return head_fwd_impl<false>(h_slab, n0, N, Ch, Chp, O, w, b, pred, g, dtype, 0, stream, on ? &k : nullptr);
}

extern "C" int nint_head_fwd(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                             const float* b, float* pred, const nint_geom* g, int dtype, void* stream) {
  return nint_head_fwd_res(h_slab, n0, N, Ch, Chp, O, w, b, pred, g, dtype, nullptr, stream);
}

// channel padding of a slab the head reads: KC of the storage type (nint.h), so every 16-byte channel vector stays inside
static bool head_seq_args_ok(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const nint_geom* g, int dtype) {
  if (!h_slab || !w || !g || B <= 0 || T <= 0 || O <= 0 || Ch <= 0 || Chp < Ch) return false;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return false;
  if (g->H <= 0 || g->W <= 0 || g->P < 0 || g->Hh < g->H + 2 * g->P || g->Wh < g->W + 2 * g->P) return false;
  return Chp % (dtype == NINT_BF16 ? 32 : 16) == 0;
}

extern "C" int nint_head_fwd_seq_res(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                     float* seq, const nint_geom* g, int dtype, const nint_head_base* base, void* stream) {
  if (!seq || !head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if ((((uintptr_t)h_slab) & 15) != 0) return NINT_E_ALIGN;
  HeadBaseK k; bool on;
  const int rc = head_base_check(base, O, dtype, &k, &on);
  if (rc != NINT_OK) return rc;
  return head_fwd_impl<true>(h_slab, B, T * B, Ch, Chp, O, w, b, seq, g, dtype, B, stream, on ? &k : nullptr);     // h_t = slot t + 1: images from B
}

extern "C" int nint_head_fwd_seq(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                 float* seq, const nint_geom* g, int dtype, void* stream) {
  return nint_head_fwd_seq_res(h_slab, B, T, Ch, Chp, O, w, b, seq, g, dtype, nullptr, stream);
}

// ------------------------------------------------------------------------------ feedback (closed-loop forward)
// nint_seq.fb_O / nint_head_feedback (nint.h): the head of N images of the top layer's slab, rounded once to ET,
// into the feedback channels [c0, c0 + O) of N images of the input slab.  One workgroup per image row.
//   (1) one thread per pixel of the row forms the O dot products with the pieces head_fwd_body is made of -- head_stage_weights,
//       the same channel loads, head_dot from the bias -- so the f32 value is nint_head_fwd's bit for bit; it is rounded to ET
//       and kept in LDS, p_s[x][o].
//   (2) every destination pixel gathers its own: thread items are (pixel, dword of the pixel's fed span), consecutive lanes on
//       consecutive dwords.  Plain slab (kf = 1): the span is the O channels from c0.  Folded slab (kf = k): slab channel
//       kx*Cx + c of pixel x is channel c of pixel x + kx - k/2 (0 outside the row; cyc: mod W), so the span runs over all k
//       copies and a dword's elements are stored only where their channel is a fed one -- a whole dword where both are
//       (bf16), else the one element.  Nothing else of xs is written: no halo pixel, no slack column, no other channel.
// SEL (scheduled sampling): the workgroup of an image whose bit of a.mask is clear returns before it touches
// anything -- a wave-uniform scalar test on a kernel argument; every byte of that image stays the caller's.  The unmasked
// instantiation is the kernel it was: it has no such test and never reads the word.
// RES (residual head): the thread that forms a pixel's dot products also reads the pixel's base -- the O stored
// values from channel (kf/2)*Cx + c0 of the same pixel of image a.xb + n, the step before -- in the pass that loads h, and adds
// each to its dot product (head_add_base) before the rounding.  The launch writes images from a.xs on and reads images from a.xb
// on: the plan keeps the two ranges apart.  The instantiation without it never reads the pointer.
// NZ (noise on the fed-back value): the same thread adds __fmul_rn(sigma[o], z) to the f32 value -- after the base --
// before the rounding: two f32 operations, never one FMA.  z is nint_input_noise's normal of (pixel y*W + x, o, a.nz_step,
// a.nz_lane0 + image): one Philox block (noise_quad, nint_common.h) per four outputs.  A channel with sigma[o] == 0 is left as the
// launch without NZ forms it.  What is staged in p_s is the stored value, so a folded slab's copies and a cyclic wrap gather one
// number per source pixel, as before.  The instantiations without it take the plan without the fields (FbPlan, as ever).
template <int DT, int CHV, bool SEL = false, bool RES = false, bool NZ = false>
__global__ __launch_bounds__(256) void head_feedback_kernel(const void* __restrict__ h, const float* __restrict__ w,
                                                            const float* __restrict__ b, void* __restrict__ xs,
                                                            std::conditional_t<NZ, FbPlanNz, FbPlan> a) {
  // (the pointers as __restrict__ arguments of their own, as head_fwd_kernel has them; a is the rest of the plan)
  if constexpr (SEL) {
    if (!((a.mask >> (blockIdx.x / a.H)) & 1ull)) return;
  }
  extern __shared__ __attribute__((aligned(16))) char smem_fb[];
  constexpr int ES = Elem<DT>::ES, EPD = 4 / ES;               // elements per dword
  float* __restrict__ w_s = (float*)smem_fb;                   // [O][CHV]
  float* __restrict__ p_s = w_s + a.O * CHV;                   // [W][O]
  head_stage_weights<CHV>(w_s, w, a.O, a.Ch);
  const int y = blockIdx.x % a.H, n = blockIdx.x / a.H;
  const size_t row = ((size_t)n * a.Hh + (y + a.P)) * a.Wh + a.P;          // first interior pixel of the row, in both slabs
  for (int x = threadIdx.x; x < a.W; x += 256) {
    const size_t hb = (row + x) * a.Chp;
    float hv[CHV];
#pragma unroll
    for (int c = 0; c < CHV; c += 4) {
      const f32x4_t v = (c < a.Chp) ? load_vec4<DT>(h, hb + c) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
      hv[c] = v[0]; hv[c + 1] = v[1]; hv[c + 2] = v[2]; hv[c + 3] = v[3];
    }
    f32x4_t z = {0.f, 0.f, 0.f, 0.f};
    for (int o = 0; o < a.O; ++o) {
      float p = head_dot<CHV>(b ? b[o] : 0.f, w_s + o * CHV, hv);
      if constexpr (RES) p = head_add_base(p, load_elem<DT>(a.xb, (row + x) * a.Cxp + (size_t)((a.kf >> 1) * a.Cx + a.c0 + o)));
      if constexpr (NZ) {
        if ((o & 3) == 0) z = noise_quad((uint32_t)(y * a.W + x), (uint32_t)(o >> 2), a.nz_step, a.nz_lane0 + (uint32_t)n, a.nz_seed, a.nz_draw);
        const float sg = a.nz_sigma[o];
        if (sg != 0.f) {
          // (the rule's __fmul_rn and __fadd_rn: HIP defines both as the plain operators, which the compiler contracts into one FMA
          // wherever it may -- so they are written as operators under contraction off)
#pragma clang fp contract(off)
          const float add = sg * z[o & 3];
          p = p + add;
        }
      }
      p_s[x * a.O + o] = DT == NINT_BF16 ? bf2f(f2bf(p)) : p;
    }
  }
  __syncthreads();
  const int first = a.c0, last = (a.kf - 1) * a.Cx + a.c0 + a.O;          // the fed span of a pixel's channels
  const int d0 = first / EPD, nd = (last + EPD - 1) / EPD - d0;
  for (int i = threadIdx.x; i < a.W * nd; i += 256) {
    const int x = i / nd, d = d0 + (i - x * nd);
    float v[EPD]; bool on[EPD];
#pragma unroll
    for (int e = 0; e < EPD; ++e) {
      const int ch = d * EPD + e, kx = ch / a.Cx, c = ch - kx * a.Cx;
      on[e] = kx < a.kf && c >= a.c0 && c < a.c0 + a.O;
      int xi = x + kx - (a.kf >> 1);
      if (a.cyc) xi = xi < 0 ? xi + a.W : (xi >= a.W ? xi - a.W : xi);
      v[e] = (on[e] && xi >= 0 && xi < a.W) ? p_s[xi * a.O + (c - a.c0)] : 0.f;
    }
    char* px = (char*)xs + (row + x) * (size_t)a.Cxp * ES;
    if constexpr (DT == NINT_BF16) {
      if (on[0] && on[1]) *(uint32_t*)(px + 4 * (size_t)d) = pack_bf16x2(v[0], v[1]);
      else if (on[0]) *(uint16_t*)(px + 4 * (size_t)d) = f2bf(v[0]);
      else if (on[1]) *(uint16_t*)(px + 4 * (size_t)d + 2) = f2bf(v[1]);
    } else {
      if (on[0]) *(float*)(px + 4 * (size_t)d) = v[0];
    }
  }
}

// what nint_head_feedback and its adjoint check of the numbers they share, in this order: NINT_E_ARG, then (aligned: the caller's
// pointers) NINT_E_ALIGN, then NINT_E_SHAPE -- the staged head with a row of predictions beside the weights, for both.  (The
// W * O term is the FORWARD kernel's LDS; the backward launch stages the weights alone and takes the rule only so that it
// holds exactly the forward's shapes: its own LDS is FbBwdPlan.lds.)
static int feedback_check(int N, int Ch, int Chp, int O, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g,
                          int dtype, bool aligned) {
  if (!g || N <= 0 || O <= 0 || Ch <= 0 || Cx <= 0) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  const int es = dtype == NINT_BF16 ? 2 : 4;
  if (g->H <= 0 || g->W <= 0 || g->P < 0 || g->Hh < g->H + 2 * g->P || g->Wh < g->W + 2 * g->P) return NINT_E_ARG;
  if (Chp < Ch || Chp % (dtype == NINT_BF16 ? 32 : 16) != 0) return NINT_E_ARG;
  if (c0 < 0 || c0 + O > Cx) return NINT_E_ARG;
  if (xfold_k < 0 || (xfold_k > 0 && !(xfold_k & 1))) return NINT_E_ARG;
  const int kf = xfold_k > 1 ? xfold_k : 1;
  if (Cxp < kf * Cx || (Cxp * es) % 16 != 0) return NINT_E_ARG;
  if (lon_cyclic != 0 && lon_cyclic != 1) return NINT_E_ARG;
  if (lon_cyclic && (g->W < g->P || g->W < kf / 2)) return NINT_E_ARG;
  if (!aligned) return NINT_E_ALIGN;
  if (!head_staged_holds(Chp, O)) return NINT_E_SHAPE;
  if (((size_t)O * head_chv(Chp) + (size_t)g->W * O) * sizeof(float) > 160 * 1024) return NINT_E_SHAPE;
  return NINT_OK;
}

int nint_internal_feedback_plan(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g,
                                int dtype, FbPlan* plan) {
  if (!h_slab || !w || !xs_slab || !plan || n0 < 0 || x_n0 < 0) return NINT_E_ARG;
  const int rc = feedback_check(N, Ch, Chp, O, Cx, Cxp, c0, xfold_k, lon_cyclic, g, dtype,
                                ((((uintptr_t)h_slab) | ((uintptr_t)xs_slab)) & 15) == 0);
  if (rc != NINT_OK) return rc;
  const int es = dtype == NINT_BF16 ? 2 : 4, kf = xfold_k > 1 ? xfold_k : 1;
  const size_t lds = ((size_t)O * head_chv(Chp) + (size_t)g->W * O) * sizeof(float);
  const size_t halo_px = (size_t)g->Hh * g->Wh;
  FbPlan p = {};
  p.h = (const char*)h_slab + (size_t)n0 * halo_px * Chp * es; p.w = w; p.b = b;
  p.xs = (char*)xs_slab + (size_t)x_n0 * halo_px * Cxp * es;
  p.N = N; p.Ch = Ch; p.Chp = Chp; p.O = O; p.Cx = Cx; p.Cxp = Cxp; p.c0 = c0; p.kf = kf; p.cyc = lon_cyclic; p.dtype = dtype;
  p.H = g->H; p.W = g->W; p.P = g->P; p.Hh = g->Hh; p.Wh = g->Wh; p.lds = lds;
  *plan = p;
  return NINT_OK;
}

int nint_internal_feedback_enqueue(const FbPlanNz* p, void* stream) {
  const int rc = nint_by_dtype(p->dtype, [&](auto dt) -> int {
    return head_by_chv(p->Chp, [&](auto chv) -> int {
      constexpr int DT = decltype(dt)::value, CHV = decltype(chv)::value;
      const dim3 grid((unsigned)((size_t)p->N * p->H));
      if (p->nz) {                                 // (the instantiations with the noise take the whole plan, the others the FbPlan in it)
        auto kern = p->res ? (p->sel ? head_feedback_kernel<DT, CHV, true, true, true> : head_feedback_kernel<DT, CHV, false, true, true>)
                           : (p->sel ? head_feedback_kernel<DT, CHV, true, false, true> : head_feedback_kernel<DT, CHV, false, false, true>);
        if (p->lds > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds));
        hipLaunchKernelGGL(kern, grid, dim3(256), p->lds, (hipStream_t)stream, p->h, p->w, p->b, p->xs, *p);
        return NINT_OK;
      }
      auto kern = p->res ? (p->sel ? head_feedback_kernel<DT, CHV, true, true> : head_feedback_kernel<DT, CHV, false, true>)
                         : (p->sel ? head_feedback_kernel<DT, CHV, true, false> : head_feedback_kernel<DT, CHV, false, false>);
      if (p->lds > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds));
      hipLaunchKernelGGL(kern, grid, dim3(256), p->lds, (hipStream_t)stream, p->h, p->w, p->b, p->xs, (const FbPlan&)*p);
      return NINT_OK;
    });
  });
  if (rc != NINT_OK) return rc;
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_head_feedback(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                  void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic,
                                  const nint_geom* g, int dtype, void* stream) {
  FbPlanNz p = {};
  const int rc = nint_internal_feedback_plan(h_slab, n0, N, Ch, Chp, O, w, b, xs_slab, x_n0, Cx, Cxp, c0, xfold_k, lon_cyclic, g, dtype, &p);
  return rc != NINT_OK ? rc : nint_internal_feedback_enqueue(&p, stream);
}

// ... for the images of `fed` (HOST bytes, one per image, 0 or 1; N <= 64) alone: nint_head_feedback's checks in its order,
// then the mask's (nint_internal_mask_word)
extern "C" int nint_head_feedback_sel(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                      void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic,
                                      const uint8_t* fed, const nint_geom* g, int dtype, void* stream) {
  FbPlanNz p = {};
  int rc = nint_internal_feedback_plan(h_slab, n0, N, Ch, Chp, O, w, b, xs_slab, x_n0, Cx, Cxp, c0, xfold_k, lon_cyclic, g, dtype, &p);
  if (rc == NINT_OK) rc = nint_internal_mask_word(fed, N, &p.mask);
  if (rc != NINT_OK) return rc;
  p.sel = 1;
  return p.mask ? nint_internal_feedback_enqueue(&p, stream) : (int)NINT_OK;       // (no image fed: nothing to launch)
}

// The base of a residual feedback launch (FbPlan.xb / .res): images [base_n0, base_n0 + N) of the slab the launch writes images
// [x_n0, x_n0 + N) of -- the two ranges apart, else NINT_E_ARG.  Called behind nint_internal_feedback_plan, whose checks cover the slab.
int nint_internal_feedback_base(FbPlan* p, const void* xs_slab, int x_n0, int base_n0, int N) {
  if (base_n0 < 0 || (base_n0 < x_n0 + N && x_n0 < base_n0 + N)) return NINT_E_ARG;
  const size_t es = p->dtype == NINT_BF16 ? 2 : 4;
  p->xb = (const char*)xs_slab + (size_t)base_n0 * p->Hh * p->Wh * p->Cxp * es;
  p->res = 1;
  return NINT_OK;
}

// ... with the residual head's base: p = dot + the value stored in the feedback channels of image base_n0 + i,
// rounded and stored into image x_n0 + i.  base_n0 < 0: no base; fed == NULL: every image -- with both, nint_head_feedback.
extern "C" int nint_head_feedback_res(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                      void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, int base_n0,
                                      const uint8_t* fed, const nint_geom* g, int dtype, void* stream) {
  return nint_head_feedback_noise(h_slab, n0, N, Ch, Chp, O, w, b, xs_slab, x_n0, Cx, Cxp, c0, xfold_k, lon_cyclic, base_n0, fed, g, dtype,
                                  stream, nullptr, 0);
}

// The noise of a feedback launch (FbPlanNz.nz*): called behind nint_internal_feedback_plan, which fills the FbPlan in it alone.  This
// function owns the noise's fields and sets every one of them: off (fn or its sigma NULL) is nz = 0, whatever the plan held.
int nint_internal_feedback_noise(FbPlanNz* p, const nint_feedback_noise* fn, uint32_t step) {
  p->nz_sigma = nullptr; p->nz_seed = p->nz_draw = p->nz_step = p->nz_lane0 = 0; p->nz = 0;
  if (!fn || !fn->sigma) return NINT_OK;
  if ((((uintptr_t)fn->sigma) & 3) != 0) return NINT_E_ALIGN;
  p->nz_sigma = fn->sigma; p->nz_seed = fn->seed; p->nz_draw = fn->draw; p->nz_step = step; p->nz_lane0 = fn->lane0;
  p->nz = 1;
  return NINT_OK;
}

// ... and with noise on the stored value: nint_head_feedback_res's checks in its order, then the noise's
extern "C" int nint_head_feedback_noise(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                        void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, int base_n0,
                                        const uint8_t* fed, const nint_geom* g, int dtype, void* stream,
                                        const nint_feedback_noise* fn, uint32_t step) {
  FbPlanNz p = {};
  int rc = nint_internal_feedback_plan(h_slab, n0, N, Ch, Chp, O, w, b, xs_slab, x_n0, Cx, Cxp, c0, xfold_k, lon_cyclic, g, dtype, &p);
  if (rc == NINT_OK && base_n0 >= 0) rc = nint_internal_feedback_base(&p, xs_slab, x_n0, base_n0, N);
  if (rc == NINT_OK && fed) { rc = nint_internal_mask_word(fed, N, &p.mask); p.sel = 1; }
  if (rc == NINT_OK) rc = nint_internal_feedback_noise(&p, fn, step);
  if (rc != NINT_OK) return rc;
  return !p.sel || p.mask ? nint_internal_feedback_enqueue(&p, stream) : (int)NINT_OK;
}

// ------------------------------------------------------------------------------ feedback, backward (roll-out training)
// nint_head_feedback_bwd (nint.h): the adjoint of the launch above for the N images of one fed step u.  It is
// nint_head_bwd's dh pass -- head_bwd_dh_body, one thread per pixel, the weights staged once per workgroup, the Chp record
// stored in whole vectors -- over a cotangent that is formed on the way: DpFed hands the body g = dpred + xi and stores it back,
// each element by the one thread that reads it.  xi, the d/dx of step u on the feedback channels, comes out of the compact
// dx block by element loads: the fed span starts at any channel c0 (37 of 40: across a 16-byte group), and every 64-byte
// line it touches is fetched once per pixel either way.  Plain slab: the pixel's own channel, as nint_unpack_compact reads it;
// folded slab: the k terms of nint_unfold_dx[_cyclic] in its order, from 0.f.
// SEL (scheduled sampling): an image whose bit of `mask` is clear was not fed -- xi is 0 without a read of dx,
// dpred is handed on as it stands and not stored, so the launch is nint_head_bwd's dh pass for that image.  The test is per
// thread: a 256-thread workgroup straddles image boundaries.
// RES (residual head): the base of step u is the fed value itself, so the total cotangent g_u of p_u comes back
// beside xi_u: g = fl32(fl32(dpred + xi) + dpn), dpn the same element of the dpred image of step u (final: the plan is time-major,
// descending), which this launch does not write.  An unfed image takes neither.
template <int DT, bool SEL = false, bool RES = false>
struct DpFed {
  const void* __restrict__ dx; float* dp; int O, W, Cx, Cxp, c0, kf, cyc; size_t HW; unsigned long long mask; const float* dpn;
  __device__ __forceinline__ float operator()(size_t n, int o, size_t yx) const {
    if constexpr (SEL) {
      if (!((mask >> n) & 1ull)) return dp[(n * O + o) * HW + yx];
    }
    const int x = (int)(yx % (size_t)W);
    const size_t row = n * HW + yx - x;                        // first pixel of the row in the compact block
    float xi;
    if (kf == 1) xi = load_elem<DT>(dx, (row + x) * Cxp + c0 + o);
    else {
      xi = 0.f;
      for (int kx = 0; kx < kf; ++kx) {
        int xs = x - kx + kf / 2;
        if (cyc) xs = xs < 0 ? xs + W : (xs >= W ? xs - W : xs);
        if (xs >= 0 && xs < W) xi += load_elem<DT>(dx, (row + xs) * Cxp + kx * Cx + c0 + o);
      }
    }
    float* p = dp + (n * O + o) * HW + yx;
    float g = *p + xi;
    if constexpr (RES) g = g + dpn[(n * O + o) * HW + yx];
    *p = g;
    return g;
  }
};

template <int DT, int CHV, bool SEL = false, bool RES = false>
__global__ __launch_bounds__(256) void head_feedback_bwd_kernel(const void* __restrict__ dx, float* dpred, const float* __restrict__ w,
                                                                void* __restrict__ dh, FbBwdPlan a) {
  extern __shared__ __attribute__((aligned(16))) char smem_fbb[];
  const DpFed<DT, SEL, RES> dp{dx, dpred, a.O, a.W, a.Cx, a.Cxp, a.c0, a.kf, a.cyc, (size_t)a.H * a.W, a.mask, RES ? a.pnext : nullptr};
  head_bwd_dh_body<DT, CHV>((float*)smem_fbb, w, dp, dh, a.N, a.Ch, a.Chp, a.O, a.H, a.W);
}

int nint_internal_feedback_bwd_plan(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch, int Chp,
                                    int O, const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g,
                                    int dtype, FbBwdPlan* plan) {
  if (!dx || !dpred || !dh || !w || !plan || dx_n0 < 0 || p_n0 < 0 || dh_n0 < 0) return NINT_E_ARG;
  const int rc = feedback_check(N, Ch, Chp, O, Cx, Cxp, c0, xfold_k, lon_cyclic, g, dtype,
                                ((((uintptr_t)dx) | ((uintptr_t)dh)) & 15) == 0 && (((uintptr_t)dpred) & 3) == 0);
  if (rc != NINT_OK) return rc;
  const size_t es = dtype == NINT_BF16 ? 2 : 4, comp_px = (size_t)g->H * g->W;
  FbBwdPlan p = {};
  p.dx = (const char*)dx + (size_t)dx_n0 * comp_px * Cxp * es; p.dpred = dpred + (size_t)p_n0 * O * comp_px;
  p.dh = (char*)dh + (size_t)dh_n0 * comp_px * Chp * es; p.w = w;
  p.N = N; p.Ch = Ch; p.Chp = Chp; p.O = O; p.Cx = Cx; p.Cxp = Cxp; p.c0 = c0; p.kf = xfold_k > 1 ? xfold_k : 1; p.cyc = lon_cyclic;
  p.dtype = dtype; p.H = g->H; p.W = g->W;
  p.lds = (size_t)O * head_chv(Chp) * sizeof(float);           // the staged weights [O][CHV], as in nint_head_bwd's dh pass
  *plan = p;
  return NINT_OK;
}

int nint_internal_feedback_bwd_enqueue(const FbBwdPlan* p, void* stream) {
  const size_t npix = (size_t)p->N * p->H * p->W;
  const int rc = nint_by_dtype(p->dtype, [&](auto dt) -> int {
    return head_by_chv(p->Chp, [&](auto chv) -> int {
      constexpr int DT = decltype(dt)::value, CHV = decltype(chv)::value;
      auto kern = p->res ? (p->sel ? head_feedback_bwd_kernel<DT, CHV, true, true> : head_feedback_bwd_kernel<DT, CHV, false, true>)
                         : (p->sel ? head_feedback_bwd_kernel<DT, CHV, true, false> : head_feedback_bwd_kernel<DT, CHV, false, false>);
      if (p->lds > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds));
      hipLaunchKernelGGL(kern, dim3((unsigned)((npix + 255) / 256)), dim3(256), p->lds, (hipStream_t)stream, p->dx, p->dpred, p->w, p->dh, *p);
      return NINT_OK;
    });
  });
  if (rc != NINT_OK) return rc;
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_head_feedback_bwd(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch, int Chp,
                                      int O, const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g,
                                      int dtype, void* stream) {
  FbBwdPlan p;
  const int rc = nint_internal_feedback_bwd_plan(dx, dx_n0, dpred, p_n0, dh, dh_n0, N, Ch, Chp, O, w, Cx, Cxp, c0, xfold_k, lon_cyclic,
                                                 g, dtype, &p);
  return rc != NINT_OK ? rc : nint_internal_feedback_bwd_enqueue(&p, stream);
}

// ... with xi taken for the images of `fed` alone (HOST bytes, one per image, 0 or 1; N <= 64): an unfed image keeps its dpred
// and gets dh = W^T dpred.  A mask of zeros is legal: the plain head backward (dh only) of the N images.
extern "C" int nint_head_feedback_bwd_sel(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch,
                                          int Chp, int O, const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic,
                                          const uint8_t* fed, const nint_geom* g, int dtype, void* stream) {
  FbBwdPlan p;
  int rc = nint_internal_feedback_bwd_plan(dx, dx_n0, dpred, p_n0, dh, dh_n0, N, Ch, Chp, O, w, Cx, Cxp, c0, xfold_k, lon_cyclic,
                                           g, dtype, &p);
  if (rc == NINT_OK) rc = nint_internal_mask_word(fed, N, &p.mask);
  if (rc != NINT_OK) return rc;
  p.sel = 1;
  return nint_internal_feedback_bwd_enqueue(&p, stream);
}

// ... with the residual head's skip term: g = (dpred + xi) + dpred image pnext_n0 + i on a fed image.
// pnext_n0 < 0: no such term; fed == NULL: every image -- with both, nint_head_feedback_bwd.  The images [pnext_n0, pnext_n0 + N)
// are only read: they must lie apart from [p_n0, p_n0 + N), else NINT_E_ARG.
extern "C" int nint_head_feedback_bwd_res(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch,
                                          int Chp, int O, const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic,
                                          int pnext_n0, const uint8_t* fed, const nint_geom* g, int dtype, void* stream) {
  FbBwdPlan p;
  int rc = nint_internal_feedback_bwd_plan(dx, dx_n0, dpred, p_n0, dh, dh_n0, N, Ch, Chp, O, w, Cx, Cxp, c0, xfold_k, lon_cyclic,
                                           g, dtype, &p);
  if (rc == NINT_OK && pnext_n0 >= 0) {
    if (pnext_n0 < p_n0 + N && p_n0 < pnext_n0 + N) rc = NINT_E_ARG;
    else { p.pnext = dpred + (size_t)pnext_n0 * O * g->H * g->W; p.res = 1; }
  }
  if (rc == NINT_OK && fed) { rc = nint_internal_mask_word(fed, N, &p.mask); p.sel = 1; }
  if (rc != NINT_OK) return rc;
  return nint_internal_feedback_bwd_enqueue(&p, stream);
}

// SEQ: d loss / d (head output) comes from the sequence tensors (DpSeq: dpred = dseq, dlast, Bs = B, T) instead of dpred alone
template <bool SEQ>
static int head_bwd_impl(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* dpred,
                         const float* dlast, int Bs, int T, void* dh, float* dw, float* db, int acc, const nint_geom* g, int dtype,
                         float* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t npix = (size_t)N * g->H * g->W;
  if (dh) {
    const dim3 gp((unsigned)((npix + 255) / 256));
    const size_t w_lds = (size_t)O * head_chv(Chp) * sizeof(float);    // staged weights [O][CHV]
    const int rc = nint_by_dtype(dtype, [&](auto dt) -> int {
      constexpr int DT = decltype(dt)::value;
      if (!head_staged_holds(Chp, O)) {
        hipLaunchKernelGGL((head_bwd_dh_wide_kernel<DT, SEQ>), grid1d(npix * Chp), dim3(256), 0, st, w, dpred, dlast, Bs, T, dh, N, Ch, Chp, O, g->H, g->W);
        return NINT_OK;
      }
      return head_by_chv(Chp, [&](auto chv) -> int {
        auto kern = head_bwd_dh_kernel<DT, decltype(chv)::value, SEQ>;
        if (w_lds > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w_lds));
        hipLaunchKernelGGL(kern, gp, dim3(256), w_lds, st, w, dpred, dlast, Bs, T, dh, N, Ch, Chp, O, g->H, g->W);
        return NINT_OK;
      });
    });
    if (rc != NINT_OK) return rc;
    NINT_LAUNCH_CHECK();
  }
  if (!dw || !db) return NINT_OK;
  const int nout = O * (Ch + 1);
  const int row_floats = (O | 1) + ((Ch + 1) | 1);
  const int Rd = O < Ch + 1 ? O : Ch + 1, Td = O < Ch + 1 ? Ch + 1 : O;      // register / thread dimension of the register-tiled kernel
  // the two-stage paths: per-workgroup partials in the caller's scratch (stage = pixels staged in LDS at a time), then the fold
  int stage = 0;
  size_t lds = 0;
  bool rtile = false;
  if (scratch && nout > 512 && Rd <= 32 && Td <= 512 && scratch_bytes >= (size_t)256 * nout * sizeof(float)) {
    const int SR = (Rd + 3) & ~3, ST = Td | 1, NH = 512 / Td < 8 ? 512 / Td : 8;
    stage = HEAD_DW_LDS_FLOATS / (SR + ST);
    if (stage > HEAD_DW_PIX) stage = HEAD_DW_PIX;
    size_t lds_f = (size_t)stage * (SR + ST);
    if ((size_t)NH * Td * SR > lds_f) lds_f = (size_t)NH * Td * SR;            // the closing fold's buffer
    lds = lds_f * sizeof(float);
    rtile = stage >= 8 && lds <= 64 * 1024;
  }
  const bool tiled = !rtile && scratch && nout <= HEAD_DW_NK * 512 && 8 * row_floats <= HEAD_DW_LDS_FLOATS &&
                     scratch_bytes >= (size_t)256 * nout * sizeof(float);
  if (tiled) {
    stage = HEAD_DW_LDS_FLOATS / row_floats;                   // pixels staged at a time (60 KiB of LDS)
    if (stage > HEAD_DW_PIX) stage = HEAD_DW_PIX;
    lds = (size_t)stage * row_floats * sizeof(float);
  }
  if (rtile || tiled) {
    const size_t cap = scratch_bytes / ((size_t)nout * sizeof(float));
    const size_t want = (npix + HEAD_DW_PIX - 1) / HEAD_DW_PIX;
    const int nblk = (int)(want < cap ? want : cap);
    nint_by_dtype(dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      auto kern = rtile ? head_bwd_dw_rtile_kernel<DT, SEQ> : head_bwd_dw_tiled_kernel<DT, SEQ>;
      hipLaunchKernelGGL(kern, dim3(nblk), dim3(512), lds, st, h_slab, n0, N, Ch, Chp, O, dpred, dlast, Bs, T, scratch, g->H, g->W, g->P, g->Hh, g->Wh, stage);
    });
    NINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_bwd_dw_final_kernel, dim3(nint_cdiv(nout, 64)), dim3(1024), 0, st, scratch, nblk, Ch, O, dw, db, acc);
  } else {
    nint_by_dtype(dtype, [&](auto dt) {
      hipLaunchKernelGGL((head_bwd_dw_kernel<decltype(dt)::value, SEQ>), dim3(O * (Ch + 1)), dim3(256), 0, st, h_slab, n0, N, Ch, Chp, O, dpred, dlast, Bs, T, dw, db, g->H, g->W, g->P, g->Hh, g->Wh, acc);
    });
  }
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_head_bwd_acc(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                                 const float* dpred, void* dh, float* dw, float* db, int accumulate, const nint_geom* g, int dtype,
                                 float* scratch, size_t scratch_bytes, void* stream) {
  if (!h_slab || !w || !dpred || !g || N <= 0 || O <= 0 || Ch <= 0) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  if (accumulate != 0 && accumulate != 1) return NINT_E_ARG;
  return head_bwd_impl<false>(h_slab, n0, N, Ch, Chp, O, w, dpred, nullptr, 0, 0, dh, dw, db, accumulate, g, dtype, scratch, scratch_bytes, stream);
}

extern "C" int nint_head_bwd(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                             const float* dpred, void* dh, float* dw, float* db, const nint_geom* g, int dtype,
                             float* scratch, size_t scratch_bytes, void* stream) {
  return nint_head_bwd_acc(h_slab, n0, N, Ch, Chp, O, w, dpred, dh, dw, db, 0, g, dtype, scratch, scratch_bytes, stream);
}

extern "C" int nint_head_bwd_seq_acc(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* dseq,
                                     const float* dpred_last, void* dh_seq, float* dw, float* db, int accumulate, const nint_geom* g,
                                     int dtype, float* scratch, size_t scratch_bytes, void* stream) {
  if (!head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if ((!dseq && !dpred_last) || (!dw) != (!db) || (!dh_seq && !dw)) return NINT_E_ARG;
  if (accumulate != 0 && accumulate != 1) return NINT_E_ARG;
  if (((((uintptr_t)h_slab) | ((uintptr_t)dh_seq)) & 15) != 0) return NINT_E_ALIGN;
  return head_bwd_impl<true>(h_slab, B, T * B, Ch, Chp, O, w, dseq, dpred_last, B, T, dh_seq, dw, db, accumulate, g, dtype, scratch, scratch_bytes, stream);
}

extern "C" int nint_head_bwd_seq(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* dseq,
                                 const float* dpred_last, void* dh_seq, float* dw, float* db, const nint_geom* g, int dtype,
                                 float* scratch, size_t scratch_bytes, void* stream) {
  return nint_head_bwd_seq_acc(h_slab, B, T, Ch, Chp, O, w, dseq, dpred_last, dh_seq, dw, db, 0, g, dtype, scratch, scratch_bytes, stream);
}

// ------------------------------------------------------------------------------ loss
// train.py:102,105: crop, MSELoss + L1Loss (mean), and its configurable form (nint_loss_spec; nint.h has the arithmetic of
// all three).  Two launches on the same stream: (1) per-workgroup partial sums in double (fixed order), (2) one workgroup
// folds them, writes the loss and adds to the running statistics.  Either alone (loss_partial_kernel: pred from memory) or
// fused with the head (head_loss_kernel below).  What differs between the entries is the LOSS ELEMENT, a compile-time policy:
//   LossPlain  the reference's loss: term d^2 + |d|, dpred = (2 d + sgn d) / n on the crop, n = N * O * Hc * Wc.
//   LossMap    the _weighted entries: every term of a crop cell carries the cell's weight wgt[cy][cx] as a double factor, n
//              becomes cnt = N * O * sum(wgt).  With wgt = 1 it gives LossPlain's bits.
//   LossSpec   term a d^2 + b |d| + c H(d) with coefficients known at run time; the weight is the product of the cell's
//              (optional map) and the output's (optional ow; per (step, output) in the sequence entry).  A zero coefficient
//              takes its term out (flags, not products: 0 * inf is NaN).  Spec (1, 1, 0) gives the bits of the other two.
// A policy is built inside the kernel from the kernel's arguments (wgt, cnt[, LossSpecK]) and supplies
//   NS, Sums, add     the running sums of a thread (sum-of-squares, sum |d|, sum y, sum y^2[, sum H]) and one element's terms
//   inv_n             1 / n of the gradient
//   CELL, cell        whether cells carry a weight, and the weight of crop cell cy * Wc + cx; a cell of weight 0 leaves the
//                     crop, so its targets are not read
//   OW, out           whether outputs carry a weight, and the weight of (step, output); weight 0 reads no target
//   weight, grad      the element's f64 weight from the two, and d loss / d pred
//   HEAD_DOT          whether the fused pass forms its prediction by head_dot or by the loop it had (see head_dot)
//   Mix               what closes the fold: NS and the loss from the folded sums
struct LossMseL1 {                               // what LossPlain and LossMap share
  static constexpr int NS = 4;
  static constexpr bool OW = false;
  static constexpr bool BASE = false;            // no residual form: the default spec reproduces their bits (LossSpecRes)
  static constexpr bool HEAD_DOT = false;        // the fused pass keeps the loop it had: head_dot there costs the default step a wave per SIMD
  using Mix = LossMseL1;
  struct Sums { double s2, s1, sy, syy; };      // (an aggregate, zeroed by `= {}`: a constructor call would stand between the kernel and its early passes)
  __device__ __forceinline__ double mix(double s0, double s1, double, double count) const { return s0 / count + s1 / count; }
  __device__ __forceinline__ float out(size_t, int, int) const { return 1.f; }
  __device__ __forceinline__ double weight(double wd, float) const { return wd; }
};

struct LossPlain : LossMseL1 {                   // (receives wgt and cnt without reading them)
  static constexpr bool CELL = false;
  __device__ __forceinline__ LossPlain(const float*, double) {}
  __device__ __forceinline__ double inv_n(int N, int O, int Hc, int Wc) const { return 1.0 / ((double)N * O * Hc * Wc); }
  __device__ __forceinline__ float cell(size_t) const { return 1.f; }
  __device__ __forceinline__ Sums add(Sums s, double, float d, float t) const {
    s.s2 += (double)d * d;
    s.s1 += fabs((double)d);
    s.sy += t;
    s.syy += (double)t * t;
    return s;
  }
  __device__ __forceinline__ float grad(float d, double inv_n, double) const {
    return (float)((2.0 * d + (d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0))) * inv_n);
  }
};

struct LossMap : LossMseL1 {
  static constexpr bool CELL = true;
  const float* wgt; double cnt;                  // cnt = N * O * wsum
  __device__ __forceinline__ LossMap(const float* wgt_, double cnt_) : wgt(wgt_), cnt(cnt_) {}
  __device__ __forceinline__ double inv_n(int, int, int, int) const { return 1.0 / cnt; }
  __device__ __forceinline__ float cell(size_t cyx) const { return wgt[cyx]; }
  __device__ __forceinline__ Sums add(Sums s, double wd, float d, float t) const {
    s.s2 += wd * ((double)d * d);
    s.s1 += wd * fabs((double)d);
    s.sy += wd * t;
    s.syy += wd * ((double)t * t);
    return s;
  }
  __device__ __forceinline__ float grad(float d, double inv_n, double wd) const {
    return (float)(((2.0 * d + (d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0))) * inv_n) * wd);
  }
};

// The spec's coefficients as the kernels receive them, and the closing mix (a zero coefficient's term is not formed).
struct LossSpecK {
  double a, b, c, delta;       // coefficients and the Huber threshold
  const float* ow;             // weight per output (plain, fused) or per (step, output) (sequence); nullptr: 1
  static constexpr int NS = 5;
  __device__ __forceinline__ double mix(double s0, double s1, double sh, double count) const {
#pragma clang fp contract(off)
    double loss = 0.0;
    bool any = false;
    if (a != 0.0) { loss = a * (s0 / count); any = true; }
    if (b != 0.0) { const double t = b * (s1 / count); loss = any ? loss + t : t; any = true; }
    if (c != 0.0) { const double t = c * (sh / count); loss = any ? loss + t : t; }
    return loss;
  }
};

// The running sums join their terms with ONE fused multiply-add each -- what the compiler makes of LossMap::add
// (s2 += wd * ((double)d * d) is v_fmac_f64 there), spelled out here so that spec (1, 1, 0) keeps those bits whatever the
// optimiser does with this body.
struct LossSpecSums {
  double s2 = 0, s1 = 0, sy = 0, syy = 0, sh = 0;
  __device__ __forceinline__ void add(double Wd, float d, float t, double hub) {
    s2 = __builtin_fma(Wd, (double)d * d, s2);
    s1 = __builtin_fma(Wd, fabs((double)d), s1);
    sy = __builtin_fma(Wd, (double)t, sy);
    syy = __builtin_fma(Wd, (double)t * t, syy);
    sh = __builtin_fma(Wd, hub, sh);
  }
};

// H(d) and d loss / d pred of one live element: f64, left to right, every operation rounded on its own
__device__ __forceinline__ double loss_spec_huber(const LossSpecK& sp, float df) {
#pragma clang fp contract(off)
  if (sp.c == 0.0) return 0.0;
  const double d = df, ad = fabs(d);
  return ad <= sp.delta ? (0.5 * d) * d : sp.delta * (ad - 0.5 * sp.delta);
}
__device__ __forceinline__ float loss_spec_grad(const LossSpecK& sp, float df, double inv_n, double Wd) {
#pragma clang fp contract(off)
  const double d = df;
  double g = 0.0;
  bool any = false;
  if (sp.a != 0.0) { g = sp.a * (2.0 * d); any = true; }
  if (sp.b != 0.0) {
    const double t = sp.b * (df > 0.f ? 1.0 : (df < 0.f ? -1.0 : 0.0));
    g = any ? g + t : t; any = true;
  }
  if (sp.c != 0.0) {
    const double t = sp.c * (d > sp.delta ? sp.delta : (d < -sp.delta ? -sp.delta : d));   // comparisons: a NaN d stays NaN
    g = any ? g + t : t;
  }
  return (float)((g * inv_n) * Wd);
}

struct LossSpec {
  static constexpr int NS = 5;
  static constexpr bool CELL = true, OW = true, HEAD_DOT = true, BASE = false;
  using Mix = LossSpecK;
  using Sums = LossSpecSums;
  const float* wgt; double cnt; LossSpecK k;     // wgt may be nullptr; cnt = images * (osum or O) * (wsum or Hc * Wc)
  __device__ __forceinline__ LossSpec(const float* wgt_, double cnt_, const LossSpecK& k_) : wgt(wgt_), cnt(cnt_), k(k_) {}
  __device__ __forceinline__ double inv_n(int, int, int, int) const { return 1.0 / cnt; }
  __device__ __forceinline__ float cell(size_t cyx) const { return wgt ? wgt[cyx] : 1.f; }
  __device__ __forceinline__ float out(size_t step, int O, int o) const { return k.ow ? k.ow[step * O + o] : 1.f; }
  __device__ __forceinline__ double weight(double wd, float q) const { return (double)q * wd; }
  __device__ __forceinline__ Sums add(Sums s, double Wd, float d, float t) const { s.add(Wd, d, t, loss_spec_huber(k, d)); return s; }
  __device__ __forceinline__ float grad(float d, double inv_n, double Wd) const { return loss_spec_grad(k, d, inv_n, Wd); }
};

// LossSpec for the RESIDUAL HEAD (the _res fused entries): the same element; the fused pass adds the base it
// carries to every dot product (head_add_base), so the loss, d loss / d pred and dL/dh see p = d + base.  Built from the kernel's
// arguments (wgt, cnt, LossSpecK, HeadBaseK); the closing fold is LossSpec's and takes the LossSpecK alone.
struct LossSpecRes : LossSpec {
  static constexpr bool BASE = true;
  HeadBaseK base;
  __device__ __forceinline__ LossSpecRes(const float* wgt_, double cnt_, const LossSpecK& k_, const HeadBaseK& b_) : LossSpec(wgt_, cnt_, k_), base(b_) {}
};

// The fold of a workgroup's NQ running sums, red[q][thread] -> red[q][0]: a fixed-order tree from `half` threads down.
// (Text, not a function: behind a call the early passes lose the loop, and loss_final_kernel compiles differently.)
#define LOSS_WG_FOLD(red, NQ, half) \
  __syncthreads(); \
  for (int st_ = (half); st_ > 0; st_ >>= 1) { \
    if ((int)threadIdx.x < st_) \
      for (int q_ = 0; q_ < (NQ); ++q_) red[q_][threadIdx.x] += red[q_][threadIdx.x + st_]; \
    __syncthreads(); \
  }

// Coef: nothing, or the LossSpecK of LossSpec -- the other instances keep the argument list they had
template <class Elem, class... Coef>
__global__ __launch_bounds__(1024) void loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                           float* __restrict__ dpred, double* __restrict__ partial,
                                                           int N, int O, int H, int W, int oy, int ox, int Hc, int Wc,
                                                           const float* __restrict__ wgt, double cnt, const Coef... sp) {
  const Elem e(wgt, cnt, sp...);
  const size_t total = (size_t)N * O * H * W;
  const double inv_n = e.inv_n(N, O, Hc, Wc);
  typename Elem::Sums s = {};
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    size_t r = i / W;
    const int yy = r % H;
    const size_t no = r / H;
    const int cy = yy - oy, cx = x - ox;
    float g = 0.f;
    if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) {
      const float cw = e.cell((size_t)cy * Wc + cx), q = e.out(0, O, (int)(no % (size_t)O));
      if (cw != 0.f && q != 0.f) {
        const double Wd = e.weight(cw, q);
        const float t = y[(no * Hc + cy) * Wc + cx];
        const float d = pred[i] - t;
        s = e.add(s, Wd, d, t);
        g = e.grad(d, inv_n, Wd);
      }
    }
    if (dpred) dpred[i] = g;
  }
  constexpr int NS = Elem::NS;
  __shared__ double red[NS][1024];
  red[0][threadIdx.x] = s.s2; red[1][threadIdx.x] = s.s1; red[2][threadIdx.x] = s.sy; red[3][threadIdx.x] = s.syy;
  if constexpr (NS == 5) red[4][threadIdx.x] = s.sh;
  LOSS_WG_FOLD(red, NS, blockDim.x >> 1)
  if (threadIdx.x < NS) partial[blockIdx.x * NS + threadIdx.x] = red[threadIdx.x][0];
}

template <class Mix, class... Coef>
__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ loss_out,
                                                         double* __restrict__ stats, double count, const Coef... sp) {
  // thread (b, q) = one partial; fixed-order tree over the blocks
  constexpr int NS = Mix::NS;
  __shared__ double red[NS][256];
  for (int q = 0; q < NS; ++q) {
    double s = 0;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += partial[b * NS + q];
    red[q][threadIdx.x] = s;
  }
  LOSS_WG_FOLD(red, NS, 128)
  if (threadIdx.x == 0) {
    const double s0 = red[0][0], s1 = red[1][0], s2 = red[2][0], s3 = red[3][0];
    const double loss = Mix{sp...}.mix(s0, s1, NS == 5 ? red[NS - 1][0] : 0.0, count);
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

// The caller's scratch, loss_out: [0] = the loss, [1] = padding, then from [2] (8-byte aligned) NS doubles per workgroup of
// the partial-sum launch.  The plain pass runs LOSS_BLOCKS workgroups, the fused pass up to LOSS_BLOCKS_MAX -- what both
// NINT_LOSS_SCRATCH_FLOATS (4 sums) and NINT_LOSS_SPEC_SCRATCH_FLOATS (5 sums) hold.
#define LOSS_BLOCKS 256
#define LOSS_BLOCKS_MAX ((NINT_LOSS_SCRATCH_FLOATS - 2) / 8)
static_assert((NINT_LOSS_SPEC_SCRATCH_FLOATS - 2) / 10 == LOSS_BLOCKS_MAX, "the spec passes take the grids of their twins: the same partials per sum");
static_assert(LOSS_BLOCKS <= LOSS_BLOCKS_MAX, "the plain pass fits the same scratch");

// the plain pass: cnt is the n of the loss (the final kernel's count); k: the LossSpecK of LossSpec
template <class Elem, class... Coef>
static int loss_launch(const float* pred, const float* y, const float* wgt, double cnt, float* dpred, float* loss_out, double* stats,
                       int N, int O, int H, int W, int oy, int ox, int Hc, int Wc, void* stream, const Coef... k) {
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)(loss_out + 2);
  hipLaunchKernelGGL((loss_partial_kernel<Elem, Coef...>), dim3(LOSS_BLOCKS), dim3(1024), 0, st, pred, y, dpred, partial, N, O, H, W, oy, ox, Hc, Wc, wgt, cnt, k...);
  NINT_LAUNCH_CHECK();
  hipLaunchKernelGGL((loss_final_kernel<typename Elem::Mix, Coef...>), dim3(1), dim3(256), 0, st, partial, LOSS_BLOCKS, loss_out, stats, cnt, k...);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// The checks the loss entries share.  Crop window inside H x W; `area`: the entries that take weights also refuse an empty one.
static inline bool loss_crop_ok(int H, int W, int oy, int ox, int Hc, int Wc, bool area) {
  return oy >= 0 && ox >= 0 && oy + Hc <= H && ox + Wc <= W && (!area || (Hc > 0 && Wc > 0));
}
// the weight map of the _weighted entries: present, and a total that is positive and finite (!(wsum > 0) also catches NaN)
static inline bool loss_weights_ok(const float* wgt, double wsum) { return wgt && wsum > 0.0 && wsum <= DBL_MAX; }
// loss_out holds doubles from [2]; the map and ow (either may be nullptr) are float arrays
static inline bool loss_aligned(const float* loss_out, const float* wgt, const float* ow) {
  return (((uintptr_t)loss_out) & 7) == 0 && ((((uintptr_t)wgt) | ((uintptr_t)ow)) & 3) == 0;
}
// The spec's own checks (nint.h).  nout: O of the plain and fused entries, T*O of the sequence entry.
static int loss_spec_check(const nint_loss_spec* sp, int nout, const float* wgt, double wsum) {
  if (!sp) return NINT_E_ARG;
  const double co[3] = {sp->mse, sp->l1, sp->huber};
  for (double v : co)
    if (!(v >= 0.0) || v > DBL_MAX) return NINT_E_ARG;
  if (sp->mse == 0.0 && sp->l1 == 0.0 && sp->huber == 0.0) return NINT_E_ARG;
  if (sp->huber != 0.0 && (!(sp->delta > 0.0) || sp->delta > DBL_MAX)) return NINT_E_ARG;
  if (sp->ow) {
    if (sp->now != nout || !(sp->osum > 0.0) || sp->osum > DBL_MAX) return NINT_E_ARG;
  } else if (sp->now != 0) {
    return NINT_E_ARG;
  }
  if (wgt && !loss_weights_ok(wgt, wsum)) return NINT_E_ARG;
  return NINT_OK;
}
static inline LossSpecK loss_spec_k(const nint_loss_spec* sp) {
  return LossSpecK{sp->mse, sp->l1, sp->huber, sp->huber != 0.0 ? sp->delta : 1.0, sp->ow};
}
// cnt = images * (osum or outputs) * (wsum or Hc * Wc), left to right (nint.h).  With ow the sequence entry's weights run
// over (step, output): `images` is then B, not T*B.
static inline double loss_spec_cnt(const nint_loss_spec* sp, int images, int O, const float* wgt, double wsum, int Hc, int Wc) {
  return (double)images * (sp->ow ? sp->osum : (double)O) * (wgt ? wsum : (double)Hc * Wc);
}

extern "C" int nint_loss_mse_l1_crop(const float* pred, const float* y, float* dpred, float* loss_out, double* stats,
                                     int N, int O, int H, int W, int oy, int ox, int Hc, int Wc, void* stream) {
  if (!pred || !y || !loss_out || N <= 0 || O <= 0 || !loss_crop_ok(H, W, oy, ox, Hc, Wc, false)) return NINT_E_ARG;
  if (!loss_aligned(loss_out, nullptr, nullptr)) return NINT_E_ALIGN;
  return loss_launch<LossPlain>(pred, y, nullptr, (double)N * O * Hc * Wc, dpred, loss_out, stats, N, O, H, W, oy, ox, Hc, Wc, stream);
}

extern "C" int nint_loss_mse_l1_crop_weighted(const float* pred, const float* y, const float* wgt, double wsum, float* dpred,
                                              float* loss_out, double* stats, int N, int O, int H, int W, int oy, int ox,
                                              int Hc, int Wc, void* stream) {
  if (!pred || !y || !loss_out || N <= 0 || O <= 0 || !loss_crop_ok(H, W, oy, ox, Hc, Wc, true)) return NINT_E_ARG;
  if (!loss_weights_ok(wgt, wsum)) return NINT_E_ARG;
  if (!loss_aligned(loss_out, wgt, nullptr)) return NINT_E_ALIGN;
  return loss_launch<LossMap>(pred, y, wgt, (double)N * O * wsum, dpred, loss_out, stats, N, O, H, W, oy, ox, Hc, Wc, stream);
}

extern "C" int nint_loss_crop_spec(const float* pred, const float* y, const float* wgt, double wsum, const nint_loss_spec* spec,
                                   float* dpred, float* loss_out, double* stats, int N, int O, int H, int W, int oy, int ox,
                                   int Hc, int Wc, void* stream) {
  if (!pred || !y || !loss_out || N <= 0 || O <= 0 || !loss_crop_ok(H, W, oy, ox, Hc, Wc, true)) return NINT_E_ARG;
  const int rc = loss_spec_check(spec, O, wgt, wsum);
  if (rc != NINT_OK) return rc;
  if (!loss_aligned(loss_out, wgt, spec->ow)) return NINT_E_ALIGN;
  return loss_launch<LossSpec>(pred, y, wgt, loss_spec_cnt(spec, N, O, wgt, wsum, Hc, Wc), dpred, loss_out, stats, N, O, H, W, oy, ox, Hc, Wc,
                               stream, loss_spec_k(spec));
}

// ------------------------------------------------------------------------------ head + loss, fused (training)
// train.py:96-109 around the 1x1 head in ONE pass over the pixels: pred = w . h + b (model.py:274), crop, the loss element's
// partial sums (train.py:102,105), d loss / d pred, and dL/dh = w^T . dpred.  One thread per pixel (grid-stride):
// the channel vector is read once, pred never goes to memory, dpred is written for the head's weight gradient.
// Same arithmetic, in the same order, as head_fwd_kernel -> loss_partial_kernel<Elem> -> head_bwd_dh_kernel.
// (HEAD_OCH outputs per chunk: head_staged_holds)
// SEQ (the _seq_ entries): the images are all T*B steps of the slab, image n = t*B + b; the targets are (B, T, O, Hc, Wc),
// plane block b*T + t (head_image); dpred and dh stay in image order, which is what the weight-gradient stage and BPTT read.
// Elem: the pixel's weight is read once per pass, next to the crop test, and a cell of weight 0 leaves the crop: neither its
// targets nor its prediction enter anything.  LossSpec reads the output's weight with its target.  The static LDS is the 8 KiB
// of four sums for every policy -- a fifth sum folds through red[0] after the other four -- and with it the limit
// (head_staged_holds).
template <int DT, int CHV, bool SEQ, class Elem>
__device__ __forceinline__ void head_loss_body(char* smem_hl, const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                               const float* __restrict__ w, const float* __restrict__ b,
                                               const float* __restrict__ y, float* __restrict__ dpred,
                                               void* __restrict__ dh, double* __restrict__ partial, int H, int W,
                                               int P, int Hh, int Wh, int oy, int ox, int Hc, int Wc, int Bs, const Elem e) {
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
  const double inv_n = e.inv_n(N, O, Hc, Wc);
  constexpr int CQ = CHV / 4;                    // channels per wave in phase 2
  typename Elem::Sums s = {};
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
    bool in = live && cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
    double wd = 1.0;
    if constexpr (Elem::CELL) {
      const float wf = in ? e.cell((size_t)cy * Wc + cx) : 0.f;
      in = in && wf != 0.f;
      wd = wf;
    }
    const size_t step = SEQ ? n / Bs : 0;        // of the pixel's image n = t*B + b: the row of the (step, output) weights
    float* dp = dpred + ((size_t)n * O * H + yy) * W + x;
    const float* yp = y + (head_image<SEQ>(n, Bs, N / (SEQ ? Bs : 1)) * O * Hc + cy) * Wc + cx;
    size_t xb = 0;                               // residual head: the pixel's base, fetched with the targets of the outputs that count
    if constexpr (Elem::BASE) xb = head_base_at(e.base, (size_t)n, yy, x, P, Hh, Wh);
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
        float tq[OU], qq[OU];                    // targets and output weights (0: outside the crop, or past the wave's outputs)
#pragma unroll
        for (int u = 0; u < OU; ++u) qq[u] = (in && o0 + u < oe) ? (Elem::OW ? e.out(step, O, o0 + u) : 1.f) : 0.f;
#pragma unroll
        for (int u = 0; u < OU; ++u) tq[u] = (Elem::OW ? qq[u] != 0.f : in && o0 + u < oe) ? yp[(size_t)(o0 + u) * Hc * Wc] : 0.f;
        [[maybe_unused]] float bq[OU];
        if constexpr (Elem::BASE) {
#pragma unroll
          for (int u = 0; u < OU; ++u) bq[u] = qq[u] != 0.f ? load_elem<DT>(e.base.xs, xb + (o0 + u)) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < OU; ++u) {
          const int o = o0 + u;
          if (o >= oe) break;
          float p = b ? b[o] : 0.f;
          if constexpr (Elem::HEAD_DOT) {
            p = head_dot<CHV>(p, w_s + o * CHV, hv);
            if constexpr (Elem::BASE) p = head_add_base(p, bq[u]);
          } else {                               // head_dot's chain as the optimiser forms it from this loop (see head_dot)
            const f32x4_t* wr = (const f32x4_t*)(w_s + o * CHV);
#pragma unroll
            for (int c = 0; c < CHV; c += 4) {
              const f32x4_t wv = wr[c / 4];
              p += wv[0] * hv[c]; p += wv[1] * hv[c + 1]; p += wv[2] * hv[c + 2]; p += wv[3] * hv[c + 3];
            }
          }
          float gq = 0.f;
          if (Elem::OW ? qq[u] != 0.f : in) {
            const float t = tq[u];
            const float d = p - t;
            const double Wd = e.weight(wd, qq[u]);
            s = e.add(s, Wd, d, t);
            gq = e.grad(d, inv_n, Wd);
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
  constexpr int NS = Elem::NS;
  __shared__ double red[4][256];
  red[0][threadIdx.x] = s.s2; red[1][threadIdx.x] = s.s1; red[2][threadIdx.x] = s.sy; red[3][threadIdx.x] = s.syy;
  LOSS_WG_FOLD(red, 4, 128)
  if (threadIdx.x < 4) partial[blockIdx.x * NS + threadIdx.x] = red[threadIdx.x][0];
  if constexpr (NS == 5) {                       // the fifth sum, by the same tree
    __syncthreads();
    red[0][threadIdx.x] = s.sh;
    LOSS_WG_FOLD(red, 1, 128)
    if (threadIdx.x == 0) partial[blockIdx.x * NS + 4] = red[0][0];
  }
}

// Coef: nothing, or the LossSpecK of LossSpec (loss_partial_kernel)
template <int DT, int CHV, bool SEQ, class Elem, class... Coef>
__global__ __launch_bounds__(256) void head_loss_kernel(const void* __restrict__ h, int n0, int N, int Ch, int Chp, int O,
                                                        const float* __restrict__ w, const float* __restrict__ b,
                                                        const float* __restrict__ y, float* __restrict__ dpred,
                                                        void* __restrict__ dh, double* __restrict__ partial, int H, int W,
                                                        int P, int Hh, int Wh, int oy, int ox, int Hc, int Wc, int Bs,
                                                        const float* __restrict__ wgt, double cnt, const Coef... sp) {
  extern __shared__ __attribute__((aligned(16))) char smem_hl[];
  head_loss_body<DT, CHV, SEQ>(smem_hl, h, n0, N, Ch, Chp, O, w, b, y, dpred, dh, partial, H, W, P, Hh, Wh, oy, ox, Hc, Wc, Bs, Elem(wgt, cnt, sp...));
}

// the closing fold of a fused pass: loss_final_kernel<Mix> with the first of the pass's coefficient arguments, if any (LossSpecRes
// carries its base behind the LossSpecK, which the fold has no use for)
template <class Mix>
static void loss_final_first(hipStream_t st, double* partial, int nblk, float* loss_out, double* stats, double cnt) {
  hipLaunchKernelGGL((loss_final_kernel<Mix>), dim3(1), dim3(256), 0, st, partial, nblk, loss_out, stats, cnt);
}
template <class Mix, class K0, class... Rest>
static void loss_final_first(hipStream_t st, double* partial, int nblk, float* loss_out, double* stats, double cnt, const K0& k0, const Rest&...) {
  hipLaunchKernelGGL((loss_final_kernel<Mix, K0>), dim3(1), dim3(256), 0, st, partial, nblk, loss_out, stats, cnt, k0);
}

// The fused pass.  SEQ: the sequence entry (n0 = Bs = B, N = T*B).  cnt: the n of the loss; k: the LossSpecK of LossSpec
template <bool SEQ, class Elem, class... Coef>
static int head_loss_launch(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                            const float* y, const float* wgt, double cnt, float* dpred, void* dh, float* loss_out,
                            double* stats, const nint_geom* g, int oy, int ox, int Hc, int Wc, int dtype, int Bs, void* stream,
                            const Coef... k) {
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)(loss_out + 2);
  // 64 pixels per workgroup and pass: up to LOSS_BLOCKS_MAX workgroups
  const size_t npix = (size_t)N * g->H * g->W;
  const int nblk = (int)((npix + 63) / 64 < LOSS_BLOCKS_MAX ? (npix + 63) / 64 : LOSS_BLOCKS_MAX);
  if (!head_staged_holds(Chp, O)) return NINT_E_SHAPE;
  const size_t lds = head_loss_lds(Chp, O);
  const int rc = nint_by_dtype(dtype, [&](auto dt) { return head_by_chv(Chp, [&](auto chv) -> int {
    auto kern = head_loss_kernel<decltype(dt)::value, decltype(chv)::value, SEQ, Elem, Coef...>;
    if (lds + 8192 > 64 * 1024) NINT_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), lds, st, h_slab, n0, N, Ch, Chp, O, w, b, y, dpred, dh, partial, g->H, g->W, g->P, g->Hh, g->Wh, oy, ox, Hc, Wc, Bs, wgt, cnt, k...);
    return NINT_OK; }); });
  if (rc != NINT_OK) return rc;
  NINT_LAUNCH_CHECK();
  loss_final_first<typename Elem::Mix>(st, partial, nblk, loss_out, stats, cnt, k...);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// what the one-step fused entries check first (the sequence entries: head_seq_args_ok)
static bool head_loss_args_ok(const void* h_slab, int N, int Ch, int O, const float* w, const nint_geom* g, int dtype) {
  return h_slab && w && g && N > 0 && O > 0 && Ch > 0 && (dtype == NINT_BF16 || dtype == NINT_F32);
}
// the 16-byte channel vectors of the sequence entries' slabs
static inline bool head_seq_aligned(const void* h_slab, const void* dh_seq) { return ((((uintptr_t)h_slab) | ((uintptr_t)dh_seq)) & 15) == 0; }

// Every fused entry: NINT_E_ARG, then NINT_E_SHAPE for the channel count (wider heads run nint_head_fwd[_seq] + the plain
// loss entry of the same element + nint_head_bwd[_seq]), then NINT_E_ALIGN, then the launcher's NINT_E_SHAPE for the LDS.
extern "C" int nint_head_loss_fused(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                    const float* y, float* dpred, void* dh, float* loss_out, double* stats, const nint_geom* g,
                                    int oy, int ox, int Hc, int Wc, int dtype, void* stream) {
  if (!y || !dpred || !dh || !loss_out || !head_loss_args_ok(h_slab, N, Ch, O, w, g, dtype)) return NINT_E_ARG;
  if (!loss_crop_ok(g->H, g->W, oy, ox, Hc, Wc, false)) return NINT_E_ARG;
  if (Chp > 128 || Chp % 4) return NINT_E_SHAPE;
  if (!loss_aligned(loss_out, nullptr, nullptr)) return NINT_E_ALIGN;
  return head_loss_launch<false, LossPlain>(h_slab, n0, N, Ch, Chp, O, w, b, y, nullptr, (double)N * O * Hc * Wc, dpred, dh, loss_out, stats, g,
                                            oy, ox, Hc, Wc, dtype, 0, stream);
}

extern "C" int nint_head_loss_fused_weighted(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                             const float* y, const float* wgt, double wsum, float* dpred, void* dh, float* loss_out,
                                             double* stats, const nint_geom* g, int oy, int ox, int Hc, int Wc, int dtype, void* stream) {
  if (!y || !dpred || !dh || !loss_out || !head_loss_args_ok(h_slab, N, Ch, O, w, g, dtype)) return NINT_E_ARG;
  if (!loss_crop_ok(g->H, g->W, oy, ox, Hc, Wc, true) || !loss_weights_ok(wgt, wsum)) return NINT_E_ARG;
  if (Chp > 128 || Chp % 4) return NINT_E_SHAPE;
  if (!loss_aligned(loss_out, wgt, nullptr)) return NINT_E_ALIGN;
  return head_loss_launch<false, LossMap>(h_slab, n0, N, Ch, Chp, O, w, b, y, wgt, (double)N * O * wsum, dpred, dh, loss_out, stats, g,
                                          oy, ox, Hc, Wc, dtype, 0, stream);
}

// (the _spec entries are their _res twins without a base: the twin's checks in the twin's order, then the base's)
extern "C" int nint_head_loss_fused_res(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                        const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred,
                                        void* dh, float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc,
                                        int Wc, int dtype, const nint_head_base* base, void* stream) {
  if (!y || !dpred || !dh || !loss_out || !head_loss_args_ok(h_slab, N, Ch, O, w, g, dtype)) return NINT_E_ARG;
  if (!loss_crop_ok(g->H, g->W, oy, ox, Hc, Wc, true)) return NINT_E_ARG;
  int rc = loss_spec_check(spec, O, wgt, wsum);
  if (rc != NINT_OK) return rc;
  if (Chp > 128 || Chp % 4) return NINT_E_SHAPE;
  if (!loss_aligned(loss_out, wgt, spec->ow)) return NINT_E_ALIGN;
  HeadBaseK k; bool on;
  if ((rc = head_base_check(base, O, dtype, &k, &on)) != NINT_OK) return rc;
  const double cnt = loss_spec_cnt(spec, N, O, wgt, wsum, Hc, Wc);
  if (on)
    return head_loss_launch<false, LossSpecRes>(h_slab, n0, N, Ch, Chp, O, w, b, y, wgt, cnt, dpred, dh, loss_out, stats, g, oy, ox, Hc, Wc,
                                                dtype, 0, stream, loss_spec_k(spec), k);
  return head_loss_launch<false, LossSpec>(h_slab, n0, N, Ch, Chp, O, w, b, y, wgt, cnt, dpred, dh,
                                           loss_out, stats, g, oy, ox, Hc, Wc, dtype, 0, stream, loss_spec_k(spec));
}

extern "C" int nint_head_loss_fused_spec(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                         const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred,
                                         void* dh, float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc,
                                         int Wc, int dtype, void* stream) {
  return nint_head_loss_fused_res(h_slab, n0, N, Ch, Chp, O, w, b, y, wgt, wsum, spec, dpred, dh, loss_out, stats, g, oy, ox, Hc, Wc, dtype,
                                  nullptr, stream);
}

extern "C" int nint_head_loss_seq_fused(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                        const float* y, float* dpred, void* dh_seq, float* loss_out, double* stats,
                                        const nint_geom* g, int oy, int ox, int Hc, int Wc, int dtype, void* stream) {
  if (!y || !dpred || !dh_seq || !loss_out || !head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if (!loss_crop_ok(g->H, g->W, oy, ox, Hc, Wc, true)) return NINT_E_ARG;
  if (Chp > 128) return NINT_E_SHAPE;
  if (!loss_aligned(loss_out, nullptr, nullptr) || !head_seq_aligned(h_slab, dh_seq)) return NINT_E_ALIGN;
  return head_loss_launch<true, LossPlain>(h_slab, B, T * B, Ch, Chp, O, w, b, y, nullptr, (double)(T * B) * O * Hc * Wc, dpred, dh_seq, loss_out,
                                           stats, g, oy, ox, Hc, Wc, dtype, B, stream);
}

extern "C" int nint_head_loss_seq_fused_weighted(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                                 const float* y, const float* wgt, double wsum, float* dpred, void* dh_seq,
                                                 float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc,
                                                 int Wc, int dtype, void* stream) {
  if (!y || !dpred || !dh_seq || !loss_out || !head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if (!loss_crop_ok(g->H, g->W, oy, ox, Hc, Wc, true) || !loss_weights_ok(wgt, wsum)) return NINT_E_ARG;
  if (Chp > 128) return NINT_E_SHAPE;
  if (!loss_aligned(loss_out, wgt, nullptr) || !head_seq_aligned(h_slab, dh_seq)) return NINT_E_ALIGN;
  return head_loss_launch<true, LossMap>(h_slab, B, T * B, Ch, Chp, O, w, b, y, wgt, (double)(T * B) * O * wsum, dpred, dh_seq, loss_out,
                                         stats, g, oy, ox, Hc, Wc, dtype, B, stream);
}

extern "C" int nint_head_loss_seq_fused_res(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                            const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred,
                                            void* dh_seq, float* loss_out, double* stats, const nint_geom* g, int oy, int ox,
                                            int Hc, int Wc, int dtype, const nint_head_base* base, void* stream) {
  if (!y || !dpred || !dh_seq || !loss_out || !head_seq_args_ok(h_slab, B, T, Ch, Chp, O, w, g, dtype)) return NINT_E_ARG;
  if (!loss_crop_ok(g->H, g->W, oy, ox, Hc, Wc, true) || (long long)T * O > INT_MAX) return NINT_E_ARG;
  int rc = loss_spec_check(spec, T * O, wgt, wsum);
  if (rc != NINT_OK) return rc;
  if (Chp > 128) return NINT_E_SHAPE;
  if (!loss_aligned(loss_out, wgt, spec->ow) || !head_seq_aligned(h_slab, dh_seq)) return NINT_E_ALIGN;
  HeadBaseK k; bool on;
  if ((rc = head_base_check(base, O, dtype, &k, &on)) != NINT_OK) return rc;
  // with ow the weights run over (step, output): cnt = B * osum * wsum; without, the twin's (T*B) * O * wsum
  const double cnt = loss_spec_cnt(spec, spec->ow ? B : T * B, O, wgt, wsum, Hc, Wc);
  if (on)
    return head_loss_launch<true, LossSpecRes>(h_slab, B, T * B, Ch, Chp, O, w, b, y, wgt, cnt, dpred, dh_seq, loss_out, stats, g, oy, ox, Hc,
                                               Wc, dtype, B, stream, loss_spec_k(spec), k);
  return head_loss_launch<true, LossSpec>(h_slab, B, T * B, Ch, Chp, O, w, b, y, wgt, cnt, dpred, dh_seq, loss_out, stats, g, oy, ox, Hc, Wc,
                                          dtype, B, stream, loss_spec_k(spec));
}

extern "C" int nint_head_loss_seq_fused_spec(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                             const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred,
                                             void* dh_seq, float* loss_out, double* stats, const nint_geom* g, int oy, int ox,
                                             int Hc, int Wc, int dtype, void* stream) {
  return nint_head_loss_seq_fused_res(h_slab, B, T, Ch, Chp, O, w, b, y, wgt, wsum, spec, dpred, dh_seq, loss_out, stats, g, oy, ox, Hc, Wc,
                                      dtype, nullptr, stream);
}

// ------------------------------------------------------------------------------ evaluation: skill sums (test.ipynb)
// What the analysis notebook computes from the gathered predictions -- r_squared_temporal (:377-385), r_squared_spatial
// (:462-485), the time-mean maps (:605,:630) and the cos-latitude weighted means (:684-693,:796-803) -- follows from running
// f64 sums: five per map cell and accumulator set ("slot": sum y, sum p, sum y^2, sum p^2, sum (y-p)^2) and eight per
// (sample, output) over the crop.  One pass forms them from the prediction (nint_skill_accum) or straight from the top
// layer's hidden state (nint_head_skill_accum: the head of head_fwd_body, pred never in memory).
//
// Mapping: grid = (256-pixel blocks of the crop, groups of SKILL_OG outputs); a thread owns ONE crop pixel and SKILL_OG
// outputs for the whole call -- the (slot, o, cy, cx) cells of every slot.  The host orders the call's samples by slot
// (stable: n ascending inside a slot, slot -1 last), so a slot's five sums of a cell are loaded once, grow in registers in
// sample order and are stored once: bit-identical run to run and under any split of the samples into consecutive calls (a
// store and reload of an f64 changes nothing).  No atomics.  The per-sample sums are reduced per wave by a fixed exchange
// tree (skill_wave_fold), one partial row per (sample, output, wave), and folded in a fixed order by skill_fold_kernel:
// block mapping and fold order depend on (O, Hc, Wc) only, never on N or on the sample's position in the call.
// Arithmetic: d = (double)p - (double)y, every product and every sum a separate f64 operation (contraction is off in the
// shared body, so both entries and every instance round alike).
#define SKILL_OG 4
struct SkillPlan { int32_t slot[NINT_SKILL_MAX_N]; uint8_t idx[NINT_SKILL_MAX_N]; };   // the call's samples in slot order

// (skill_wave_fold, the per-wave sum of eight values at once: nint_common.h -- ensemble.hip forms its sample rows with it too)

// the prediction of (sample n, output o0 + u) at the thread's pixel, from memory ...
struct SkillPredPlain {
  const float* __restrict__ pred; int O, o0; size_t HW, off;
  __device__ __forceinline__ void sample(int) {}
  __device__ __forceinline__ float operator()(int n, int u) const { return pred[((size_t)n * O + o0 + u) * HW + off]; }
};
// ... or from the hidden state: head_fwd_body's arithmetic (zero-padded weight rows in LDS, head_dot), so pred_out matches
// nint_head_fwd bit for bit.  The sample's predictions wait in the thread's LDS column p_s for operator().
template <int DT, int CHV>
struct SkillPredHead {
  const void* __restrict__ h; const float* w_s; float* p_s; const float* __restrict__ b; int n0, Chp, o0, on; size_t img, off;
  __device__ __forceinline__ void sample(int n) {
    // (the weight rows stay in LDS: without this fence their reads are hoisted out of the sample loop into registers)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const size_t hb = (size_t)(n0 + n) * img + off;
    float hv[CHV];
#pragma unroll
    for (int c = 0; c < CHV; c += 4) {
      const f32x4_t v = (c < Chp) ? load_vec4<DT>(h, hb + c) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
      hv[c] = v[0]; hv[c + 1] = v[1]; hv[c + 2] = v[2]; hv[c + 3] = v[3];
    }
#pragma unroll 1                                 // (one output's weight row in registers at a time)
    for (int u = 0; u < on; ++u) p_s[u * 256 + threadIdx.x] = head_dot<CHV>(b ? b[o0 + u] : 0.f, w_s + u * CHV, hv);
  }
  __device__ __forceinline__ float operator()(int, int u) const { return p_s[u * 256 + threadIdx.x]; }
};

// the accumulation both entries share.  q = the thread's crop pixel (clamped; live = inside the crop), o0 / on = its outputs
template <class Src>
__device__ __forceinline__ void skill_accum_body(Src& src, const float* __restrict__ y, double rw, double* __restrict__ pix,
                                                 double* __restrict__ part, float* __restrict__ pred_out, const SkillPlan& plan,
                                                 int N, int O, size_t HWc, size_t q, bool live, int o0, int on) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const size_t NP = (size_t)gridDim.x * 4;                            // partial rows per (sample, output): one per wave
  const size_t prow = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const size_t plane = (size_t)O * HWc;                               // one of a slot's NINT_SKILL_PIX planes
  double acc[SKILL_OG][NINT_SKILL_PIX];
#pragma unroll
  for (int u = 0; u < SKILL_OG; ++u)
#pragma unroll
    for (int k = 0; k < NINT_SKILL_PIX; ++k) acc[u][k] = 0.0;
  int cur = -1;                                                       // the slot whose sums are in acc
  for (int i = 0; i < N; ++i) {
    const int n = plan.idx[i], s = plan.slot[i];
    if (s != cur) {
      if (live) {
#pragma unroll
        for (int u = 0; u < SKILL_OG; ++u)
#pragma unroll
          for (int k = 0; k < NINT_SKILL_PIX; ++k) {
            if (u >= on) continue;
            if (cur >= 0) pix[((size_t)cur * NINT_SKILL_PIX + k) * plane + (size_t)(o0 + u) * HWc + q] = acc[u][k];
            if (s >= 0) acc[u][k] = pix[((size_t)s * NINT_SKILL_PIX + k) * plane + (size_t)(o0 + u) * HWc + q];
          }
      }
      cur = s;
    }
    src.sample(n);
    float tq[SKILL_OG];
#pragma unroll
    for (int u = 0; u < SKILL_OG; ++u) tq[u] = u < on ? y[((size_t)n * O + o0 + u) * HWc + q] : 0.f;
#pragma unroll
    for (int u = 0; u < SKILL_OG; ++u) {
      if (u >= on) continue;                                          // (block-uniform)
      const float pf = src(n, u);
      if (pred_out && live) pred_out[((size_t)n * O + o0 + u) * HWc + q] = pf;
      const double p = live ? (double)pf : 0.0, t = live ? (double)tq[u] : 0.0;   // lanes past the crop add zeros
      const double d = p - t;
      const double dd = d * d, tt = t * t, pp = p * p;
      if (s >= 0) {
        acc[u][0] += t; acc[u][1] += p; acc[u][2] += tt; acc[u][3] += pp; acc[u][4] += dd;
      }
      const double v[NINT_SKILL_SAMPLE] = {dd, fabs(d), t, tt, p, pp, rw * t, rw * p};
      const double tot = skill_wave_fold(v, lane);
      if ((lane & 7) == 0) part[(((size_t)n * O + o0 + u) * NP + prow) * NINT_SKILL_SAMPLE + (lane >> 3)] = tot;
    }
  }
  if (cur >= 0 && live) {
#pragma unroll
    for (int u = 0; u < SKILL_OG; ++u)
#pragma unroll
      for (int k = 0; k < NINT_SKILL_PIX; ++k)
        if (u < on) pix[((size_t)cur * NINT_SKILL_PIX + k) * plane + (size_t)(o0 + u) * HWc + q] = acc[u][k];
  }
}

__global__ __launch_bounds__(256) void skill_accum_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                          const double* __restrict__ row_w, double* __restrict__ pix,
                                                          double* __restrict__ part, const SkillPlan plan, int N, int O, int H,
                                                          int W, int oy, int ox, int Hc, int Wc) {
  const size_t HWc = (size_t)Hc * Wc, q0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = q0 < HWc;
  const size_t q = live ? q0 : HWc - 1;
  const int cy = (int)(q / Wc), cx = (int)(q - (size_t)cy * Wc);
  const int o0 = blockIdx.y * SKILL_OG, on = min(SKILL_OG, O - o0);
  SkillPredPlain src{pred, O, o0, (size_t)H * W, (size_t)(cy + oy) * W + (cx + ox)};
  skill_accum_body(src, y, row_w ? row_w[cy] : 1.0, pix, part, nullptr, plan, N, O, HWc, q, live, o0, on);
}

template <int DT, int CHV>
__global__ __launch_bounds__(256) void head_skill_accum_kernel(const void* __restrict__ h, int n0, int Ch, int Chp,
                                                               const float* __restrict__ w, const float* __restrict__ b,
                                                               const float* __restrict__ y, const double* __restrict__ row_w,
                                                               double* __restrict__ pix, double* __restrict__ part,
                                                               float* __restrict__ pred_out, const SkillPlan plan, int N, int O,
                                                               int P, int Hh, int Wh, int oy, int ox, int Hc, int Wc) {
  __shared__ __attribute__((aligned(16))) float w_s[SKILL_OG * CHV];
  __shared__ float p_s[SKILL_OG * 256];                                // the thread's predictions of one sample
  const int o0 = blockIdx.y * SKILL_OG, on = min(SKILL_OG, O - o0);
  head_stage_weights<CHV>(w_s, w + (size_t)o0 * Ch, on, Ch);           // the group's rows of [O][CHV]
  const size_t HWc = (size_t)Hc * Wc, q0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = q0 < HWc;
  const size_t q = live ? q0 : HWc - 1;
  const int cy = (int)(q / Wc), cx = (int)(q - (size_t)cy * Wc);
  SkillPredHead<DT, CHV> src;
  src.h = h; src.w_s = w_s; src.p_s = p_s; src.b = b; src.n0 = n0; src.Chp = Chp; src.o0 = o0; src.on = on;
  src.img = (size_t)Hh * Wh * Chp;
  src.off = ((size_t)(cy + oy + P) * Wh + (cx + ox + P)) * Chp;
  skill_accum_body(src, y, row_w ? row_w[cy] : 1.0, pix, part, pred_out, plan, N, O, HWc, q, live, o0, on);
}

// sample[pair][k] = the NP partial rows of pair = (sample, output) in a fixed order: one wave per pair, lane = (j, k) adds the
// rows j, j + 8, ..., then the eight j in order
__global__ __launch_bounds__(256) void skill_fold_kernel(const double* __restrict__ part, double* __restrict__ sample, int npair, int NP) {
  const int lane = threadIdx.x & 63, pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= npair) return;                                           // (a whole wave)
  const int k = lane & 7, j = lane >> 3;
  const double* p = part + (size_t)pair * NP * NINT_SKILL_SAMPLE;
  double s = 0.0;
#pragma unroll 4
  for (int i = j; i < NP; i += 8) s += p[(size_t)i * NINT_SKILL_SAMPLE + k];
  double t = __shfl(s, k);
  for (int jj = 1; jj < 8; ++jj) t += __shfl(s, jj * 8 + k);
  if (j == 0) sample[(size_t)pair * NINT_SKILL_SAMPLE + k] = t;
}

int nint_internal_skill_fold_enqueue(const double* part, double* sample, int npair, int NP, void* stream) {
  hipLaunchKernelGGL(skill_fold_kernel, dim3(nint_cdiv(npair, 4)), dim3(256), 0, (hipStream_t)stream, part, sample, npair, NP);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

static inline size_t skill_pix_blocks(int Hc, int Wc) { return ((size_t)Hc * Wc + 255) / 256; }

extern "C" size_t nint_skill_scratch_bytes(int N, int O, int Hc, int Wc) {
  if (N <= 0 || O <= 0 || Hc <= 0 || Wc <= 0) return 0;
  const size_t nc = N < NINT_SKILL_MAX_N ? N : NINT_SKILL_MAX_N;       // larger calls run in pieces that reuse the scratch
  return nc * O * skill_pix_blocks(Hc, Wc) * 4 * NINT_SKILL_SAMPLE * sizeof(double);
}

// the checks both entries share (H x W: the grid the crop window lies in)
static int skill_args_check(const float* y, const int32_t* slot, int nslots, const double* pix, const double* sample,
                            const double* scratch, size_t scratch_bytes, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc) {
  if (!y || !pix || !sample || !scratch || N <= 0 || O <= 0 || Hc <= 0 || Wc <= 0 || nslots < 1) return NINT_E_ARG;
  if (oy < 0 || ox < 0 || oy + Hc > H || ox + Wc > W) return NINT_E_ARG;
  if (slot)
    for (int n = 0; n < N; ++n)
      if (slot[n] < -1 || slot[n] >= nslots) return NINT_E_ARG;
  if (scratch_bytes < nint_skill_scratch_bytes(N, O, Hc, Wc)) return NINT_E_ARG;
  return NINT_OK;
}

// pieces of at most NINT_SKILL_MAX_N samples: launch(first sample, count, plan), then the fold of that piece's partial rows
template <class L>
static int skill_run(const int32_t* slot, double* sample, double* scratch, int N, int O, int Hc, int Wc, hipStream_t st, L&& launch) {
  const int NP = (int)skill_pix_blocks(Hc, Wc) * 4;
  for (int c0 = 0; c0 < N; c0 += NINT_SKILL_MAX_N) {
    const int nc = N - c0 < NINT_SKILL_MAX_N ? N - c0 : NINT_SKILL_MAX_N;
    int order[NINT_SKILL_MAX_N];
    for (int i = 0; i < nc; ++i) order[i] = i;
    auto key = [&](int i) { const int s = slot ? slot[c0 + i] : 0; return s < 0 ? INT_MAX : s; };
    std::stable_sort(order, order + nc, [&](int a, int b) { return key(a) < key(b); });
    SkillPlan plan = {};
    for (int i = 0; i < nc; ++i) {
      plan.idx[i] = (uint8_t)order[i];
      plan.slot[i] = slot ? slot[c0 + order[i]] : 0;
    }
    launch(c0, nc, plan);
    NINT_LAUNCH_CHECK();
    const int rc = nint_internal_skill_fold_enqueue(scratch, sample + (size_t)c0 * O * NINT_SKILL_SAMPLE, nc * O, NP, st);
    if (rc != NINT_OK) return rc;
  }
  return NINT_OK;
}

extern "C" int nint_skill_accum(const float* pred, const float* y, const int32_t* slot, int nslots, const double* row_w,
                                double* pix, double* sample, double* scratch, size_t scratch_bytes, int N, int O, int H, int W,
                                int oy, int ox, int Hc, int Wc, void* stream) {
  if (!pred) return NINT_E_ARG;
  const int rc = skill_args_check(y, slot, nslots, pix, sample, scratch, scratch_bytes, N, O, H, W, oy, ox, Hc, Wc);
  if (rc != NINT_OK) return rc;
  if (((((uintptr_t)pix) | ((uintptr_t)sample) | ((uintptr_t)scratch) | ((uintptr_t)row_w)) & 7) != 0) return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)skill_pix_blocks(Hc, Wc), (unsigned)nint_cdiv(O, SKILL_OG));
  const size_t HWc = (size_t)Hc * Wc;
  return skill_run(slot, sample, scratch, N, O, Hc, Wc, st, [&](int c0, int nc, const SkillPlan& plan) {
    hipLaunchKernelGGL(skill_accum_kernel, grid, dim3(256), 0, st, pred + (size_t)c0 * O * H * W, y + (size_t)c0 * O * HWc, row_w,
                       pix, scratch, plan, nc, O, H, W, oy, ox, Hc, Wc);
  });
}

extern "C" int nint_head_skill_accum(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                     const float* y, const int32_t* slot, int nslots, const double* row_w, double* pix,
                                     double* sample, float* pred_out, double* scratch, size_t scratch_bytes, const nint_geom* g,
                                     int oy, int ox, int Hc, int Wc, int dtype, void* stream) {
  if (!h_slab || !w || !g || Ch <= 0 || Chp < Ch || n0 < 0) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  const int rc = skill_args_check(y, slot, nslots, pix, sample, scratch, scratch_bytes, N, O, g->H, g->W, oy, ox, Hc, Wc);
  if (rc != NINT_OK) return rc;
  // nint_head_loss_fused's limits (one rule for both fused head passes: SeqEngine._beyond_fused_head)
  if (Chp > 128 || Chp % 4) return NINT_E_SHAPE;
  if (((size_t)O * head_chv(Chp) + (size_t)(O < HEAD_OCH ? O : HEAD_OCH) * 64) * sizeof(float) + 8192 > 160 * 1024) return NINT_E_SHAPE;
  if (((((uintptr_t)pix) | ((uintptr_t)sample) | ((uintptr_t)scratch) | ((uintptr_t)row_w)) & 7) != 0 || (((uintptr_t)h_slab) & 15) != 0) return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)skill_pix_blocks(Hc, Wc), (unsigned)nint_cdiv(O, SKILL_OG));
  const size_t HWc = (size_t)Hc * Wc;
  return skill_run(slot, sample, scratch, N, O, Hc, Wc, st, [&](int c0, int nc, const SkillPlan& plan) {
    nint_by_dtype(dtype, [&](auto dt) { head_by_chv(Chp, [&](auto chv) {
      hipLaunchKernelGGL((head_skill_accum_kernel<decltype(dt)::value, decltype(chv)::value>), grid, dim3(256), 0, st, h_slab, n0 + c0,
                         Ch, Chp, w, b, y + (size_t)c0 * O * HWc, row_w, pix, scratch,
                         pred_out ? pred_out + (size_t)c0 * O * HWc : (float*)nullptr, plan, nc, O, g->P, g->Hh, g->Wh, oy, ox, Hc, Wc);
    }); });
  });
}
