// Input noise (nint.h): seeded Gaussian noise on a span of the input slab's channels, drawn on the device from a
// counter-based generator.  The noise of element (draw, lane, step, channel offset o, pixel) is a pure function of those five
// numbers and the seed -- one Philox4x32-10 block per (pixel, o / 4, step, lane) under the key (seed, draw) -- whatever launch
// produces it: the sweep and the recompute of a segmented window, a plain and a folded slab, one rank or many see the same values.
#include "nint_common.h"

// (the generator -- philox4x32_10, noise_pair, noise_quad -- lives in nint_common.h: head.hip inlines it too, for the noise on the
// fed-back value)

// ------------------------------------------------------------------------------ z alone (nint_noise_normal)
struct NormalPlan {
  int B, n, nq, H, W;
  uint32_t seed, draw, step0, lane0;
  size_t items;      // T*B * nq * H*W
};

// One item = (image, quad, pixel), the pixel fastest: a wave stores 64 consecutive floats of up to four channel planes.
__global__ __launch_bounds__(256) void noise_normal_kernel(float* __restrict__ out, NormalPlan a) {
  const size_t hw = (size_t)a.H * a.W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.items; i += (size_t)gridDim.x * 256) {
    const size_t pix = i % hw, r = i / hw;
    const int q = (int)(r % a.nq), img = (int)(r / a.nq);
    const f32x4_t z = noise_quad((uint32_t)pix, (uint32_t)q, a.step0 + (uint32_t)(img / a.B), a.lane0 + (uint32_t)(img % a.B), a.seed, a.draw);
    float* o = out + ((size_t)img * a.n + 4 * (size_t)q) * hw + pix;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < a.n) o[(size_t)j * hw] = z[j];
  }
}

// ------------------------------------------------------------------------------ the slab update (nint_input_noise)
// One workgroup per (image row, chunk of XT pixels); like head_feedback_kernel (head.hip) it forms the row's values once, stages
// them in LDS and lets every destination gather its own:
//   (1) items (window pixel wx, quad q): the window is the chunk widened by kf/2 pixels on either side -- the pixels the chunk's
//       fold copies mirror; its key pixel is x0 - kf/2 + wx, taken mod W on a cyclic slab and skipped outside the row on a
//       zero-padded one.  One Philox block gives the four normals of channels 4q .. 4q + 3; what is staged is the addend
//       __fmul_rn(sigma[o], z), p_s[wx][n4], beside the sigmas themselves, s_s[n4] (0 beyond n).
//   (2) items (pixel x, fold copy kx, dword j of that copy's span), consecutive lanes on consecutive dwords.  Slab channel
//       kx*Cx + c0 + o of pixel x holds pixel x + kx - kf/2, window pixel (x - x0) + kx.  A lane loads its dword, adds the addend
//       to each element that is in a span, is in the row and has sigma != 0, rounds to ET and stores the WHOLE dword if any
//       element changed: every dword has one owner, so a bf16 dword with one span half and one foreign half (an odd first
//       channel, an odd n) is read, merged and written by one lane.  Where the copies touch (n == Cx, so the spans form one run)
//       and a copy starts on an odd channel, its first dword also holds the last element of the copy before: that copy's last
//       item owns it and the later copy's item 0 stands down.
// Nothing else of xs is touched: no halo pixel, no slack column, no pad channel, no other channel.
struct NoisePlan {
  char* xs; const float* sigma;
  int B, Cx, Cxp, c0, n, nq, q0, kf, cyc, H, W, P, Hh, Wh, XT, nxc;
  uint32_t seed, draw, step0, lane0;
};

template <int DT>
__global__ __launch_bounds__(256) void input_noise_kernel(void* __restrict__ xs_, const float* __restrict__ sigma, NoisePlan a) {
  extern __shared__ __attribute__((aligned(16))) char smem_noise[];
  constexpr int ES = Elem<DT>::ES, EPD = 4 / ES;
  const int n4 = 4 * a.nq, half = a.kf >> 1;
  float* __restrict__ s_s = (float*)smem_noise;     // [n4]
  float* __restrict__ p_s = s_s + n4;                // [WX][n4]
  const int rowi = blockIdx.x / a.nxc, xc = blockIdx.x - rowi * a.nxc;
  const int y = rowi % a.H, img = rowi / a.H;
  const int x0 = xc * a.XT, xt = min(a.XT, a.W - x0), WX = xt + a.kf - 1;
  const uint32_t step = a.step0 + (uint32_t)(img / a.B), lane = a.lane0 + (uint32_t)(img % a.B);
  for (int o = threadIdx.x; o < n4; o += 256) s_s[o] = o < a.n ? sigma[o] : 0.f;
  for (int i = threadIdx.x; i < WX * a.nq; i += 256) {
    const int wx = i / a.nq, q = i - wx * a.nq;
    int xk = x0 - half + wx;
    if (a.cyc) xk = xk < 0 ? xk + a.W : (xk >= a.W ? xk - a.W : xk);
    if (xk < 0 || xk >= a.W) continue;
    const f32x4_t z = noise_quad((uint32_t)(y * a.W + xk), (uint32_t)(a.q0 + q), step, lane, a.seed, a.draw);
    f32x4_t p;
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = 4 * q + j < a.n ? __fmul_rn(sigma[4 * q + j], z[j]) : 0.f;
    *(f32x4_t*)(p_s + (size_t)wx * n4 + 4 * q) = p;
  }
  __syncthreads();
  const size_t row = ((size_t)img * a.Hh + (y + a.P)) * a.Wh + a.P;          // first interior pixel of the row
  const bool run = a.kf > 1 && a.n == a.Cx;                                  // the copies' spans touch
  const int ndm = a.n / EPD + 1;                                             // dwords a copy's span can cover, either parity
  for (int i = threadIdx.x; i < xt * a.kf * ndm; i += 256) {
    const int xl = i / (a.kf * ndm), r = i - xl * (a.kf * ndm), kx = r / ndm, j = r - kx * ndm;
    const int s = kx * a.Cx + a.c0, d = s / EPD + j;                          // the copy's first span channel; this item's dword
    if (d * EPD >= s + a.n) continue;                                         // (beyond this copy's span)
    if (run && kx > 0 && j == 0 && (s % EPD) != 0) continue;                  // (owned by the copy before)
    char* px = (char*)xs_ + ((row + x0 + xl) * (size_t)a.Cxp + (size_t)d * EPD) * ES;
    float add[EPD]; bool on[EPD];
    bool any = false;
#pragma unroll
    for (int e = 0; e < EPD; ++e) {
      int o = d * EPD + e - s, k2 = kx;
      if (run && o < 0) { o += a.n; --k2; }
      else if (run && o >= a.n && kx + 1 < a.kf) { o -= a.n; ++k2; }
      const int xi = x0 + xl + k2 - half;                                     // the mirrored pixel (before the wrap)
      on[e] = o >= 0 && o < a.n && (a.cyc || (xi >= 0 && xi < a.W)) && s_s[o] != 0.f;
      add[e] = on[e] ? p_s[(size_t)(xl + k2) * n4 + o] : 0.f;
      any |= on[e];
    }
    if (!any) continue;
    if constexpr (DT == NINT_BF16) {
      const uint32_t w = *(const uint32_t*)px;
      const uint16_t lo = on[0] ? f2bf(__fadd_rn(bf2f((uint16_t)(w & 0xffffu)), add[0])) : (uint16_t)(w & 0xffffu);
      const uint16_t hi = on[1] ? f2bf(__fadd_rn(bf2f((uint16_t)(w >> 16)), add[1])) : (uint16_t)(w >> 16);
      *(uint32_t*)px = (uint32_t)lo | ((uint32_t)hi << 16);
    } else {
      *(float*)px = __fadd_rn(*(const float*)px, add[0]);
    }
  }
}

// ------------------------------------------------------------------------------ entries
static constexpr int NOISE_LDS_FLOATS = 16384;        // 64 KiB: no opt-in, and two workgroups a CU
static constexpr int NOISE_MAX_FOLD = 4095;           // the window of one pixel and one quad still fits

static int noise_geom_check(const nint_geom* g) {
  if (g->H <= 0 || g->W <= 0 || g->P < 0 || g->Hh < g->H + 2 * g->P || g->Wh < g->W + 2 * g->P) return NINT_E_ARG;
  return NINT_OK;
}

extern "C" int nint_input_noise(void* xs_slab, int x_n0, int B, int T, int Cx, int Cxp, int c0, int n, const float* sigma,
                                int xfold_k, int lon_cyclic, uint32_t seed, uint32_t draw, uint32_t step0, uint32_t lane0,
                                const nint_geom* g, int dtype, void* stream) {
  // nint_head_feedback's checks on the slab side, in its order (feedback_check, head.hip)
  if (!xs_slab || !sigma || !g || x_n0 < 0) return NINT_E_ARG;
  if (B <= 0 || T <= 0 || n <= 0 || Cx <= 0) return NINT_E_ARG;
  if (dtype != NINT_BF16 && dtype != NINT_F32) return NINT_E_ARG;
  const int es = dtype == NINT_BF16 ? 2 : 4;
  if (noise_geom_check(g) != NINT_OK) return NINT_E_ARG;
  if (c0 < 0 || c0 > Cx - n) return NINT_E_ARG;
  if (xfold_k < 0 || (xfold_k > 0 && !(xfold_k & 1))) return NINT_E_ARG;
  const int kf = xfold_k > 1 ? xfold_k : 1;
  if ((long long)Cxp < (long long)kf * Cx || ((long long)Cxp * es) % 16 != 0) return NINT_E_ARG;
  if (lon_cyclic != 0 && lon_cyclic != 1) return NINT_E_ARG;
  if (lon_cyclic && (g->W < g->P || g->W < kf / 2)) return NINT_E_ARG;
  if ((long long)B * T > 0x7fffffffLL / g->H) return NINT_E_ARG;             // (image rows are the grid)
  if (((uintptr_t)xs_slab & 15) != 0 || ((uintptr_t)sigma & 3) != 0) return NINT_E_ALIGN;
  if (kf > NOISE_MAX_FOLD) return NINT_E_SHAPE;                               // (a fold no layer has)

  NoisePlan p = {};
  p.xs = (char*)xs_slab + (size_t)x_n0 * g->Hh * g->Wh * Cxp * es;
  p.B = B; p.Cx = Cx; p.Cxp = Cxp; p.kf = kf; p.cyc = lon_cyclic;
  p.H = g->H; p.W = g->W; p.P = g->P; p.Hh = g->Hh; p.Wh = g->Wh;
  p.seed = seed; p.draw = draw; p.step0 = step0; p.lane0 = lane0;
  // Any n runs: a span whose staged window would not fit is cut at multiples of four channels (whole Philox blocks) into
  // launches one behind the other on the stream -- a bf16 dword that two of them share is updated twice, in order.
  const int wmin = g->W < 32 ? g->W : 32;
  int oc = (NOISE_LDS_FLOATS / (kf + wmin)) & ~3;
  if (oc < 4) oc = 4;
  const size_t rows = (size_t)B * T * g->H;
  for (int ob = 0; ob < n; ob += oc) {
    p.n = n - ob < oc ? n - ob : oc;
    p.c0 = c0 + ob; p.q0 = ob / 4; p.nq = (p.n + 3) / 4;
    p.sigma = sigma + ob;
    const int n4 = 4 * p.nq;
    int xt = NOISE_LDS_FLOATS / n4 - kf;            // (1 + XT + kf - 1) * n4 floats
    p.XT = xt < g->W ? xt : g->W;
    p.nxc = (g->W + p.XT - 1) / p.XT;
    if (rows * (size_t)p.nxc > 0x7fffffffull) return NINT_E_ARG;
    const size_t lds = (size_t)(p.XT + kf) * n4 * sizeof(float);
    if (dtype == NINT_BF16)
      hipLaunchKernelGGL(input_noise_kernel<NINT_BF16>, dim3((unsigned)(rows * p.nxc)), dim3(256), lds, (hipStream_t)stream, (void*)p.xs, p.sigma, p);
    else
      hipLaunchKernelGGL(input_noise_kernel<NINT_F32>, dim3((unsigned)(rows * p.nxc)), dim3(256), lds, (hipStream_t)stream, (void*)p.xs, p.sigma, p);
    NINT_LAUNCH_CHECK();
  }
  return NINT_OK;
}

extern "C" int nint_noise_normal(float* out, int B, int T, int n, uint32_t seed, uint32_t draw, uint32_t step0, uint32_t lane0,
                                 const nint_geom* g, void* stream) {
  if (!out || !g || B <= 0 || T <= 0 || n <= 0) return NINT_E_ARG;
  if (noise_geom_check(g) != NINT_OK) return NINT_E_ARG;
  if (((uintptr_t)out & 3) != 0) return NINT_E_ALIGN;
  NormalPlan p = {};
  p.B = B; p.n = n; p.nq = (n + 3) / 4; p.H = g->H; p.W = g->W;
  p.seed = seed; p.draw = draw; p.step0 = step0; p.lane0 = lane0;
  p.items = (size_t)B * T * p.nq * g->H * g->W;
  hipLaunchKernelGGL(noise_normal_kernel, grid1d(p.items), dim3(256), 0, (hipStream_t)stream, out, p);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}
