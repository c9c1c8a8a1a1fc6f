// spectrum.hip -- zonal (along-longitude) power spectra of M member predictions against one target, on the device.
//
// Per row r of the crop of one (sample n, output o), all in f64, with the CALLER'S table tw[Wc][2] (nint_spec_twiddles, or any
// other: the kernel is a linear map with the table it is given and never computes a sine):
//   F_k = sum_x f[x] * (tw[j][0] + i tw[j][1]),  j = (k x) mod Wc,  0 <= k < K = Wc / 2 + 1
//   Y_k the target's transform, P_{i,k} member i's, S_k = sum_i P_{i,k} (i ascending), w = row_w[r] (1 without a table):
//   YY += w |Y|^2     PP += w sum_i |P_i|^2     CR += w Re(S conj Y)     CI += w Im(S conj Y)     SS += w |S|^2
// No division, no normalisation: the host derives densities, ratios and the coherence (inference.spectrum_from_sums).
//
// Two stages.  spec_rows_kernel: grid = (samples of the piece, outputs), one 256-thread workgroup owns every row of its (n, o).
// With Kt = min(K, 256) and R = min(Hc, max(1, 256 / Kt)) a thread is (row-in-tile rl = tid / Kt, wavenumber k = kb + tid % Kt):
// the workgroup walks the crop in tiles of R rows and, per tile, image by image -- the target, then member 0 .. M-1 -- puts the
// tile's rows into LDS as f64 and every thread transforms its row at its k, a chain of Wc fused multiply-adds per component
// from 0.0 with x ascending, the table in LDS.  The five row terms (every product and sum its own operation) are added to the
// thread's five sums, tile after tile; the R threads of a k are then added in ascending rl through LDS and the five sums of
// (n, o, k) go to scratch [n][o][plane][K].  spec_fold_kernel: one thread per (slot, plane, o, k) adds the piece's samples of its
// slot in ascending n to the stored value.  No floating-point atomics; the order is a function of (M, O, Hc, Wc) only, so spec
// is bit-identical run to run, under any split of the samples into consecutive calls and for N beyond one launch.
// A sample with slot -1 is skipped by both stages (its scratch rows are neither written nor read).
#include <cmath>
#include "nint_common.h"

#define SPEC_THREADS 256
static_assert(NINT_SPEC_MAX_W <= 2 * SPEC_THREADS, "K = Wc / 2 + 1 needs at most two passes of SPEC_THREADS wavenumbers");

// the piece's samples: where each one's member 0 lies (elements from pred) and its slot
struct SpecPlan { int64_t off[NINT_SPEC_MAX_N]; int32_t slot[NINT_SPEC_MAX_N]; };

struct SpecGeom { int K, Kt, R; };
static inline SpecGeom spec_geom(int Hc, int Wc) {
  SpecGeom g;
  g.K = Wc / 2 + 1;
  g.Kt = g.K < SPEC_THREADS ? g.K : SPEC_THREADS;
  const int r = SPEC_THREADS / g.Kt;                                    // >= 1
  g.R = r < Hc ? r : Hc;
  return g;
}

// rows [r0, r0 + rn) of the crop of one image (row pitch `pitch` elements, src at the crop's first pixel) -> LDS as f64
__device__ __forceinline__ void spec_stage(const float* __restrict__ src, size_t pitch, int r0, int rn, int Wc, double* f_s, int tid) {
  __syncthreads();                                                     // every thread is done with the image before
  for (int idx = tid; idx < rn * Wc; idx += SPEC_THREADS) {
    const int r = idx / Wc, x = idx - r * Wc;
    f_s[idx] = (double)src[(size_t)(r0 + r) * pitch + x];
  }
  __syncthreads();
}

// F_k of the LDS row f[0 .. Wc): x ascending, one fused multiply-add per component and x, from 0.0
__device__ __forceinline__ void spec_dft(const double* f, const double2* tw_s, int k, int Wc, double& re, double& im) {
  double a = 0.0, b = 0.0;
  int j = 0;
  for (int x = 0; x < Wc; ++x) {
    const double fx = f[x];
    const double2 t = tw_s[j];
    a = __builtin_fma(fx, t.x, a);
    b = __builtin_fma(fx, t.y, b);
    j += k;
    j -= j >= Wc ? Wc : 0;                                             // j = (k x) mod Wc without a division: k < Wc
  }
  re = a; im = b;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_rows_kernel(const float* __restrict__ pred, int64_t member_stride, int M,
                                                                 const float* __restrict__ y, const double* __restrict__ row_w,
                                                                 const double* __restrict__ tw, double* __restrict__ part,
                                                                 const SpecPlan plan, int O, int H, int W, int oy, int ox, int Hc,
                                                                 int Wc, int K, int Kt, int R) {
#pragma clang fp contract(off)
  __shared__ double2 tw_s[NINT_SPEC_MAX_W];                            // the caller's table
  __shared__ double f_s[NINT_SPEC_MAX_W];                              // R rows of one image (R * Wc <= NINT_SPEC_MAX_W)
  __shared__ double red_s[NINT_SPEC_PLANES][SPEC_THREADS];
  const int tid = threadIdx.x, n = blockIdx.x, o = blockIdx.y;
  if (plan.slot[n] < 0) return;                                        // (block-uniform) a sample left out adds nothing
  for (int j = tid; j < Wc; j += SPEC_THREADS) tw_s[j] = make_double2(tw[2 * j], tw[2 * j + 1]);
  const int rl = tid / Kt, kk = tid - rl * Kt;
  const size_t HW = (size_t)H * W;
  const float* yimg = y + ((size_t)n * O + o) * Hc * Wc;
  const float* pimg = pred + plan.off[n] + (size_t)o * HW + (size_t)oy * W + ox;
  const double* frow = f_s + rl * Wc;
  for (int kb = 0; kb < K; kb += Kt) {                                 // (one pass unless K > SPEC_THREADS)
    const int k = kb + kk;
    const bool on = rl < R && k < K;
    double acc[NINT_SPEC_PLANES] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r0 = 0; r0 < Hc; r0 += R) {
      const int rn = min(R, Hc - r0);
      const bool live = on && rl < rn;
      double Yr = 0.0, Yi = 0.0, Sr = 0.0, Si = 0.0, pp = 0.0;
      spec_stage(yimg, (size_t)Wc, r0, rn, Wc, f_s, tid);
      if (live) spec_dft(frow, tw_s, k, Wc, Yr, Yi);
      for (int i = 0; i < M; ++i) {
        spec_stage(pimg + (size_t)i * member_stride, (size_t)W, r0, rn, Wc, f_s, tid);
        if (live) {
          double Pr, Pi;
          spec_dft(frow, tw_s, k, Wc, Pr, Pi);
          Sr += Pr;
          Si += Pi;
          pp += Pr * Pr + Pi * Pi;
        }
      }
      if (live) {
        const double w = row_w ? row_w[r0 + rl] : 1.0;
        acc[0] += w * (Yr * Yr + Yi * Yi);
        acc[1] += w * pp;
        acc[2] += w * (Sr * Yr + Si * Yi);
        acc[3] += w * (Si * Yr - Sr * Yi);
        acc[4] += w * (Sr * Sr + Si * Si);
      }
    }
#pragma unroll
    for (int p = 0; p < NINT_SPEC_PLANES; ++p) red_s[p][tid] = acc[p];
    __syncthreads();
    if (rl == 0 && k < K) {
#pragma unroll
      for (int p = 0; p < NINT_SPEC_PLANES; ++p) {
        double s = red_s[p][kk];
        for (int q = 1; q < R; ++q) s += red_s[p][q * Kt + kk];
        part[(((size_t)n * O + o) * NINT_SPEC_PLANES + p) * K + k] = s;
      }
    }
    __syncthreads();
  }
}

// one owner per (slot, plane, o, k): the stored value plus the piece's samples of the slot in ascending n
__global__ __launch_bounds__(SPEC_THREADS) void spec_fold_kernel(const double* __restrict__ part, double* __restrict__ spec,
                                                                 const SpecPlan plan, int nc, int nslots, int O, int K) {
#pragma clang fp contract(off)
  const size_t e = (size_t)blockIdx.x * SPEC_THREADS + threadIdx.x;
  const size_t POK = (size_t)NINT_SPEC_PLANES * O * K;
  if (e >= (size_t)nslots * POK) return;
  const int s = (int)(e / POK);
  const size_t pok = e - (size_t)s * POK;                              // (plane * O + o) * K + k
  const int p = (int)(pok / ((size_t)O * K));
  const size_t ok = pok - (size_t)p * O * K;
  const int o = (int)(ok / K), k = (int)(ok - (size_t)o * K);
  double v = 0.0;
  bool any = false;
  for (int n = 0; n < nc; ++n) {
    if (plan.slot[n] != s) continue;
    if (!any) { v = spec[e]; any = true; }
    v += part[(((size_t)n * O + o) * NINT_SPEC_PLANES + p) * K + k];
  }
  if (any) spec[e] = v;
}

extern "C" size_t nint_spec_scratch_bytes(int N, int M, int O, int Hc, int Wc) {
  if (N <= 0 || M <= 0 || O <= 0 || Hc <= 0 || Wc < 2) return 0;
  const size_t nc = N < NINT_SPEC_MAX_N ? N : NINT_SPEC_MAX_N;         // larger calls run in pieces that reuse the scratch
  return nc * O * NINT_SPEC_PLANES * (size_t)(Wc / 2 + 1) * sizeof(double);
}

// tw[j] = (cos(2 pi j / Wc), -sin(2 pi j / Wc)): the angle is reduced in integers to a quadrant q and an octant angle
// pi r / (2 Wc), 0 <= 2 r <= Wc, whose cosine and sine are taken in long double and rounded once; the rest is sign changes and
// a swap, so quarter turns are exact, tw[Wc - j] = conj(tw[j]) bit for bit, and no component is a negative zero.
extern "C" int nint_spec_twiddles(int Wc, double* tw) {
  if (!tw || Wc < 2) return NINT_E_ARG;
  if (Wc > NINT_SPEC_MAX_W) return NINT_E_SHAPE;
  const long double half_pi = 1.57079632679489661923132169163975144L;
  for (int j = 0; j < Wc; ++j) {
    const int q = (4 * j) / Wc, r = 4 * j - q * Wc;                    // the angle is (q + r / Wc) quarter turns, 0 <= r < Wc
    const bool swap = 2 * r > Wc;
    const int rr = swap ? Wc - r : r;
    double c, s;
    if (rr == 0) { c = 1.0; s = 0.0; }
    else if (2 * rr == Wc) { c = s = (double)sqrtl(0.5L); }
    else {
      const long double th = half_pi * (long double)rr / (long double)Wc;
      c = (double)cosl(th);
      s = (double)sinl(th);
    }
    const double cq = swap ? s : c, sq = swap ? c : s;                 // of the angle inside the quadrant
    const double co = q == 0 ? cq : q == 1 ? -sq : q == 2 ? -cq : sq;
    const double si = q == 0 ? sq : q == 1 ? cq : q == 2 ? -sq : -cq;
    tw[2 * j] = co + 0.0;                                              // (-0.0 + 0.0 = +0.0)
    tw[2 * j + 1] = -si + 0.0;
  }
  return NINT_OK;
}

extern "C" int nint_spec_accum(const float* pred, const int64_t* sample_off, int64_t member_stride, int M, const float* y,
                               const int32_t* slot, int nslots, const double* row_w, const double* tw, double* spec,
                               double* scratch, size_t scratch_bytes, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc,
                               void* stream) {
  if (!pred || !sample_off || !y || !tw || !spec || !scratch) return NINT_E_ARG;
  if (M < 1 || M > NINT_ENS_MAX_M || N < 1 || O < 1 || nslots < 1 || member_stride < 0) return NINT_E_ARG;
  if (Hc < 1 || Wc < 2 || oy < 0 || ox < 0 || oy + Hc > H || ox + Wc > W) return NINT_E_ARG;
  for (int n = 0; n < N; ++n) {
    if (sample_off[n] < 0) return NINT_E_ARG;
    if (slot && (slot[n] < -1 || slot[n] >= nslots)) return NINT_E_ARG;
  }
  if (Wc > NINT_SPEC_MAX_W) return NINT_E_SHAPE;
  if (scratch_bytes < nint_spec_scratch_bytes(N, M, O, Hc, Wc)) return NINT_E_ARG;
  if (((((uintptr_t)spec) | ((uintptr_t)scratch) | ((uintptr_t)row_w) | ((uintptr_t)tw)) & 7) != 0) return NINT_E_ALIGN;
  if (((((uintptr_t)pred) | ((uintptr_t)y)) & 3) != 0) return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const SpecGeom g = spec_geom(Hc, Wc);
  const size_t entries = (size_t)nslots * NINT_SPEC_PLANES * O * g.K;
  const size_t HWc = (size_t)Hc * Wc;
  for (int c0 = 0; c0 < N; c0 += NINT_SPEC_MAX_N) {                    // pieces of at most NINT_SPEC_MAX_N samples
    const int nc = N - c0 < NINT_SPEC_MAX_N ? N - c0 : NINT_SPEC_MAX_N;
    SpecPlan plan = {};
    bool any = false;
    for (int i = 0; i < nc; ++i) {
      plan.off[i] = sample_off[c0 + i];
      plan.slot[i] = slot ? slot[c0 + i] : 0;
      any |= plan.slot[i] >= 0;
    }
    if (!any) continue;
    hipLaunchKernelGGL(spec_rows_kernel, dim3((unsigned)nc, (unsigned)O), dim3(SPEC_THREADS), 0, st, pred, member_stride, M,
                       y + (size_t)c0 * O * HWc, row_w, tw, scratch, plan, O, H, W, oy, ox, Hc, Wc, g.K, g.Kt, g.R);
    NINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_fold_kernel, dim3((unsigned)((entries + SPEC_THREADS - 1) / SPEC_THREADS)), dim3(SPEC_THREADS), 0, st,
                       scratch, spec, plan, nc, nslots, O, g.K);
    NINT_LAUNCH_CHECK();
  }
  return NINT_OK;
}
