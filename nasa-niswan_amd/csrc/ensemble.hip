// ensemble.hip -- ensemble statistics of M member predictions against one target, on the device.
//
// Per cell (sample n, output o, crop pixel), all in f64, every product and every sum its own operation (contraction is off), no
// division:   x_i = member i, t = target, dM = (double)M
//   S = x_0 + ... + x_{M-1}  (in that order)        E = S - dM*t
//   A = sum_i |x_i - t|      (i ascending)           V = sum_i (dM*x_i - S)^2   (i ascending)
//   D = sum_{i<j} |x_i - x_j|  ((i, j) in lexicographic order)
//   r = #{i : x_i < t};  a cell whose target or any member is NaN goes to bin M + 1 instead of bin r
// From these sums the host derives the ensemble mean's MSE, the spread, the fair and the plain CRPS, the bias and R2
// (inference.ensemble_from_sums); keeping the division by M there makes integer data exact for every M.
//
// Mapping: skill_accum_kernel's (head.hip).  grid = (256-pixel blocks of the crop, groups of ENS_OG outputs); a thread owns ONE
// crop pixel and takes its group's outputs one after the other, so it owns the (slot, o, cy, cx) cells of every slot for the whole
// call.  The host orders the call's samples by slot (stable: n ascending inside a slot, slot -1 last); a slot's seven sums of a cell
// are loaded once, grow in registers in sample order and are stored once: bit-identical run to run and under any split of the
// samples into consecutive calls.  The members of a cell are read once (consecutive lanes read consecutive pixels of every member
// image) and wait in the thread's own LDS column x_s[i][thread] for the pair loop -- M * 1 KiB of dynamic LDS per workgroup, no
// bank conflict, no barrier (no thread reads another's column).
// The per-sample sums: one partial row per (sample, output, wave) by skill_wave_fold, folded in a fixed order by
// skill_fold_kernel (head.hip); block mapping and fold order depend on (O, Hc, Wc) only.
// The rank histogram: integer counts, so any reduction is exact.  A workgroup counts the cells of one (slot, output) with LDS
// integer atomics into hist_s[M + 2] and adds the non-zero bins to rank_hist with vector global 64-bit atomics when the slot
// changes and after the last sample.
#include <algorithm>
#include <climits>
#include "nint_common.h"

#define ENS_OG 4
static_assert(NINT_ENS_SAMPLE == NINT_SKILL_SAMPLE, "the sample rows go through skill_wave_fold and skill_fold_kernel");
static_assert(NINT_ENS_MAX_N <= 256, "EnsPlan::idx is a byte");

// the call's samples in slot order: where each one's member 0 lies (elements from pred), its slot, its index in the piece
struct EnsPlan { int64_t off[NINT_ENS_MAX_N]; int32_t slot[NINT_ENS_MAX_N]; uint8_t idx[NINT_ENS_MAX_N]; };

__global__ __launch_bounds__(256) void ens_accum_kernel(const float* __restrict__ pred, int64_t member_stride, int M,
                                                        const float* __restrict__ y, const double* __restrict__ row_w,
                                                        double* __restrict__ pix, double* __restrict__ part,
                                                        unsigned long long* __restrict__ rank_hist, float* __restrict__ mean_out,
                                                        const EnsPlan plan, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc) {
#pragma clang fp contract(off)
  extern __shared__ float x_s[];                                       // [M][256]: the thread's members of one cell
  __shared__ int hist_s[NINT_ENS_MAX_M + 2];                           // the workgroup's counts of one (slot, output)
  const int tid = threadIdx.x, lane = tid & 63, NB = M + 2;
  const size_t HWc = (size_t)Hc * Wc, HW = (size_t)H * W, q0 = (size_t)blockIdx.x * 256 + tid;
  const bool live = q0 < HWc;
  const size_t q = live ? q0 : HWc - 1;                                // (lanes past the crop read its last pixel and add zeros)
  const int cy = (int)(q / Wc), cx = (int)(q - (size_t)cy * Wc);
  const size_t goff = (size_t)(cy + oy) * W + (cx + ox);
  const int o0 = blockIdx.y * ENS_OG, on = min(ENS_OG, O - o0);
  const double rw = row_w ? row_w[cy] : 1.0, dM = (double)M;
  const size_t NP = (size_t)gridDim.x * 4;                             // partial rows per (sample, output): one per wave
  const size_t prow = (size_t)blockIdx.x * 4 + (tid >> 6);
  const size_t plane = (size_t)O * HWc;                                // one of a slot's NINT_ENS_PIX planes
  float* xc = x_s + tid;
  if (tid < NB) hist_s[tid] = 0;                                       // (every store of a slot's counts leaves zeros behind)
  __syncthreads();

  for (int u = 0; u < on; ++u) {                                       // (block-uniform)
    const int o = o0 + u;
    double acc[NINT_ENS_PIX];
#pragma unroll
    for (int k = 0; k < NINT_ENS_PIX; ++k) acc[k] = 0.0;
    int cur = -1;                                                      // the slot whose sums are in acc and whose counts in hist_s
    for (int i = 0; i <= N; ++i) {                                     // turn N: the last slot's store
      const int s = i < N ? plan.slot[i] : -1;
      if (s != cur) {                                                  // (block-uniform)
        if (cur >= 0) {
          __syncthreads();                                             // every count of slot `cur` is in hist_s
          if (tid < NB) {
            const int c = hist_s[tid];
            if (c) atomicAdd(rank_hist + ((size_t)cur * O + o) * NB + tid, (unsigned long long)c);
            hist_s[tid] = 0;
          }
          __syncthreads();
        }
        if (live) {
#pragma unroll
          for (int k = 0; k < NINT_ENS_PIX; ++k) {
            if (cur >= 0) pix[((size_t)cur * NINT_ENS_PIX + k) * plane + (size_t)o * HWc + q] = acc[k];
            if (s >= 0) acc[k] = pix[((size_t)s * NINT_ENS_PIX + k) * plane + (size_t)o * HWc + q];
          }
        }
        cur = s;
      }
      if (i == N) break;
      const int n = plan.idx[i];
      const float tf = y[((size_t)n * O + o) * HWc + q];
      const float* pm = pred + plan.off[i] + (size_t)o * HW + goff;
      const double t = live ? (double)tf : 0.0;
      double S = 0.0, A = 0.0;
      int r = 0;
      bool bad = tf != tf;
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        const float xf = live ? pm[(size_t)m * member_stride] : 0.f;
        xc[m * 256] = xf;
        const double x = (double)xf;
        S += x;
        A += fabs(x - t);
        r += x < t;
        bad |= xf != xf;
      }
      double V = 0.0, D = 0.0;
      for (int m = 0; m < M; ++m) {
        const double xm = (double)xc[m * 256];
        const double dv = dM * xm - S;
        V += dv * dv;
        for (int j = m + 1; j < M; ++j) D += fabs(xm - (double)xc[j * 256]);
      }
      const double E = S - dM * t;
      const double EE = E * E;
      if (mean_out && live) mean_out[((size_t)n * O + o) * HWc + q] = (float)(S / dM);   // the one division, outside every sum
      if (s >= 0) {
        acc[0] += EE; acc[1] += V; acc[2] += A; acc[3] += D; acc[4] += E; acc[5] += t; acc[6] += t * t;
        if (live) atomicAdd(&hist_s[bad ? M + 1 : r], 1);
      }
      const double v[NINT_ENS_SAMPLE] = {EE, V, A, D, rw * EE, rw * V, rw * A, rw * D};
      const double tot = skill_wave_fold(v, lane);
      if ((lane & 7) == 0) part[(((size_t)n * O + o) * NP + prow) * NINT_ENS_SAMPLE + (lane >> 3)] = tot;
    }
  }
}

static inline size_t ens_pix_blocks(int Hc, int Wc) { return ((size_t)Hc * Wc + 255) / 256; }

extern "C" size_t nint_ens_scratch_bytes(int N, int M, int O, int Hc, int Wc) {
  if (N <= 0 || M <= 0 || O <= 0 || Hc <= 0 || Wc <= 0) return 0;
  const size_t nc = N < NINT_ENS_MAX_N ? N : NINT_ENS_MAX_N;           // larger calls run in pieces that reuse the scratch
  return nc * O * ens_pix_blocks(Hc, Wc) * 4 * NINT_ENS_SAMPLE * sizeof(double);   // (the histogram needs none: any M)
}

extern "C" int nint_ens_accum(const float* pred, const int64_t* sample_off, int64_t member_stride, int M, const float* y,
                              const int32_t* slot, int nslots, const double* row_w, double* pix, double* sample,
                              int64_t* rank_hist, float* mean_out, double* scratch, size_t scratch_bytes, int N, int O, int H,
                              int W, int oy, int ox, int Hc, int Wc, void* stream) {
  if (!pred || !sample_off || !y || !pix || !sample || !rank_hist || !scratch) return NINT_E_ARG;
  if (M < 2 || M > NINT_ENS_MAX_M || N < 1 || O < 1 || nslots < 1 || member_stride < 0) return NINT_E_ARG;
  if (Hc < 1 || Wc < 1 || oy < 0 || ox < 0 || oy + Hc > H || ox + Wc > W) return NINT_E_ARG;
  for (int n = 0; n < N; ++n) {
    if (sample_off[n] < 0) return NINT_E_ARG;
    if (slot && (slot[n] < -1 || slot[n] >= nslots)) return NINT_E_ARG;
  }
  if (scratch_bytes < nint_ens_scratch_bytes(N, M, O, Hc, Wc)) return NINT_E_ARG;
  if (((((uintptr_t)pix) | ((uintptr_t)sample) | ((uintptr_t)rank_hist) | ((uintptr_t)scratch) | ((uintptr_t)row_w)) & 7) != 0) return NINT_E_ALIGN;
  if (((((uintptr_t)pred) | ((uintptr_t)y) | ((uintptr_t)mean_out)) & 3) != 0) return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ens_pix_blocks(Hc, Wc), (unsigned)nint_cdiv(O, ENS_OG));
  const int NP = (int)grid.x * 4;
  const size_t HWc = (size_t)Hc * Wc;
  for (int c0 = 0; c0 < N; c0 += NINT_ENS_MAX_N) {                     // pieces of at most NINT_ENS_MAX_N samples, as skill_run's
    const int nc = N - c0 < NINT_ENS_MAX_N ? N - c0 : NINT_ENS_MAX_N;
    int order[NINT_ENS_MAX_N];
    for (int i = 0; i < nc; ++i) order[i] = i;
    auto key = [&](int i) { const int s = slot ? slot[c0 + i] : 0; return s < 0 ? INT_MAX : s; };
    std::stable_sort(order, order + nc, [&](int a, int b) { return key(a) < key(b); });
    EnsPlan plan = {};
    for (int i = 0; i < nc; ++i) {
      plan.idx[i] = (uint8_t)order[i];
      plan.slot[i] = slot ? slot[c0 + order[i]] : 0;
      plan.off[i] = sample_off[c0 + order[i]];
    }
    hipLaunchKernelGGL(ens_accum_kernel, grid, dim3(256), (size_t)M * 256 * sizeof(float), st, pred, member_stride, M,
                       y + (size_t)c0 * O * HWc, row_w, pix, scratch, (unsigned long long*)rank_hist,
                       mean_out ? mean_out + (size_t)c0 * O * HWc : (float*)nullptr, plan, nc, O, H, W, oy, ox, Hc, Wc);
    NINT_LAUNCH_CHECK();
    const int rc = nint_internal_skill_fold_enqueue(scratch, sample + (size_t)c0 * O * NINT_ENS_SAMPLE, nc * O, NP, st);
    if (rc != NINT_OK) return rc;
  }
  return NINT_OK;
}
