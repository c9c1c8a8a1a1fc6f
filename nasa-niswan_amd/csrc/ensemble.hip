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
#include <cfloat>
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

// ------------------------------------------------------------------------------ the training loss
// nint_ens_loss: the almost-fair CRPS of M member lanes, d loss / d pred of every member and the epoch statistics in one pass
// over the members where they lie (include/nint.h carries the rule).
// Mapping: nothing accumulates per pixel here, so the samples go on the grid: grid = (256-pixel blocks of the FULL H x W image,
// groups of ENS_OG outputs, samples of the piece).  A thread owns one pixel of every member image of its (sample, output): outside
// the crop (or under a zero weight) it stores M zeros; inside it reads the M members once into its own LDS column
// x_s[i][thread] (no bank conflict, no barrier), runs the pair loop from there and stores M gradients.  Consecutive lanes touch
// consecutive pixels in every load and store.  The seven sums of a (sample, output): skill_wave_fold per wave, the workgroup's
// four waves joined in wave order through LDS (the kernel's one barrier), one partial row per (sample, output, workgroup),
// skill_fold_kernel over the workgroups, and ens_loss_final_kernel over the (sample, output) rows in ascending order: no
// floating-point atomics, and no figure depends on how the samples are cut into launches.
struct EnsLossPlan { int64_t poff[NINT_ENS_MAX_N]; int64_t doff[NINT_ENS_MAX_N]; int32_t row[NINT_ENS_MAX_N]; };

// sgn with sgn(0) = 0 that keeps a NaN (comparisons, as C(d) of the spec loss)
__device__ __forceinline__ double ens_sgn(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d); }

__global__ __launch_bounds__(256) void ens_loss_kernel(const float* __restrict__ pred, int64_t pstride, float* __restrict__ dpred,
                                                       int64_t dstride, int M, const float* __restrict__ y,
                                                       const float* __restrict__ wgt, const float* __restrict__ ow, double kp,
                                                       double cnt, double* __restrict__ part, const EnsLossPlan plan, int O, int H,
                                                       int W, int oy, int ox, int Hc, int Wc) {
#pragma clang fp contract(off)
  extern __shared__ float x_s[];                                       // [M][256]: the thread's members of one cell
  __shared__ double red_s[ENS_OG][4][NINT_ENS_SAMPLE];                 // the four waves' sums of each output of the group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.z;
  const size_t HW = (size_t)H * W, HWc = (size_t)Hc * Wc, p = (size_t)blockIdx.x * 256 + tid;
  const bool in_img = p < HW;
  const int py = (int)(p / W), px = (int)(p - (size_t)py * W), cy = py - oy, cx = px - ox;
  const bool in_crop = in_img && cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
  const size_t cyx = in_crop ? (size_t)cy * Wc + cx : 0;
  const float cw = in_crop ? (wgt ? wgt[cyx] : 1.f) : 0.f;
  const int o0 = blockIdx.y * ENS_OG, on = min(ENS_OG, O - o0);
  const double dM = (double)M, inv_n = 1.0 / cnt;
  const float* owr = ow ? ow + (size_t)plan.row[n] * O : nullptr;
  float* xc = x_s + tid;
  for (int u = 0; u < on; ++u) {                                       // (block-uniform)
    const int o = o0 + u;
    const float q = owr ? owr[o] : 1.f;
    float* dp = dpred + plan.doff[n] + (size_t)o * HW + p;
    double v[NINT_ENS_SAMPLE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (in_crop && cw != 0.f && q != 0.f) {                            // Wd != 0: two non-zero f32 have a non-zero f64 product
      const double Wd = (double)q * (double)cw;
      const double t = (double)y[((size_t)n * O + o) * HWc + cyx];
      const float* pm = pred + plan.poff[n] + (size_t)o * HW + p;
      double S = 0.0, A = 0.0;
#pragma unroll 4
      for (int i = 0; i < M; ++i) {
        const float xf = pm[(size_t)i * pstride];
        xc[i * 256] = xf;
        const double x = (double)xf;
        S += x;
        A += fabs(x - t);
      }
      const double m = S / dM;                                         // the one division of the cell: the statistics' mean
      double V = 0.0, D = 0.0;
      for (int i = 0; i < M; ++i) {
        const double xi = (double)xc[i * 256];
        const double dv = dM * xi - S;
        V += dv * dv;
        double R = 0.0;
        for (int j = 0; j < M; ++j) {
          if (j == i) continue;
          const double d = xi - (double)xc[j * 256];
          R += ens_sgn(d);
          if (j > i) D += fabs(d);
        }
        dp[(size_t)i * dstride] = (float)(((ens_sgn(xi - t) / dM - kp * R) * inv_n) * Wd);
      }
      const double e = m - t;
      v[0] = Wd * A; v[1] = Wd * D; v[2] = Wd * V; v[3] = Wd * (e * e); v[4] = Wd * fabs(e); v[5] = Wd * t; v[6] = Wd * (t * t);
    } else if (in_img) {
      for (int i = 0; i < M; ++i) dp[(size_t)i * dstride] = 0.f;
    }
    const double tot = skill_wave_fold(v, lane);
    if ((lane & 7) == 0) red_s[u][wave][lane >> 3] = tot;
  }
  __syncthreads();
  if (tid < on * NINT_ENS_SAMPLE) {
    const int u = tid >> 3, k = tid & 7;
    const double s = ((red_s[u][0][k] + red_s[u][1][k]) + red_s[u][2][k]) + red_s[u][3][k];
    part[(((size_t)n * O + o0 + u) * gridDim.x + blockIdx.x) * NINT_ENS_SAMPLE + k] = s;
  }
}

// rows [nrows][NINT_ENS_SAMPLE]: SA, SD, SV, S2, S1, Sy, Syy of every (sample, output), added in ascending row order by one
// thread per sum; then the loss, the statistics of the ensemble mean and the ensemble sums (include/nint.h)
__global__ __launch_bounds__(64) void ens_loss_final_kernel(const double* __restrict__ rows, int nrows, double dM, double kp, double cnt,
                                                           float* __restrict__ loss_out, double* __restrict__ stats,
                                                           double* __restrict__ ens_out) {
#pragma clang fp contract(off)
  __shared__ double tot_s[NINT_ENS_SAMPLE];
  const int k = threadIdx.x;
  if (k < NINT_ENS_SAMPLE) {
    double s = 0.0;
#pragma unroll 8
    for (int r = 0; r < nrows; ++r) s += rows[(size_t)r * NINT_ENS_SAMPLE + k];
    tot_s[k] = s;
  }
  __syncthreads();
  if (k == 0) {
    const double SA = tot_s[0], SD = tot_s[1], SV = tot_s[2], S2 = tot_s[3], S1 = tot_s[4], Sy = tot_s[5], Syy = tot_s[6];
    const double loss = (SA / dM - kp * SD) / cnt;
    loss_out[0] = (float)loss;
    stats[0] += S2; stats[1] += S1; stats[2] += Sy; stats[3] += Syy; stats[4] += cnt;
    const double ss_tot = Syy - Sy * Sy / cnt;
    const double r2 = ss_tot > 0.0 ? 1.0 - S2 / ss_tot : (S2 == 0.0 ? 1.0 : 0.0);   // the loss entries' constant-target convention
    stats[5] += loss; stats[6] += r2; stats[7] += 1.0;
    ens_out[0] += SA; ens_out[1] += SD; ens_out[2] += SV; ens_out[3] += cnt;
  }
}

static inline size_t ens_loss_blocks(int H, int W) { return ((size_t)H * W + 255) / 256; }

// scratch: the workgroups' partial rows of one piece, then the (sample, output) rows of the whole call
extern "C" size_t nint_ens_loss_scratch_bytes(int N, int M, int O, int H, int W) {
  if (N <= 0 || M <= 0 || O <= 0 || H <= 0 || W <= 0) return 0;
  const size_t nc = N < NINT_ENS_MAX_N ? N : NINT_ENS_MAX_N;
  return (nc * O * ens_loss_blocks(H, W) + (size_t)N * O) * NINT_ENS_SAMPLE * sizeof(double);
}

extern "C" int nint_ens_loss(const float* pred, const int64_t* pred_off, int64_t pred_stride, float* dpred, const int64_t* dpred_off,
                             int64_t dpred_stride, int M, const float* y, const float* wgt, double wsum,
                             const nint_ens_loss_spec* spec, float* loss_out, double* stats, double* ens_out, double* scratch,
                             size_t scratch_bytes, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc, void* stream) {
  if (!pred || !pred_off || !dpred || !dpred_off || !y || !spec || !loss_out || !stats || !ens_out || !scratch) return NINT_E_ARG;
  if (M < 2 || M > NINT_ENS_MAX_M || N < 1 || O < 1 || pred_stride < 0 || dpred_stride < 0) return NINT_E_ARG;
  for (int n = 0; n < N; ++n)
    if (pred_off[n] < 0 || dpred_off[n] < 0) return NINT_E_ARG;
  if (!(spec->alpha >= 0.0) || !(spec->alpha <= 1.0)) return NINT_E_ARG;
  if (!(spec->cnt > 0.0) || spec->cnt > DBL_MAX) return NINT_E_ARG;
  if (wgt && (!(wsum > 0.0) || wsum > DBL_MAX)) return NINT_E_ARG;
  if (spec->ow) {
    if (spec->nrows < 1) return NINT_E_ARG;
    for (int n = 0; spec->ow_row && n < N; ++n)
      if (spec->ow_row[n] < 0 || spec->ow_row[n] >= spec->nrows) return NINT_E_ARG;
  } else if (spec->ow_row || spec->nrows != 0) {
    return NINT_E_ARG;
  }
  if (Hc < 1 || Wc < 1 || oy < 0 || ox < 0 || oy + Hc > H || ox + Wc > W) return NINT_E_ARG;
  if (scratch_bytes < nint_ens_loss_scratch_bytes(N, M, O, H, W)) return NINT_E_ARG;
  if (((((uintptr_t)stats) | ((uintptr_t)ens_out) | ((uintptr_t)scratch)) & 7) != 0) return NINT_E_ALIGN;
  if (((((uintptr_t)pred) | ((uintptr_t)dpred) | ((uintptr_t)y) | ((uintptr_t)wgt) | ((uintptr_t)spec->ow) | ((uintptr_t)loss_out)) & 3) != 0)
    return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const double dM = (double)M;
  const double kp = (dM - 1.0 + spec->alpha) / (dM * dM * (dM - 1.0));   // (M^2 (M - 1) <= 2^18: exact)
  const int NP = (int)ens_loss_blocks(H, W);
  const size_t HWc = (size_t)Hc * Wc;
  const size_t ncmax = N < NINT_ENS_MAX_N ? N : NINT_ENS_MAX_N;
  double* rows = scratch + ncmax * O * NP * NINT_ENS_SAMPLE;
  for (int c0 = 0; c0 < N; c0 += NINT_ENS_MAX_N) {                     // pieces of at most NINT_ENS_MAX_N samples
    const int nc = N - c0 < NINT_ENS_MAX_N ? N - c0 : NINT_ENS_MAX_N;
    EnsLossPlan plan = {};
    for (int i = 0; i < nc; ++i) {
      plan.poff[i] = pred_off[c0 + i];
      plan.doff[i] = dpred_off[c0 + i];
      plan.row[i] = spec->ow_row ? spec->ow_row[c0 + i] : 0;
    }
    const dim3 grid((unsigned)NP, (unsigned)nint_cdiv(O, ENS_OG), (unsigned)nc);
    hipLaunchKernelGGL(ens_loss_kernel, grid, dim3(256), (size_t)M * 256 * sizeof(float), st, pred, pred_stride, dpred, dpred_stride,
                       M, y + (size_t)c0 * O * HWc, wgt, spec->ow, kp, spec->cnt, scratch, plan, O, H, W, oy, ox, Hc, Wc);
    NINT_LAUNCH_CHECK();
    const int rc = nint_internal_skill_fold_enqueue(scratch, rows + (size_t)c0 * O * NINT_ENS_SAMPLE, nc * O, NP, st);
    if (rc != NINT_OK) return rc;
  }
  hipLaunchKernelGGL(ens_loss_final_kernel, dim3(1), dim3(64), 0, st, rows, N * O, dM, kp, spec->cnt, loss_out, stats, ens_out);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}
