// pointwise.hip -- the elementwise kernels: the LSTM pointwise backward (planned, then enqueued, like the conv launches)
// and flat Adam, with the gradient-norm guard in front of it (norm reduction, clip coefficient, skipped steps).  One-read/one-write
// streaming over flat index ranges.
#include "nint_common.h"

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
  nint_by_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL((lstm_bwd_pointwise_kernel<decltype(dt)::value>), grid1d(total), dim3(256), 0, (hipStream_t)stream, *a);
  });
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

// ------------------------------------------------------------------------------ Adam
// torch.optim.Adam single-tensor update order (train.py:71,110):
//   m = lerp(m, g, 1-b1) ; v = b2*v + (1-b2)*g*g ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// (one element update for the plain and the guarded kernel: the same operations in the same order, so the same roundings)
__device__ __forceinline__ void adam_flat_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, size_t i, float step_size, float w1, float b2, float w2,
                                                 float eps, float inv_sqrt_bc2_denom, float grad_scale) {
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

__global__ void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, size_t n, float step_size, float w1, float b2, float w2,
                                 float eps, float inv_sqrt_bc2_denom, float grad_scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    adam_flat_update(p, g, m, v, i, step_size, w1, b2, w2, eps, inv_sqrt_bc2_denom, grad_scale);
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

// ------------------------------------------------------------------------------ gradient norm, clipping, skipped steps
// The guard of the training step, decided on the device (nint.h has the arithmetic): S = sum g[i]^2 in f64 by the loss
// kernels' two-stage fixed-order reduction -- NINT_GRAD_NORM_BLOCKS workgroups whatever the device, each thread a fixed
// strided share of g, a tree in LDS, one workgroup folding the partials; no atomics, so S depends on (g, n) only.
// Dword loads: g needs no more than its natural alignment, and the share of a thread does not depend on the pointer.
#define GN_THREADS 1024
__global__ __launch_bounds__(GN_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, size_t n,
                                                                       double* __restrict__ partial) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  for (; i + 3 * stride < n; i += 4 * stride) {               // four independent loads in flight per thread
    const double x0 = g[i], x1 = g[i + stride], x2 = g[i + 2 * stride], x3 = g[i + 3 * stride];
    a0 += x0 * x0; a1 += x1 * x1; a2 += x2 * x2; a3 += x3 * x3;
  }
  for (; i < n; i += stride) {
    const double x = g[i];
    a0 += x * x;
  }
  __shared__ double red[GN_THREADS];
  red[threadIdx.x] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  for (int s = GN_THREADS >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one workgroup of NINT_GRAD_NORM_BLOCKS threads: the fixed-order tree over the partials; every thread returns S
__device__ __forceinline__ double grad_norm_fold(const double* __restrict__ partial, int nblocks) {
  __shared__ double red[NINT_GRAD_NORM_BLOCKS];
  red[threadIdx.x] = (int)threadIdx.x < nblocks ? partial[threadIdx.x] : 0.0;
  __syncthreads();
  for (int s = NINT_GRAD_NORM_BLOCKS >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(NINT_GRAD_NORM_BLOCKS) void grad_norm_final_kernel(const double* __restrict__ partial, int nblocks,
                                                                                float grad_scale, double* __restrict__ out) {
  const double S = grad_norm_fold(partial, nblocks);
  if (threadIdx.x == 0) {
    out[0] = S;
    out[1] = (double)grad_scale * sqrt(S);
  }
}

// the decisions of a guarded step and its counters, by ONE thread: state[0..15] as nint.h lists them; returns bc1 of step applied + 1
__device__ __forceinline__ double adam_guard_decide(double S, float grad_scale, double max_norm, int skip_nonfinite, double lr,
                                                    double beta1, double beta2, double* __restrict__ state) {
  const double gs = (double)grad_scale;
  const double norm = gs * sqrt(S);
  const bool finite = isfinite(S);
  double coef = 1.0;
  if (max_norm > 0.0) {
    const double c = max_norm / (norm + 1e-6);
    coef = c < 1.0 ? c : 1.0;                                 // (a NaN norm: 1)
  }
  const bool apply = finite || !skip_nonfinite;
  const double step = state[NINT_OPT_APPLIED] + 1.0;
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  state[NINT_OPT_APPLIED] += apply ? 1.0 : 0.0;
  state[NINT_OPT_SKIPPED] += apply ? 0.0 : 1.0;
  state[NINT_OPT_CLIPPED] += (finite && coef < 1.0) ? 1.0 : 0.0;
  state[NINT_OPT_CALLS] += 1.0;
  if (finite) {
    state[NINT_OPT_SUM_NORM] += norm;
    state[NINT_OPT_FINITE] += 1.0;
    if (norm > state[NINT_OPT_MAX_NORM]) state[NINT_OPT_MAX_NORM] = norm;
  }
  state[NINT_OPT_S] = S;
  state[NINT_OPT_NORM] = norm;
  state[NINT_OPT_COEF] = coef;
  state[NINT_OPT_SCALE] = (double)(float)(gs * coef);
  state[NINT_OPT_STEP_SIZE] = (double)(float)(lr / bc1);
  state[NINT_OPT_SQRT_BC2] = (double)(float)sqrt(bc2);
  state[NINT_OPT_APPLY] = apply ? 1.0 : 0.0;
  state[14] = 0.0;
  state[15] = 0.0;
  return bc1;
}

// the control kernel of nint_adam_flat_guarded: folds the partials, takes the step's decisions, keeps the counters
__global__ __launch_bounds__(NINT_GRAD_NORM_BLOCKS) void adam_guard_kernel(const double* __restrict__ partial, int nblocks,
                                                                           float grad_scale, double max_norm, int skip_nonfinite,
                                                                           double lr, double beta1, double beta2,
                                                                           double* __restrict__ state) {
  const double S = grad_norm_fold(partial, nblocks);
  if (threadIdx.x != 0) return;
  adam_guard_decide(S, grad_scale, max_norm, skip_nonfinite, lr, beta1, beta2, state);
}

// adam_flat_kernel with its step scalars read from `state` (f32 values held in doubles: the casts are exact)
__global__ void adam_flat_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                         float* __restrict__ v, size_t n, const double* __restrict__ state, float w1, float b2,
                                         float w2, float eps) {
  if (state[NINT_OPT_APPLY] == 0.0) return;                   // a skipped step: nothing is stored
  const float step_size = (float)state[NINT_OPT_STEP_SIZE], sqrt_bc2 = (float)state[NINT_OPT_SQRT_BC2];
  const float grad_scale = (float)state[NINT_OPT_SCALE];
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    adam_flat_update(p, g, m, v, i, step_size, w1, b2, w2, eps, sqrt_bc2, grad_scale);
}

extern "C" size_t nint_grad_norm_scratch_bytes(void) { return NINT_GRAD_NORM_BLOCKS * sizeof(double); }

// the partial-sum launch; *nblocks = the number of partials written (0 for n == 0: the fold then gives S = 0)
static int grad_norm_partials(const float* g, size_t n, double* scratch, hipStream_t st, int* nblocks) {
  *nblocks = 0;
  if (n == 0) return NINT_OK;
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(NINT_GRAD_NORM_BLOCKS), dim3(GN_THREADS), 0, st, g, n, scratch);
  NINT_LAUNCH_CHECK();
  *nblocks = NINT_GRAD_NORM_BLOCKS;
  return NINT_OK;
}

extern "C" int nint_grad_norm_flat(const float* g, size_t n, float grad_scale, double* out, double* scratch,
                                   size_t scratch_bytes, void* stream) {
  if (!g || !out || !scratch || scratch_bytes < nint_grad_norm_scratch_bytes()) return NINT_E_ARG;
  if (((((uintptr_t)out) | ((uintptr_t)scratch)) & 7) != 0) return NINT_E_ALIGN;
  int nblocks;
  const int rc = grad_norm_partials(g, n, scratch, (hipStream_t)stream, &nblocks);
  if (rc != NINT_OK) return rc;
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(NINT_GRAD_NORM_BLOCKS), 0, (hipStream_t)stream, scratch, nblocks,
                     grad_scale, out);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_adam_flat_guarded(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1,
                                      double beta2, double eps, float grad_scale, double max_norm, int skip_nonfinite,
                                      double* state, double* scratch, size_t scratch_bytes, void* stream) {
  if (!p || !g || !m || !v || !state || !scratch || scratch_bytes < nint_grad_norm_scratch_bytes()) return NINT_E_ARG;
  if (!(max_norm >= 0.0)) return NINT_E_ARG;                  // negative or NaN
  if (((((uintptr_t)state) | ((uintptr_t)scratch)) & 7) != 0) return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  int nblocks;
  const int rc = grad_norm_partials(g, n, scratch, st, &nblocks);
  if (rc != NINT_OK) return rc;
  hipLaunchKernelGGL(adam_guard_kernel, dim3(1), dim3(NINT_GRAD_NORM_BLOCKS), 0, st, scratch, nblocks, grad_scale, max_norm,
                     skip_nonfinite ? 1 : 0, lr, beta1, beta2, state);
  NINT_LAUNCH_CHECK();
  if (n == 0) return NINT_OK;
  hipLaunchKernelGGL(adam_flat_guarded_kernel, grid1d(n), dim3(256), 0, st, p, g, m, v, n, state, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)eps);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// ------------------------------------------------------------------------------ grouped AdamW (fine-tuning)
// Ranges of the flat buffer with a learning rate and a decoupled weight decay each (nint.h: nint_adam_flat_groups).  ONE launch:
// blockIdx.y is the group, its workgroups grid-stride over the group's range; the table travels by value.  Elements outside the
// groups' ranges are touched by no thread.
struct AdamGroups { unsigned long long begin[NINT_MAX_OPT_GROUPS], end[NINT_MAX_OPT_GROUPS]; float step_size[NINT_MAX_OPT_GROUPS], decay[NINT_MAX_OPT_GROUPS]; };
struct AdamGroupRates { double lr[NINT_MAX_OPT_GROUPS], wd[NINT_MAX_OPT_GROUPS]; int n; };

// torch.optim.AdamW's single-tensor order: the decoupled decay (one f32 multiply; 1.0f without decay: p as it was), then Adam's update
__device__ __forceinline__ void adamw_flat_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, size_t i, float decay, float step_size, float w1, float b2,
                                                  float w2, float eps, float sqrt_bc2, float grad_scale) {
  p[i] = __fmul_rn(p[i], decay);
  adam_flat_update(p, g, m, v, i, step_size, w1, b2, w2, eps, sqrt_bc2, grad_scale);
}

__global__ void adam_flat_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                        float* __restrict__ v, AdamGroups t, float w1, float b2, float w2, float eps,
                                        float sqrt_bc2, float grad_scale) {
  const int k = blockIdx.y;
  const size_t end = t.end[k];
  const float step_size = t.step_size[k], decay = t.decay[k];
  for (size_t i = t.begin[k] + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < end; i += (size_t)gridDim.x * blockDim.x)
    adamw_flat_update(p, g, m, v, i, decay, step_size, w1, b2, w2, eps, sqrt_bc2, grad_scale);
}

// nint_adam_flat_groups_guarded's control kernel: adam_guard_kernel's decisions (state[NINT_OPT_STEP_SIZE] from group 0's lr), then
// every group's step size and decay multiplier into gstate
__global__ __launch_bounds__(NINT_GRAD_NORM_BLOCKS) void adam_guard_groups_kernel(const double* __restrict__ partial, int nblocks,
                                                                                  float grad_scale, double max_norm,
                                                                                  int skip_nonfinite, AdamGroupRates r, double beta1,
                                                                                  double beta2, double* __restrict__ state,
                                                                                  double* __restrict__ gstate) {
  const double S = grad_norm_fold(partial, nblocks);
  if (threadIdx.x != 0) return;
  const double bc1 = adam_guard_decide(S, grad_scale, max_norm, skip_nonfinite, r.lr[0], beta1, beta2, state);
  for (int k = 0; k < r.n; ++k) {
    gstate[2 * k] = (double)(float)(r.lr[k] / bc1);
    gstate[2 * k + 1] = (double)(float)(1.0 - r.lr[k] * r.wd[k]);
  }
}

__global__ void adam_flat_groups_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, AdamGroups t, const double* __restrict__ state,
                                                const double* __restrict__ gstate, float w1, float b2, float w2, float eps) {
  if (state[NINT_OPT_APPLY] == 0.0) return;                   // a skipped step: nothing is stored
  const int k = blockIdx.y;
  const size_t end = t.end[k];
  const float step_size = (float)gstate[2 * k], decay = (float)gstate[2 * k + 1];
  const float sqrt_bc2 = (float)state[NINT_OPT_SQRT_BC2], grad_scale = (float)state[NINT_OPT_SCALE];
  for (size_t i = t.begin[k] + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < end; i += (size_t)gridDim.x * blockDim.x)
    adamw_flat_update(p, g, m, v, i, decay, step_size, w1, b2, w2, eps, sqrt_bc2, grad_scale);
}

// the table's checks (nint.h) and its device form; *longest = the longest group (the grid's x extent covers it)
static int adam_groups_table(const nint_opt_group* groups, int ngroups, AdamGroups* t, AdamGroupRates* r, size_t* longest) {
  if (!groups || ngroups < 1 || ngroups > NINT_MAX_OPT_GROUPS) return NINT_E_ARG;
  *t = AdamGroups{}; *r = AdamGroupRates{}; *longest = 0;
  for (int k = 0; k < ngroups; ++k) {
    const nint_opt_group& q = groups[k];
    if (q.end <= q.begin || (k > 0 && q.begin != groups[k - 1].end)) return NINT_E_ARG;        // empty, unsorted, a gap or an overlap
    if (!(q.lr >= 0.0 && q.lr < HUGE_VAL) || !(q.weight_decay >= 0.0 && q.weight_decay < HUGE_VAL)) return NINT_E_ARG;   // negative, NaN or inf
    t->begin[k] = q.begin; t->end[k] = q.end;
    r->lr[k] = q.lr; r->wd[k] = q.weight_decay;
    if (q.end - q.begin > *longest) *longest = (size_t)(q.end - q.begin);
  }
  r->n = ngroups;
  return NINT_OK;
}

extern "C" int nint_adam_flat_groups(float* p, const float* g, float* m, float* v, const nint_opt_group* groups, int ngroups,
                                     double beta1, double beta2, double eps, int step, float grad_scale, void* stream) {
  if (!p || !g || !m || !v || step < 1) return NINT_E_ARG;
  AdamGroups t; AdamGroupRates r; size_t longest;
  const int rc = adam_groups_table(groups, ngroups, &t, &r, &longest);
  if (rc != NINT_OK) return rc;
  const double bc1 = 1.0 - pow(beta1, step);                  // (nint_adam_flat's host expressions)
  const double bc2 = 1.0 - pow(beta2, step);
  for (int k = 0; k < ngroups; ++k) {
    t.step_size[k] = (float)(r.lr[k] / bc1);
    t.decay[k] = (float)(1.0 - r.lr[k] * r.wd[k]);
  }
  hipLaunchKernelGGL(adam_flat_groups_kernel, dim3(grid1d(longest).x, ngroups), dim3(256), 0, (hipStream_t)stream, p, g, m, v, t,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)sqrt(bc2), grad_scale);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_adam_flat_groups_guarded(float* p, const float* g, float* m, float* v, const nint_opt_group* groups,
                                             int ngroups, double beta1, double beta2, double eps, float grad_scale,
                                             double max_norm, int skip_nonfinite, double* state, double* gstate, double* scratch,
                                             size_t scratch_bytes, void* stream) {
  if (!p || !g || !m || !v || !state || !gstate || !scratch || scratch_bytes < nint_grad_norm_scratch_bytes()) return NINT_E_ARG;
  if (!(max_norm >= 0.0)) return NINT_E_ARG;                  // negative or NaN
  AdamGroups t; AdamGroupRates r; size_t longest;
  int rc = adam_groups_table(groups, ngroups, &t, &r, &longest);
  if (rc != NINT_OK) return rc;
  if (((((uintptr_t)state) | ((uintptr_t)gstate) | ((uintptr_t)scratch)) & 7) != 0) return NINT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const size_t begin = (size_t)groups[0].begin, n = (size_t)groups[ngroups - 1].end - begin;
  int nblocks;
  rc = grad_norm_partials(g + begin, n, scratch, st, &nblocks);          // the norm of the trained range only
  if (rc != NINT_OK) return rc;
  hipLaunchKernelGGL(adam_guard_groups_kernel, dim3(1), dim3(NINT_GRAD_NORM_BLOCKS), 0, st, scratch, nblocks, grad_scale, max_norm,
                     skip_nonfinite ? 1 : 0, r, beta1, beta2, state, gstate);
  NINT_LAUNCH_CHECK();
  hipLaunchKernelGGL(adam_flat_groups_guarded_kernel, dim3(grid1d(longest).x, ngroups), dim3(256), 0, st, p, g, m, v, t, state,
                     gstate, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}
