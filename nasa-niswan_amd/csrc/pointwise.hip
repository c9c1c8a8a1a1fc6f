// pointwise.hip -- the elementwise kernels: the LSTM pointwise backward (planned, then enqueued, like the conv launches)
// and flat Adam.  One-read/one-write streaming over flat index ranges.
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
