// seq.hip -- library entry points that are not kernels themselves: version / device info,
// the hardware self-test, and the whole-sequence drivers that plan every launch of a
// ConvLSTM forward (model.py:253-274) or of its backward pass -- the BPTT chain, then the layers'
// weight-gradient reductions and their fold -- as one list of steps and enqueue it from C++ on
// one HIP stream, so the Python side pays one ctypes call per pass instead of one per kernel.
#include <string.h>
#include <vector>
#include "nint_common.h"

extern "C" int nint_version(void) { return NINT_VERSION; }

extern "C" const char* nint_error_string(int code) {
  switch (code) {
    case NINT_OK: return "ok";
    case NINT_E_ARG: return "nint: invalid argument";
    case NINT_E_SHAPE: return "nint: shape not supported by any kernel instantiation";
    case NINT_E_LDS: return "nint: tile does not fit in LDS";
    case NINT_E_ALIGN: return "nint: pointer not 16-byte aligned";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "nint: unknown error";
  }
}

extern "C" int nint_device_info(int* n_cu, int* lds_bytes_per_cu, int* wave_size, char* name, int name_len) {
  int dev = 0;
  NINT_CHECK_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  NINT_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
  if (n_cu) *n_cu = prop.multiProcessorCount;
  if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
  if (wave_size) *wave_size = prop.warpSize;
  if (name && name_len > 0) {
    strncpy(name, prop.gcnArchName, name_len - 1);
    name[name_len - 1] = 0;
  }
  return NINT_OK;
}

extern "C" int nint_geom_make(nint_geom* g, int H, int W, int P) {
  if (!g || H <= 0 || W <= 0 || P < 0) return NINT_E_ARG;
  g->H = H; g->W = W; g->P = P;
  g->Hh = nint_round_up(H, 8) + 2 * P;
  g->Wh = nint_round_up(W, 32) + 2 * P;
  return NINT_OK;
}

// ------------------------------------------------------------------------------ self-test
// out[0..255]     : D of mfma_f32_16x16x32_bf16 with A[m][k] = m + 1 (k == 3 only), B[k][n] = 32 + n (k == 3 only),
//                   i.e. D[m][n] = (m+1)*(32+n) (asymmetric),
//                   stored as out[lane*4 + r]   -> pins the C/D register map and the A/B k-slot pairing
// out[1024..2047] : same for mfma_f32_16x16x4f32 with the one-hot k = 2
// out[2048..2303] : ds_read_b64_tr_b16 of an LDS image img[row][col] = 64*row + col (16 columns,
//                   32-byte rows), lane 4q+p of each 16-lane group addressing row 4*g+q, cols 4p..4p+3
//                   stored as out[2048 + lane*4 + e]
__global__ void selftest_kernel(float* out) {
  const int lane = threadIdx.x;
  const int g = lane >> 4, i16 = lane & 15;
  {
    bf16x8_t a, b;
    for (int j = 0; j < 8; ++j) {
      const int kk = 8 * g + j;
      a[j] = (__bf16)(kk == 3 ? (float)(i16 + 1) : 0.f);
      b[j] = (__bf16)(kk == 3 ? (float)(32 + i16) : 0.f);
    }
    f32x4_t c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[lane * 4 + r] = c[r];
  }
  {
    const float a = (g == 2) ? (float)(i16 + 1) : 0.f;
    const float b = (g == 2) ? (float)(32 + i16) : 0.f;
    f32x4_t c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[1024 + lane * 4 + r] = c[r];
  }
  {
    __shared__ __attribute__((aligned(16))) uint16_t img[16 * 16];
    for (int i = lane; i < 256; i += 64) img[i] = (uint16_t)(64 * (i / 16) + (i % 16));
    __syncthreads();
    const int q = i16 >> 2, p = i16 & 3;
    const char* ad = (const char*)img + (4 * g + q) * 32 + p * 8;
    s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)ad);
    for (int e = 0; e < 4; ++e) out[2048 + lane * 4 + e] = (float)(uint16_t)v[e];
  }
}

extern "C" int nint_selftest(float* out, void* stream) {
  if (!out) return NINT_E_ARG;
  hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

// ------------------------------------------------------------------------------ sequence drivers
// Every launch of a pass is enqueued from C++ on the CALLER's stream, in dependency order.  The library owns no streams, events
// or other state.  A (t, layer) wavefront on side streams and weight-gradient reductions overlapped with the BPTT chain were both at
// or below this order (co-resident MFMA-bound kernels evict each other's LDS / register budget); independent
// launches go out as ONE grid instead (nint_seq.wave; conv_lstm_multi_kernel and its kin).
static inline size_t esize(int dtype) { return dtype == NINT_BF16 ? 2 : 4; }

// In-step timing probe (nint_seq.probe): a one-thread launch that writes {tag, s_memrealtime} into the caller's buffer.
// Bracketing a launch with two of them costs two ordinary kernel boundaries (no event / barrier packets, which measured
// +8-10 us per bracketed launch); the back-to-back calibration pair at the start of each pass prices those boundaries.
struct Probe {
  unsigned long long* buf; int cap; int n; unsigned mask; hipStream_t st;
  void stamp(unsigned kind, int layer, int t, int end);                    // no-op unless bit `kind` of mask is set (kind 0: always)
};
__global__ void probe_stamp_kernel(unsigned long long* slot, unsigned long long tag) {
  if (threadIdx.x == 0) { slot[0] = tag; slot[1] = __builtin_amdgcn_s_memrealtime(); }
}
void Probe::stamp(unsigned kind, int layer, int t, int end) {
  if (!buf || n >= cap || (kind != NINT_PROBE_CAL && !((mask >> kind) & 1))) return;
  const unsigned long long tag = kind | ((unsigned long long)layer << 8) | ((unsigned long long)t << 16) | ((unsigned long long)end << 31) | (1ull << 63);
  hipLaunchKernelGGL(probe_stamp_kernel, dim3(1), dim3(64), 0, st, buf + 2 * (size_t)n, tag);
  ++n;
}
static Probe make_probe(const nint_seq* s, bool bwd, void* stream) {
  Probe p = {};
  if (s->probe && s->probe_mask && s->probe_slots >= 8) {
    const int half = s->probe_slots / 2;
    p.buf = s->probe + (bwd ? 2 * (size_t)half : 0);
    p.cap = half; p.mask = (unsigned)s->probe_mask; p.st = (hipStream_t)stream;
    p.stamp(NINT_PROBE_CAL, 0, 0, 0);          // two back-to-back stamps: the price of the brackets themselves
    p.stamp(NINT_PROBE_CAL, 0, 0, 1);
  }
  return p;
}

// ONE PASS VALUE: what a call of the eight entries is -- the window, what it feeds back (never NULL in here: NO_FB is the open
// loop), the direction and, roll-out only, where the head cotangents travel.  pass_check, plan_pass, run_pass.
enum { PASS_FWD, PASS_BWD, PASS_ROLLOUT };         // nint_seq_fwd[_closed] | nint_seq_bwd[_closed] | nint_seq_bwd_rollout
static const nint_feedback NO_FB = {};
// SCHEDULED SAMPLING: `mask` (T*B host bytes, or nullptr: "use fb->from") says per step and image what is fed.
// It is read here, on the host, while the pass is checked and planned; a launch gets its step's 64-bit word by value.
struct Pass {
  const nint_seq* s; const nint_feedback* fb; const nint_feedback_grad* rg; int dir; const uint8_t* mask;
  bool res;                                        // RESIDUAL HEAD: the feedback launches of the plan are the _res ones
  const nint_feedback_noise* fn;                   // NOISE ON THE FED-BACK VALUE (forward only), or nullptr: none
  bool bwd() const { return dir != PASS_FWD; }
  // the first step with a fed image (a mask; any non-zero byte counts, so that a bad byte is looked at), else fb->from
  int first() const {
    if (!mask) return fb->from;
    for (int t = 0; t < s->T; ++t) if (word_any(t)) return t;
    return s->T;
  }
  bool word_any(int t) const { for (int b = 0; b < s->B; ++b) if (mask[(size_t)t * s->B + b]) return true; return false; }
  unsigned long long word(int t) const {                             // (pass_check: B <= 64, bytes 0 / 1)
    unsigned long long m = 0;
    for (int b = 0; b < s->B && b < 64; ++b) if (mask[(size_t)t * s->B + b]) m |= 1ull << b;
    return m;
  }
  bool fed() const { return fb->O > 0 && first() < s->T; }           // steps [F, T) run time-major, fed images on the fed-back prediction
  bool rollout() const { return dir == PASS_ROLLOUT && fed(); }      // ... and this pass differentiates through it
};
static Pass pass_of(const nint_seq* s, const nint_feedback* fb, const nint_feedback_grad* rg, int dir, const nint_feedback_mask* fm = nullptr,
                    bool res = false, const nint_feedback_noise* fn = nullptr) {
  // (a mask beside a head of no outputs says nothing; s is checked before anything reads it: pass_check step 1 comes first)
  const bool masked = fm && fm->fed && fb && fb->O > 0 && s && s->B >= 1 && s->T >= 1;
  return Pass{s, fb ? fb : &NO_FB, dir == PASS_ROLLOUT ? rg : nullptr, dir, masked ? fm->fed : nullptr, res,
              dir == PASS_FWD && fn && fn->sigma ? fn : nullptr};
}

// THE ONE CHECK; its order decides the code of a doubly wrong call (tests/golden/seq_plan.npy.xz).  KEPT DIFFERENCE between the
// backward entries: nint_seq_bwd_rollout looks at the feedback only AFTER the backward fields (a misaligned dh_seq is
// NINT_E_ALIGN there, NINT_E_ARG with nint_seq_bwd_closed) and only where O < 0 or the window is fed: with O > 0 and from >= T
// (or O = 0 and from < 0) it accepts a head that nint_seq_bwd_closed refuses.
static int pass_check(const Pass& p) {
  const nint_seq* s = p.s; const nint_feedback* fb = p.fb;
  // 1. the window
  if (!s || s->L < 1 || s->L > NINT_MAX_LAYERS || s->B < 1 || s->T < 1) return NINT_E_ARG;
  if (s->dtype != NINT_F32 && s->dtype != NINT_BF16) return NINT_E_ARG;
  if (s->wave < 0 || s->wave > 5) return NINT_E_ARG;          // the modes of nint_seq.wave (nint.h); no other value is a mode
  if (!s->xs) return NINT_E_ARG;
  if (s->lon_cyclic != 0 && s->lon_cyclic != 1) return NINT_E_ARG;    // zero padding or cyclic longitude (nint.h); no other value is a mode
  if (s->lon_cyclic && s->g.W < s->g.P) return NINT_E_ARG;            // (a wrapped halo column must be an interior column)
  for (int l = 0; l < s->L; ++l) {
    if (!s->h[l] || !s->c[l]) return NINT_E_ARG;
    if (l > 0 && s->layer[l].Cxp != s->layer[l - 1].Chp) return NINT_E_ARG;
  }
  // 2. the feedback; step 0 can only be fed from a state that was handed in
  // A mask (4.21) takes the place of `from`, which is then not read: every byte 0 or 1, and F in the place of from.  Its one
  // NINT_E_SHAPE -- more images than the mask word has bits -- comes where the feedback has been found in order.
  bool mask_ok = true;
  for (size_t i = 0; p.mask && i < (size_t)s->T * s->B; ++i) mask_ok = mask_ok && p.mask[i] <= 1;
  const int F = p.mask ? p.first() : fb->from;
  const bool fb_ok = fb->O >= 0 && fb->O <= s->layer[0].Cx && mask_ok && F >= 0 && (fb->O == 0 || (fb->w && (F > 0 || s->has_init_state)));
  const int mask_rc = p.mask && s->B > 64 ? NINT_E_SHAPE : NINT_OK;
  if (p.dir != PASS_ROLLOUT && !fb_ok) return NINT_E_ARG;
  // (residual head, 4.22: the fed value of step 0 would need p_{-1}'s base; the roll-out refuses F == 0 anyway, below)
  if (p.res && p.dir == PASS_FWD && fb->O > 0 && F == 0) return NINT_E_ARG;
  if (!p.bwd()) return mask_rc;
  // 3. the backward fields
  const int f = s->train_from;         // (nint_seq.train_from: nothing of a layer below it is read)
  if (f < 0 || f > s->L || (f > 0 && (s->need_dx || s->bwd_parts != 0))) return NINT_E_ARG;
  for (int l = f; l < s->L; ++l)
    if (!s->gates[l] || !s->dG[l] || !s->dh[l] || !s->dc[l] || !s->dW[l] || !s->db[l]) return NINT_E_ARG;
  if ((s->need_dx && !s->dx) || (f < s->L && !s->wg_partial)) return NINT_E_ARG;
  if (s->fuse_bwd < 0 || (s->fuse_bwd > 2 && !(s->fuse_bwd & 0x40000000)) || s->bwd_parts < 0 || s->bwd_parts > 2) return NINT_E_ARG;
  if (s->accumulate != 0 && s->accumulate != 1) return NINT_E_ARG;     // stored or added (nint.h); no other value is a mode
  if ((((uintptr_t)s->dh_seq) & 15) != 0) return NINT_E_ALIGN;
  // 4. a fed window has no backward pass but the roll-out: d/dx of a fed step re-enters the top layer's d/dh of the step before,
  // which re-plans BPTT (BwdPlanner::feedback_bwd).  A window in which nothing is fed back trains as ever.
  if (p.dir != PASS_ROLLOUT) return p.fed() ? (int)NINT_E_ARG : mask_rc;
  if ((fb->O < 0 || p.fed()) && !fb_ok) return NINT_E_ARG;
  if (!p.fed()) return mask_rc;
  const nint_feedback_grad* rg = p.rg;          // (where the slab and the one-step scratch travel)
  if (F == 0 || f > 0 || s->bwd_parts != 0 || !rg || !rg->dpred || !s->dh_seq) return NINT_E_ARG;     // (F == 0: a fed image at step 0)
  if (!s->need_dx && !rg->dx_step) return NINT_E_ARG;
  if ((((uintptr_t)rg->dpred) & 3) != 0 || (((uintptr_t)(s->need_dx ? s->dx : rg->dx_step)) & 15) != 0) return NINT_E_ALIGN;
  return mask_rc;
}

// A pass is first PLANNED into an ordered list of steps -- host arithmetic only: nothing is enqueued, no stream is touched, no
// buffer is read -- and then the list is enqueued (run_steps).  nint_debug_seq_plan shows the same list to tests and tools.
enum { STEP_CONV, STEP_MULTI, STEP_PW, STEP_GATE, STEP_WGRAD, STEP_FOLD, STEP_WRAP, STEP_FEEDBACK, STEP_FEEDBACK_BWD };
struct SeqProb { int op, layer, t; };              // one conv / pointwise problem (NINT_OP_*)
struct GateCall { CellFwdJob job; nint_layer ly; int carrier; };
struct SeqStep {
  int kind;        // a planned conv launch | a merged grid | a pointwise backward | a direct nint_cell_fwd call (stencil / dense-K: no planned form)
                   // | one layer's weight-gradient reduction | the fold of a pass's reductions | a halo wrap / clear (cyclic longitude)
                   // | the feedback launch of a closed-loop step (tag_t = the step; no problems, n = 0)
                   // | its adjoint in the roll-out backward (tag_t = the fed step u; no problems, n = 0)
  int probe, tag_layer, tag_t;       // the NINT_PROBE_* kind and tag it is bracketed with
  int n; SeqProb prob[NINT_MULTI_MAX + 1];         // its problems, in grid order (a reduction / the fold: none, n = 0)
  union { ConvPlan conv; MultiPlan multi; PwArgs pw; GateCall gate; WgJobPlan wg; WgFoldPlan fold; WrapTable wrap; FbPlanNz fb; FbBwdPlan fbb; };
};
typedef std::vector<SeqStep> Steps;

static SeqStep& push(Steps& out, int kind, int probe, int tag_layer, int tag_t) {
  SeqStep& st = out.emplace_back();
  st.kind = kind; st.probe = probe; st.tag_layer = tag_layer; st.tag_t = tag_t;
  return st;
}
static void push_conv(Steps& out, const ConvPlan& pl, int probe, int op, int l, int t) {
  if (pl.gx <= 0) return;            // (e.g. time 0 of the bottom layer from a zero state without an input gradient: nothing to launch, nothing to bracket)
  SeqStep& st = push(out, STEP_CONV, probe, l, t);
  st.prob[st.n++] = SeqProb{op, l, t}; st.conv = pl;
}
static void push_pw(Steps& out, const PwArgs& pa, int l, int t) {
  SeqStep& st = push(out, STEP_PW, NINT_PROBE_POINTWISE, l, t);
  st.prob[st.n++] = SeqProb{NINT_OP_POINTWISE, l, t}; st.pw = pa;
}
// plans[0..n) (pw: and a pointwise backward) as ONE grid with the problems prob[0..np) -- where a merged kernel holds them; asked
// once, here, and the answer (kernel, argument block, grid) stays in the step.  false: nothing pushed, the caller plans them one by one
static bool push_grid(Steps& out, const ConvPlan* plans, int n, const PwArgs* pw, int probe, int tag_layer, int tag_t, const SeqProb* prob, int np) {
  SeqStep& st = push(out, STEP_MULTI, probe, tag_layer, tag_t);
  if (nint_internal_multi_plan(plans, n, pw, &st.multi) != NINT_OK) { out.pop_back(); return false; }
  for (; st.n < np; ++st.n) st.prob[st.n] = prob[st.n];
  return true;
}

static int run_steps(const nint_seq* s, const Steps& steps, Probe& probe, void* stream) {
  for (const SeqStep& st : steps) {
    probe.stamp(st.probe, st.tag_layer, st.tag_t, 0);
    int rc = NINT_E_ARG;
    switch (st.kind) {
      case STEP_CONV: rc = nint_internal_conv_enqueue(&st.conv, stream); break;
      case STEP_MULTI: rc = nint_internal_multi_enqueue(&st.multi, s->dtype, stream); break;
      case STEP_PW: rc = nint_internal_pointwise_enqueue(&st.pw, s->dtype, stream); break;
      case STEP_GATE: rc = nint_cell_fwd(&st.gate.ly, &s->g, s->dtype, s->B, st.gate.job.x_slab, st.gate.job.h_prev, st.gate.job.c_prev,
                                         st.gate.job.h_out, st.gate.job.c_out, st.gate.job.gates_out, stream); break;
      case STEP_WGRAD: rc = nint_internal_wgrad_enqueue(&st.wg, stream); break;
      case STEP_FOLD: rc = nint_internal_wgrad_fold_enqueue(&st.fold, stream); break;
      case STEP_WRAP: rc = nint_internal_wrap_enqueue(&st.wrap, stream); break;
      case STEP_FEEDBACK: rc = nint_internal_feedback_enqueue(&st.fb, stream); break;
      case STEP_FEEDBACK_BWD: rc = nint_internal_feedback_bwd_enqueue(&st.fbb, stream); break;
    }
    probe.stamp(st.probe, st.tag_layer, st.tag_t, 1);
    if (rc != NINT_OK) return rc;
  }
  return NINT_OK;
}

// gate(l, t): NINT_OK = *pl is its conv launch; NINT_E_SHAPE = no planned form (pl->gx == 0), *gc is the direct call
static int plan_gate(const nint_seq* s, int n_cu, bool rows8, int l, int t, GateCall* gc, ConvPlan* pl) {
  const nint_geom* g = &s->g;
  const size_t es = esize(s->dtype), halo_px = (size_t)g->Hh * g->Wh, comp_px = (size_t)g->H * g->W, B = s->B;
  gc->ly = s->layer[l];
  const nint_layer* ly = &gc->ly;
  // wave = 2 / 3 / 4: every gate launch of the pass on 8-row tiles -- the merged grids AND the lone launches at the ends of the
  // wavefront: the time-major order with tile_rows pinned to 8, bit for bit.  The first layer's 8-row tiles make the merged grid a
  // 256-register kernel at two workgroups per CU anyway, where the narrow layers' 4-row tiles lose what they were chosen for; 8-row
  // tiles halve their weight bytes per MFMA (B = 8: forward 2.85 -> 2.71 ms, profiles/r04_d_wave_rows8.txt).
  if (rows8 && ly->tile_rows == 0) gc->ly.tile_rows = 8;
  const size_t hs = (size_t)B * halo_px * ly->Chp * es, cs = (size_t)B * comp_px * ly->Chp;
  const bool zero_state = (t == 0 && !s->has_init_state);     // model.py:259-262: zeros -> skip the h half of K
  CellFwdJob& j = gc->job; j.ly = ly;
  j.x_slab = (l == 0) ? (const char*)s->xs + (size_t)t * B * halo_px * ly->Cxp * es                // x[:, t]  (model.py:266)
                      : (const char*)s->h[l - 1] + (size_t)(t + 1) * B * halo_px * ly->Cxp * es;   // h of the layer below (model.py:271)
  j.h_prev = zero_state ? nullptr : (const char*)s->h[l] + (size_t)t * hs; j.c_prev = zero_state ? nullptr : s->c[l] + (size_t)t * cs;
  j.h_out = (char*)s->h[l] + (size_t)(t + 1) * hs; j.c_out = s->c[l] + (size_t)(t + 1) * cs;
  j.gates_out = s->gates[l] ? (char*)s->gates[l] + (size_t)t * B * comp_px * 4 * ly->Ch16 * es : nullptr;
  const int rc = nint_internal_cell_fwd_plan(&j, g, s->dtype, s->B, n_cu, pl);
  gc->carrier = pl->carrier;
  return rc;
}

// ... pushed: its planned conv launch, or (no planned form) the direct nint_cell_fwd call
static void push_gate(Steps& out, const GateCall& gc, const ConvPlan& pl, int l, int t) {
  if (pl.gx > 0) { push_conv(out, pl, NINT_PROBE_GATE, NINT_OP_GATE, l, t); return; }
  SeqStep& st = push(out, STEP_GATE, NINT_PROBE_GATE, l, t);
  st.prob[st.n++] = SeqProb{NINT_OP_GATE, l, t}; st.gate = gc; st.gate.job.ly = nullptr;      // (run_steps passes the step's own copy)
}

// Steps [t0, t1) of the forward pass.  OPEN LOOP (f == nullptr), (t, layer) WAVEFRONT: step w runs gate(l, w - l) of every layer
// -- each needs gate(l-1, w-l) and gate(l, w-l-1), both of step w-1 -- as ONE grid (conv_lstm_multi[8]_kernel).  T + L - 1 launches
// instead of T * L; the same workgroups on the same data, so the results are those of the time-major order bit for bit.  Else:
// for t, for layer (model.py:265-267).  CLOSED LOOP (f): gate(0, t) needs gate(L-1, t-1) through the feedback, so
// nothing merges: feedback(t), gate(0, t) ... gate(L-1, t), each gate on the tile_rows the same `wave` gives it in the open-loop
// pass -- the pass is then that open-loop pass, bit for bit, over an input that already holds the fed values.
// UNDER A MASK (m) the feedback launch goes out only at steps with a fed image, as the masked instantiation with
// the step's word; the gates of the step are planned as in any closed-loop step.
// RESIDUAL HEAD (res): the same launch in the same place with its base in block t-1 of xs (pass_check: t >= 1).
// NOISE (fn): the same launch in the same place, drawing for step fn->step0 + t.
static int plan_fwd_steps(const nint_seq* s, const nint_feedback* f, int n_cu, int t0, int t1, Steps& out, const Pass* m = nullptr,
                          bool res = false, const nint_feedback_noise* fn = nullptr) {
  const int L = s->L, T = t1 - t0;
  const bool wavefront = !f && s->wave && L > 1 && L <= NINT_MULTI_MAX;
  const bool rows8 = (s->wave == 2 || s->wave == 3 || s->wave == 4) && L > 1 && L <= NINT_MULTI_MAX;     // the 8-row rule (plan_gate)
  for (int w = 0; w < (wavefront ? T + L - 1 : T * L); ++w) {
    GateCall gc[NINT_MULTI_MAX]; ConvPlan pl[NINT_MULTI_MAX]; SeqProb pr[NINT_MULTI_MAX];
    int n = 0; bool planned = true;
    for (int l = wavefront ? 0 : w % L; l < (wavefront ? L : w % L + 1); ++l) {
      const int t = t0 + (wavefront ? w - l : w / L);
      if (t < t0 || t >= t1) continue;
      const unsigned long long word = m ? m->word(t) : ~0ull;
      if (f && l == 0 && word) {                 // slab t of the top layer's h -> block t of xs
        const nint_layer* l0 = &s->layer[0];
        const nint_layer* top = &s->layer[L - 1];
        SeqStep& fb = push(out, STEP_FEEDBACK, NINT_PROBE_FEEDBACK, 0, t);
        const int rc = nint_internal_feedback_plan(s->h[L - 1], t * s->B, s->B, top->Ch, top->Chp, f->O, f->w, f->b, (void*)s->xs, t * s->B,
                                                   l0->Cx, l0->Cxp, l0->Cx - f->O, l0->xfold ? l0->k : 0, s->lon_cyclic, &s->g, s->dtype, &fb.fb);
        if (rc != NINT_OK) return rc;
        int rc2 = NINT_OK;
        if (m) { fb.fb.mask = word; fb.fb.sel = 1; }
        if (res && (rc2 = nint_internal_feedback_base(&fb.fb, s->xs, t * s->B, (t - 1) * s->B, s->B)) != NINT_OK) return rc2;
        if ((rc2 = nint_internal_feedback_noise(&fb.fb, fn, fn ? fn->step0 + (uint32_t)t : 0)) != NINT_OK) return rc2;     // (fn == nullptr: nz = 0, set here)
      }
      const int rc = plan_gate(s, n_cu, rows8, l, t, &gc[n], &pl[n]);
      if (rc != NINT_OK && rc != NINT_E_SHAPE) return rc;
      planned = planned && rc == NINT_OK;
      pr[n++] = SeqProb{NINT_OP_GATE, l, t};
    }
    if (n > 1 && planned && push_grid(out, pl, n, nullptr, NINT_PROBE_WAVE, n, w, pr, n)) continue;
    // (a single launch, or a shape the merged grid does not hold: one by one)
    for (int q = 0; q < n; ++q) push_gate(out, gc[q], pl[q], pr[q].layer, pr[q].t);
  }
  return NINT_OK;
}

// steps below F = min(max(from, 0), T) are the open-loop pass of F steps -- same merges, same rows8 pinning, same launches
static int plan_fwd(const Pass& p, int n_cu, Steps& out) {
  const int T = p.s->T, F = p.fed() ? p.first() : T;           // (pass_check: from >= 0)
  out.reserve((size_t)T * (p.s->L + 1));
  const int rc = plan_fwd_steps(p.s, nullptr, n_cu, 0, F, out);
  return rc != NINT_OK || F == T ? rc : plan_fwd_steps(p.s, p.fb, n_cu, F, T, out, p.mask ? &p : nullptr, p.res, p.fn);
}

// default of the "lower layer's pointwise backward on the fused layer's x columns" option: on (962.2 -> 963.6 samples/s, profiles/HISTORY.md)
#ifndef NINT_AUTO_LO
#define NINT_AUTO_LO true
#endif

// BPTT.  A layer runs either the CLASSIC step (pointwise backward of time u, then conv backward-data of time u) or the
// FUSED step X[u] = conv backward-data of time u with the pointwise backward of time u-1 in its epilogue
// (nint_cell_bwd_fused: d/dh_{u-1} never goes to memory).  Chosen per layer by the K-steps of its dgrad launch: inside the bench
// step fusing the 18-step top layer alone gives +0.7 ... +1.0 %, the 36-step layer -0.9 %, the 200-step layer -1.7 %.
// A fused layer consumes the x columns that the layer above produced for time u-1, so it runs ONE time step behind the
// layer above: at outer step so layer l works on time u_l = so + off_l, off_l = number of fused layers among l..L-1.
// Fused layer: u = T -> pointwise backward of T-1 alone (d/dh_{T-1} comes from the head / the caller),
// 1 <= u <= T-1 -> X[u], u = 0 -> plain conv backward-data of time 0.
struct BwdPlanner {
  const nint_seq* s; int n_cu; Steps& out;
  int L, T; size_t B, es, halo_px, comp_px;
  // ---- the schedule facts, computed once (the constructor)
  bool fused[NINT_MAX_LAYERS];
  // lo: the fused layer l also runs the pointwise backward of the classic layer below, on its x columns (the last contribution to
  // that layer's d/dh of the same time step): the layer below only launches its dgrad.  loc: a CLASSIC layer does the same for the
  // classic layer below it (its dgrad then runs the fused kernel with the h columns stored, on 4-row tiles)
  bool lo[NINT_MAX_LAYERS], loc[NINT_MAX_LAYERS];
  int off[NINT_MAX_LAYERS], pw_done[NINT_MAX_LAYERS];
  // (nint_seq.wave, include/nint.h)  merge, wave 1 / 3: the bottom layer's dgrad of one outer step and the top layer's fused step of
  // the next are ADJACENT launches that share no buffer in a stack of three or more layers: ONE grid; the bottom dgrad is held back
  // until the next launch is known.  merge_d, wave 4 / 5: it waits for the dgrad of layer 1 of the next time step instead, the wide
  // launch first.  Both produce a piece of the bottom layer's d/dh, so each stores its own -- layer 1 into dh[0], the bottom layer
  // into the head of the split-K scratch, idle until the weight gradients (dh0_own) -- and the bottom layer's pointwise backward
  // adds the two (f32: the sum of the time-major order bit for bit; bf16: each piece is rounded before the f32 add).  merge_p: ... and
  // that pointwise backward of time u waits for the top layer's fused step of time u-1, the next launch and independent of it
  // (layers >= 1 only): one grid, the fused step's workgroups first (the same arithmetic; profiles/r04_f_wave4.txt).
  bool merge, merge_d, merge_p;
  void* dh0_own;
  // ---- the two hold-back slots: a launch waits here until its partner, or a launch that conflicts with it, is planned
  bool has_d, has_p;
  ConvPlan held_d; int held_u;       // the bottom layer's dgrad of time held_u
  PwArgs held_p; int held_t;         // the bottom layer's pointwise backward of time held_t
  // ---- ROLL-OUT (nint_seq_bwd_rollout; rg == nullptr: none of it): steps u >= F were fed.  Layer 0's dgrad of a
  // fed step stores its x columns (without need_dx: into the one-step scratch) and the feedback backward launch follows it.
  // plan_bwd hands in a nint_seq with fuse_bwd = 1 and wave = 0: every launch by itself, time-major.
  // Under a mask (4.21) F is the first step with a fed image and the launch of EVERY step u >= F goes out, with the step's word:
  // an all-zero word makes it the plain head backward of block u-1, so the division of dh_seq between caller and chain stays.
  // Residual head (4.22): the launch of step u also adds dpred block u, which is final by then (`res`).
  const nint_feedback* fb; const nint_feedback_grad* rg; int F; const Pass* mp; bool res;

  BwdPlanner(const Pass& p, int n_cu_, Steps& out_)
      : s(p.s), n_cu(n_cu_), out(out_), L(p.s->L), T(p.s->T), B(p.s->B), has_d(false), has_p(false), held_u(0), held_t(0), fb(p.fb),
        rg(p.rollout() ? p.rg : nullptr), F(p.rollout() ? p.first() : p.s->T), mp(p.mask ? &p : nullptr), res(p.res) {
    es = esize(s->dtype); halo_px = (size_t)s->g.Hh * s->g.Wh; comp_px = (size_t)s->g.H * s->g.W;
    const bool explicit_mask = (s->fuse_bwd & 0x40000000) != 0;
    for (int l = L - 1; l >= 0; --l) {
      const nint_layer* ly = &s->layer[l];
      const int ksteps = (4 * ly->Ch16 / (s->dtype == NINT_BF16 ? 32 : 16)) * ly->k * ly->k;   // K-steps of the layer's dgrad launch
      fused[l] = explicit_mask ? ((s->fuse_bwd >> l) & 1) != 0 : (s->fuse_bwd == 2 || (s->fuse_bwd == 0 && ksteps <= 24));
      off[l] = (l == L - 1 ? 0 : off[l + 1]) + (fused[l] ? 1 : 0);
      pw_done[l] = -1;
    }
    for (int l = 0; l < L; ++l) {
      lo[l] = fused[l] && l > 0 && !fused[l - 1] && (explicit_mask ? ((s->fuse_bwd >> (8 + l)) & 1) != 0 : NINT_AUTO_LO);
      loc[l] = !fused[l] && l > 0 && !fused[l - 1] && explicit_mask && ((s->fuse_bwd >> (16 + l)) & 1) != 0;
    }
    merge = (s->wave == 1 || s->wave == 3) && L >= 3 && fused[L - 1] && !fused[0] && !loc[0];   // (wave == 2: the forward wavefront only)
    const size_t dh0_bytes = (size_t)B * comp_px * s->layer[0].Chp * es;
    merge_d = (s->wave == 4 || s->wave == 5) && L >= 2 && !fused[0] && !fused[1] && !loc[0] && !loc[1] && s->wg_partial_bytes >= dh0_bytes;
    merge_p = merge_d && L >= 3 && fused[L - 1];
    dh0_own = merge_d ? (void*)s->wg_partial : s->dh[0];
  }

  void flush_d() { if (has_d) push_conv(out, held_d, NINT_PROBE_DGRAD, NINT_OP_DGRAD, 0, held_u); has_d = false; }
  void flush_p() { if (has_p) push_pw(out, held_p, 0, held_t); has_p = false; }

  // nint_seq.dh_seq: the top layer's d/dh_t that does not come through the recurrence (the per-step head outputs), block t; nullptr: none
  const void* seq_block(int l, int t) const {
    return s->dh_seq && l == L - 1 ? (const char*)s->dh_seq + (size_t)t * B * comp_px * s->layer[l].Chp * es : nullptr;
  }

  // the pointwise backward of layer l: consumes dh[l] / dc[l] of time t (first BPTT step: not a dc flagged all-zero), writes dG of time t
  int pointwise(int l, int t, int so) {
    if (!merge_d || l == 0) flush_d();                         // (wave = 4 / 5: the held-back dgrad touches layer 0 only)
    const nint_layer* ly = &s->layer[l];
    const size_t cs = (size_t)B * comp_px * ly->Chp, Gc = 4 * (size_t)ly->Ch16;
    PwArgs pa;
    // d/dh_t: the recurrent part in dh[l], and a second piece -- the bottom layer's own h columns under merge_d (L >= 2), or the
    // top layer's block of dh_seq (never both: the bottom layer is the top one in a single-layer stack only).  At T-1 there is
    // no recurrent part: the block IS d/dh_{T-1}
    const void* blk = seq_block(l, t);
    const void* dh = blk && t == T - 1 ? blk : s->dh[l];
    const void* dh2 = merge_d && l == 0 && t < T - 1 ? dh0_own : (blk && t < T - 1 ? blk : nullptr);
    const int rc = nint_internal_pointwise_plan(ly, &s->g, s->dtype, B, (const char*)s->gates[l] + (size_t)t * B * comp_px * Gc * es,
                                                s->c[l] + (size_t)t * cs, s->c[l] + (size_t)(t + 1) * cs, dh, s->dc[l],
                                                (char*)s->dG[l] + (size_t)t * B * halo_px * Gc * es, t == T - 1 && ((s->zero_dstate >> (2 * l)) & 1),
                                                dh2, &pa);
    if (rc != NINT_OK) return rc;
    if (merge_p && l == 0 && so + off[L - 1] >= 2) { has_p = true; held_p = pa; held_t = t; }    // the next outer step opens with a fused step of the top layer
    else push_pw(out, pa, l, t);
    return NINT_OK;
  }

  // the pointwise backward of layer l - 1 at time u as a rider on layer l's launch
  void ride_lo(DgradPw& pw, int l, int u) {
    const nint_layer* lb = &s->layer[l - 1];
    const size_t cs_b = (size_t)B * comp_px * lb->Chp, Gc_b = 4 * (size_t)lb->Ch16;
    pw.lo_gates = (const char*)s->gates[l - 1] + (size_t)u * B * comp_px * Gc_b * es;
    pw.lo_c_prev = s->c[l - 1] + (size_t)u * cs_b; pw.lo_c_new = s->c[l - 1] + (size_t)(u + 1) * cs_b;
    pw.lo_dc = s->dc[l - 1]; pw.lo_dG_out = (char*)s->dG[l - 1] + (size_t)u * B * halo_px * Gc_b * es;
    pw.lo_Ch16 = lb->Ch16; pw.lo_dc_zero = u == T - 1 && ((s->zero_dstate >> (2 * (l - 1))) & 1);
    pw_done[l - 1] = u;
  }

  // layer l's conv backward-data of time u (pw: with a pointwise backward in its epilogue)
  int dgrad(int l, int u, const DgradPw* pw, ConvPlan* pl) {
    const nint_layer* ly = &s->layer[l];
    void* dx_dst = (l > 0) ? s->dh[l - 1] : (s->need_dx ? (void*)((char*)s->dx + (size_t)u * B * comp_px * ly->Cxp * es)
                                                        : (rg && u >= F ? rg->dx_step : nullptr));
    // the x columns go to the layer below's dh or this time step's dx slab: STORED where nothing else is there (dx; a dh flagged zero at the
    // first step; a FUSED layer below, whose dh buffer only ever carries them), else accumulated onto the h columns a classic layer below stored
    const bool ow = l == 0 ? true : (u == T - 1 ? (((s->zero_dstate >> (2 * (l - 1) + 1)) & 1) != 0) : (fused[l - 1] || (merge_d && l == 1)));
    // at time 0 with a zero initial state nobody consumes d/dh_{-1}; a fused step keeps the h columns in registers
    void* dh_prev = (u == 0 && !s->has_init_state) || (pw && pw->gates) ? nullptr
                  : (l == 0 && u > 0 ? dh0_own : s->dh[l]);    // (time 0: the caller reads d/dh_{-1} from dh[0])
    return nint_internal_conv_dgrad(ly, &s->g, s->dtype, B, (const char*)s->dG[l] + (size_t)u * B * halo_px * 4 * ly->Ch16 * es, dx_dst, dh_prev,
                                    ow, pw, n_cu, pl);
  }

  // the held-back bottom dgrad and `second` (layer l, time u) as one grid, where a merged kernel holds the two shapes
  bool pair(const ConvPlan& second, int op, int l, int u) {
    const ConvPlan pl[2] = {held_d, second};
    const SeqProb pr[2] = {{NINT_OP_DGRAD, 0, held_u}, {op, l, u}};
    if (!push_grid(out, pl, 2, nullptr, NINT_PROBE_BWD_PAIR, l, u, pr, 2)) return false;
    has_d = false;
    return true;
  }

  int classic(int l, int u, int so) {
    int rc = pw_done[l] != u ? pointwise(l, u, so) : (int)NINT_OK;    // (else: the layer above already ran this pointwise backward)
    if (rc != NINT_OK) return rc;
    DgradPw pw = {};
    if (loc[l]) { ride_lo(pw, l, u); pw.tile_rows = 4; }
    ConvPlan pl;
    rc = dgrad(l, u, loc[l] ? &pw : nullptr, &pl);
    if (rc != NINT_OK) return rc;
    if (merge_d && l == 1 && has_d && pair(pl, NINT_OP_DGRAD, l, u)) return NINT_OK;   // the bottom layer's dgrad of the step before + this one
    if (!merge_d || l <= 1) flush_d();
    // (held unless it is the very last launch: there is a step of a layer above to pair it with)
    if ((merge || merge_d) && l == 0 && so > -off[0]) { has_d = pl.gx > 0; held_d = pl; held_u = u; }
    else push_conv(out, pl, NINT_PROBE_DGRAD, NINT_OP_DGRAD, l, u);
    return NINT_OK;
  }

  int fused_step(int l, int u) {                               // X[u], 1 <= u <= T - 1
    const nint_layer* ly = &s->layer[l];
    const size_t cs = (size_t)B * comp_px * ly->Chp, Gc = 4 * (size_t)ly->Ch16;
    DgradPw pw = {};
    pw.gates = (const char*)s->gates[l] + (size_t)(u - 1) * B * comp_px * Gc * es; pw.c_prev = s->c[l] + (size_t)(u - 1) * cs;
    pw.c_new = s->c[l] + (size_t)u * cs; pw.dc = s->dc[l]; pw.old = l < L - 1 ? s->dh[l] : seq_block(l, u - 1);
    pw.dG_out = (char*)s->dG[l] + (size_t)(u - 1) * B * halo_px * Gc * es;
    if (lo[l]) ride_lo(pw, l, u);
    const bool top_pair = merge && has_d && l == L - 1;        // the top layer's step right behind the held-back bottom dgrad
    if (top_pair && s->wave == 3) pw.tile_rows = 8;            // (experiment: the fused step on 8-row tiles inside the two-workgroups-per-CU grid)
    ConvPlan pl;
    const int rc = dgrad(l, u, &pw, &pl);
    if (rc != NINT_OK) return rc;
    if (top_pair && pair(pl, NINT_OP_FUSED, l, u)) return NINT_OK;
    if (!merge_d) flush_d();
    const SeqProb pr[2] = {{NINT_OP_FUSED, l, u}, {NINT_OP_POINTWISE, 0, held_t}};
    // this step and the bottom layer's pointwise backward of the step before: one grid
    if (has_p && push_grid(out, &pl, 1, &held_p, NINT_PROBE_BWD_PW, l, u, pr, 2)) { has_p = false; return NINT_OK; }
    flush_p();
    push_conv(out, pl, NINT_PROBE_FUSED, NINT_OP_FUSED, l, u);
    return NINT_OK;
  }

  // weight / bias gradients: ONE reduction over all T time steps per layer and source (bracketed with q, its index among the
  // reductions of this call), all layers' folds merged
  int wgrads() {
    WgJob jobs[NINT_MAX_LAYERS];
    for (int l = 0; l < L; ++l) {
      const nint_layer* ly = &s->layer[l];
      const char* x_all = (l == 0) ? (const char*)s->xs : (const char*)s->h[l - 1] + B * halo_px * ly->Cxp * es;  // h^{l-1}_t = slab t+1
      // h_{-1} = 0 for a sequence from the zero state: the h part of the reduction skips time step 0
      jobs[l] = WgJob{ly, T * (int)B, s->dG[l], x_all, s->h[l] /* h_{t-1} = slab t */, s->dW[l], s->db[l], s->has_init_state ? 0 : (int)B};
    }
    // (bwd_parts: layers >= 1 in the first call, layer 0 in the second; each call folds what it reduced)
    const int j0 = s->bwd_parts == 1 ? 1 : 0, j1 = s->bwd_parts == 2 ? 1 : L;
    if (j1 <= j0) return NINT_OK;
    WgJobPlan jp[NINT_MAX_LAYERS]; WgFoldPlan fold;
    const int rc = nint_internal_wgrad_plan(jobs + j0, j1 - j0, &s->g, s->dtype, s->wg_partial, s->wg_partial_bytes, s->n_cu, jp, &fold);
    if (rc != NINT_OK) return rc;
    fold.t.acc = s->accumulate;                  // the fold's one write per element stores or adds (nint_seq.accumulate)
    for (int q = 0; q < j1 - j0; ++q) push(out, STEP_WGRAD, NINT_PROBE_WGRAD, q, 0).wg = jp[q];
    push(out, STEP_FOLD, NINT_PROBE_FOLD, 0, 0).fold = fold;
    return NINT_OK;
  }

  // behind layer 0's dgrad of a fed step u: dpred images of step u-1 += xi_u, dh_seq block u-1 = W^T g_{u-1}
  int feedback_bwd(int u) {
    const nint_layer* l0 = &s->layer[0];
    const nint_layer* top = &s->layer[L - 1];
    SeqStep& st = push(out, STEP_FEEDBACK_BWD, NINT_PROBE_FEEDBACK_BWD, 0, u);
    const int rc = nint_internal_feedback_bwd_plan(s->need_dx ? s->dx : rg->dx_step, s->need_dx ? u * (int)B : 0, rg->dpred, (u - 1) * (int)B,
                                                   (void*)s->dh_seq, (u - 1) * (int)B, (int)B, top->Ch, top->Chp, fb->O, fb->w, l0->Cx, l0->Cxp,
                                                   l0->Cx - fb->O, l0->xfold ? l0->k : 0, s->lon_cyclic, &s->g, s->dtype, &st.fbb);
    if (mp) { st.fbb.mask = mp->word(u); st.fbb.sel = 1; }       // (the plan function zero-fills both: after it)
    if (res) { st.fbb.pnext = rg->dpred + (size_t)u * B * fb->O * comp_px; st.fbb.res = 1; }
    return rc;
  }

  int plan() {
    out.reserve((size_t)(T + L) * L * 2 + L + 1 + (size_t)(T - F));
    for (int so = T - 1; so >= -off[0] && s->bwd_parts != 2; --so) {      // (part 2: the chain ran in the part-1 call)
      for (int l = L - 1; l >= 0; --l) {
        const int u = so + off[l];
        if (u < 0 || u > (fused[l] ? T : T - 1)) continue;
        if (!(l == L - 1 && u >= 1 && u < T)) flush_p();       // (anything but the fused step it waits for)
        int rc = NINT_OK;
        if (!fused[l]) rc = classic(l, u, so);
        else if (u == T) rc = pointwise(l, T - 1, so);
        else if (u >= 1) rc = fused_step(l, u);
        else {                                                 // a fused layer's time 0: plain conv backward-data
          if (!merge_d) flush_d();
          ConvPlan pl;
          if ((rc = dgrad(l, 0, nullptr, &pl)) == NINT_OK) push_conv(out, pl, NINT_PROBE_DGRAD, NINT_OP_DGRAD, l, 0);
        }
        if (rc != NINT_OK) return rc;
        if (rg && l == 0 && u >= F && (rc = feedback_bwd(u)) != NINT_OK) return rc;
      }
    }
    flush_p(); flush_d();
    return wgrads();
  }
};

// nint_seq.train_from = f > 0: the backward pass of (s, f) IS the backward pass of the stack of layers f .. L-1, fed by h[f-1] from
// image B on (h^{f-1}_t = slab t+1, as BwdPlanner::wgrads reads it), with no input gradient.  This is that stack as a nint_seq of its
// own -- a shifted view of the caller's pointers -- which the one planner takes: its "bottom layer" (the wave merges, the x columns
// nobody wants, the head of wg_partial) is layer f.
static nint_seq sub_stack(const nint_seq* s, int f) {
  nint_seq v = *s;
  const int L = s->L - f;
  v.train_from = 0; v.L = L; v.need_dx = 0; v.dx = nullptr;
  v.zero_dstate = (int32_t)((uint32_t)s->zero_dstate >> (2 * f));
  if (s->fuse_bwd & 0x40000000) {                // explicit masks: each of the three byte-wide fields moves down by f layers
    const uint32_t m = (uint32_t)s->fuse_bwd;
    v.fuse_bwd = (int32_t)(0x40000000u | ((m & 0xffu) >> f) | ((((m >> 8) & 0xffu) >> f) << 8) | ((((m >> 16) & 0xffu) >> f) << 16));
  }
  v.xs = (const char*)s->h[f - 1] + (size_t)s->B * s->g.Hh * s->g.Wh * s->layer[f].Cxp * esize(s->dtype);
  for (int l = 0; l < NINT_MAX_LAYERS; ++l) {
    const int q = l + f;
    const bool in = l < L;
    v.layer[l] = in ? s->layer[q] : nint_layer{};
    v.h[l] = in ? s->h[q] : nullptr; v.c[l] = in ? s->c[q] : nullptr; v.gates[l] = in ? s->gates[q] : nullptr;
    v.dG[l] = in ? s->dG[q] : nullptr; v.dh[l] = in ? s->dh[q] : nullptr; v.dc[l] = in ? s->dc[q] : nullptr;
    v.dW[l] = in ? s->dW[q] : nullptr; v.db[l] = in ? s->db[q] : nullptr;
  }
  return v;
}

// CYCLIC LONGITUDE (nint_seq.lon_cyclic): a pass over the FINISHED plan -- the planners above know nothing of it --
// that puts halo wrap launches between its steps.  Steps go out in list order on one stream, so "right behind its writer" holds
// for every schedule: a halo slab image is wrapped behind the step that wrote its interior and before any later step reads it.
//   forward  head: xs (all T*B images, unless folded: the fold wraps by itself) and slot 0 of every h of a given initial state;
//            behind the feedback launch of a closed-loop step t: block t of xs (unless folded), whose interior it wrote;
//            behind every step with a gate problem (l, t): block t+1 of h[l] -- one launch for all of a step's problems.
//   BPTT     behind the writer of a dG block -- a pointwise backward (l, t): dG[l] block t; a fused step X[u] of layer l: dG[l]
//            block u-1; a dgrad / fused step (l, u) with the lower layer's pointwise backward as its rider: dG[l-1] block u --
//            WRAP, where a dgrad of the plan reads that block (time 0 of a bottom layer nobody wants d/dx of has none);
//            behind the step with the dgrad / fused step (l, u), which read dG[l] block u: CLEAR, because the weight gradient
//            walks roundup(W, 32) columns and the right-hand wrapped columns lie in that slack: left wrapped they would be
//            summed into dW and db a second time.  After the chain every dG image has zero halos again.
// h and xs stay wrapped: the weight gradient reads its taps from them, and their slack pixels meet dG = 0.
struct WrapList {
  Steps& out; const nint_geom& g; WrapTable t;
  WrapList(Steps& out_, const nint_geom& g_) : out(out_), g(g_) { t = WrapTable{}; }
  void add(void* base, size_t nimg, size_t px_bytes, int op) {
    if (t.n == NINT_WRAP_MAX_JOBS) flush();
    t.job[t.n++] = WrapJob{(char*)base, (int)nimg, (int)px_bytes, op};
  }
  void flush() {
    if (t.n == 0) return;
    t.H = g.H; t.W = g.W; t.P = g.P; t.Hh = g.Hh; t.Wh = g.Wh;
    push(out, STEP_WRAP, NINT_PROBE_WRAP, t.n, 0).wrap = t;
    t = WrapTable{};
  }
};

static int add_wrap_steps(const nint_seq* s, bool bwd, Steps& steps) {
  if (s->g.P < 1) return NINT_OK;                // 1 x 1 kernels only: no halo, nothing to wrap
  const size_t es = esize(s->dtype), halo_px = (size_t)s->g.Hh * s->g.Wh, B = s->B;
  const int L = s->L, T = s->T;
  Steps out;
  out.reserve(2 * steps.size() + 1);
  WrapList w(out, s->g);
  auto h_px = [&](int l) { return (size_t)s->layer[l].Chp * es; };
  auto dG_px = [&](int l) { return 4 * (size_t)s->layer[l].Ch16 * es; };
  auto dG_blk = [&](int l, int t) { return (char*)s->dG[l] + (size_t)t * B * halo_px * dG_px(l); };
  std::vector<char> read(bwd ? (size_t)L * T : 0, 0);       // dG[l] block t has a dgrad in the plan
  if (bwd) {
    for (const SeqStep& st : steps)
      for (int q = 0; q < st.n; ++q)
        if (st.prob[q].op == NINT_OP_DGRAD || st.prob[q].op == NINT_OP_FUSED) read[(size_t)st.prob[q].layer * T + st.prob[q].t] = 1;
  } else {
    if (!s->layer[0].xfold) w.add((void*)s->xs, (size_t)T * B, (size_t)s->layer[0].Cxp * es, NINT_WRAP_COPY);
    for (int l = 0; l < L && s->has_init_state; ++l) w.add(s->h[l], B, h_px(l), NINT_WRAP_COPY);
    w.flush();
  }
  auto wrap_dG = [&](int l, int t) { if (read[(size_t)l * T + t]) w.add(dG_blk(l, t), B, dG_px(l), NINT_WRAP_COPY); };
  for (const SeqStep& st : steps) {
    out.push_back(st);
    // closed loop: the feedback of step t wrote the interior of xs block t (a folded xs wraps by itself)
    if (st.kind == STEP_FEEDBACK && !s->layer[0].xfold)
      w.add((char*)s->xs + (size_t)st.tag_t * B * halo_px * s->layer[0].Cxp * es, B, (size_t)s->layer[0].Cxp * es, NINT_WRAP_COPY);
    for (int q = 0; q < st.n; ++q) {
      const int op = st.prob[q].op, l = st.prob[q].layer, t = st.prob[q].t;
      if (!bwd) {
        if (op == NINT_OP_GATE) w.add((char*)s->h[l] + (size_t)(t + 1) * B * halo_px * h_px(l), B, h_px(l), NINT_WRAP_COPY);
        continue;
      }
      if (op == NINT_OP_POINTWISE) { wrap_dG(l, t); continue; }
      // a dgrad, alone or with pointwise backward passes in its epilogue: it has read its own block ...
      const ConvArgs& a = st.kind == STEP_MULTI ? st.multi.m.a[q] : st.conv.a;
      w.add(dG_blk(l, t), B, dG_px(l), NINT_WRAP_CLEAR);
      if (op == NINT_OP_FUSED) wrap_dG(l, t - 1);            // ... X[u] wrote block u-1 of its layer,
      if (a.lo_dG) wrap_dG(l - 1, t);                         // ... and its rider block u of the layer below
    }
    w.flush();
  }
  for (const SeqStep& st : out)
    if (st.kind == STEP_WRAP) { const int rc = nint_internal_wrap_check(&st.wrap); if (rc != NINT_OK) return rc; }
  steps.swap(out);
  return NINT_OK;
}

// The backward plan: the one BwdPlanner over the caller's nint_seq or a view of it (frozen layers: sub_stack).  A ROLL-OUT (4.19):
// xi_u exists only after layer 0's dgrad of step u and the top layer's pointwise backward of step u-1 needs it, so fuse_bwd = 1, wave = 0.
static int plan_bwd(const Pass& p, int n_cu, Steps& steps) {
  const nint_seq* s = p.s;
  const int f = s->train_from;
  if (f == s->L) return NINT_OK;                 // every layer frozen: nothing to plan
  nint_seq v;                                    // (the plan keeps no pointer into it)
  Pass q = p;
  if (p.rollout()) { v = *s; v.fuse_bwd = 1; v.wave = 0; q.s = &v; }       // (pass_check: f == 0)
  else if (f > 0) { v = sub_stack(s, f); q.s = &v; }
  const int rc = BwdPlanner(q, n_cu, steps).plan();
  for (SeqStep& st : steps) {                    // the records and probe tags carry the real layer index
    for (int i = 0; i < st.n; ++i) st.prob[i].layer += f;
    if (st.kind == STEP_CONV || st.kind == STEP_MULTI || st.kind == STEP_PW) st.tag_layer += f;
  }
  return rc;
}

// THE ONE FUNNEL: check, plan (the CU count the launch-shape rules read is looked up once per pass; cyclic longitude: the wrap
// launches go in between) and, run_pass, enqueue.
static int plan_pass(const Pass& p, Steps& steps) {
  int rc = pass_check(p);
  if (rc != NINT_OK) return rc;
  const int n_cu = nint_internal_n_cu();
  rc = p.bwd() ? plan_bwd(p, n_cu, steps) : plan_fwd(p, n_cu, steps);
  return rc == NINT_OK && p.s->lon_cyclic ? add_wrap_steps(p.s, p.bwd(), steps) : rc;
}

static int run_pass(const Pass& p, void* stream) {
  Steps steps;
  const int rc = plan_pass(p, steps);
  if (rc != NINT_OK) return rc;
  Probe probe = make_probe(p.s, p.bwd(), stream);
  return run_steps(p.s, steps, probe, stream);
}
extern "C" int nint_seq_fwd(const nint_seq* s, void* stream) { return run_pass(pass_of(s, nullptr, nullptr, PASS_FWD), stream); }
extern "C" int nint_seq_bwd(const nint_seq* s, void* stream) { return run_pass(pass_of(s, nullptr, nullptr, PASS_BWD), stream); }
extern "C" int nint_seq_fwd_closed(const nint_seq* s, const nint_feedback* fb, void* stream) { return run_pass(pass_of(s, fb, nullptr, PASS_FWD), stream); }
extern "C" int nint_seq_bwd_closed(const nint_seq* s, const nint_feedback* fb, void* stream) { return run_pass(pass_of(s, fb, nullptr, PASS_BWD), stream); }
extern "C" int nint_seq_bwd_rollout(const nint_seq* s, const nint_feedback* fb, const nint_feedback_grad* rg, void* stream) { return run_pass(pass_of(s, fb, rg, PASS_ROLLOUT), stream); }
extern "C" int nint_seq_fwd_sampled(const nint_seq* s, const nint_feedback* fb, const nint_feedback_mask* fm, void* stream) { return run_pass(pass_of(s, fb, nullptr, PASS_FWD, fm), stream); }
extern "C" int nint_seq_bwd_rollout_sampled(const nint_seq* s, const nint_feedback* fb, const nint_feedback_mask* fm, const nint_feedback_grad* rg, void* stream) { return run_pass(pass_of(s, fb, rg, PASS_ROLLOUT, fm), stream); }
extern "C" int nint_seq_fwd_residual(const nint_seq* s, const nint_feedback* fb, const nint_feedback_mask* fm, void* stream) { return run_pass(pass_of(s, fb, nullptr, PASS_FWD, fm, true), stream); }
extern "C" int nint_seq_fwd_stochastic(const nint_seq* s, const nint_feedback* fb, const nint_feedback_mask* fm, int residual, const nint_feedback_noise* fn, void* stream) {
  if (residual != 0 && residual != 1) return NINT_E_ARG;
  return run_pass(pass_of(s, fb, nullptr, PASS_FWD, fm, residual == 1, fn), stream);
}
extern "C" int nint_seq_bwd_rollout_residual(const nint_seq* s, const nint_feedback* fb, const nint_feedback_mask* fm, const nint_feedback_grad* rg, void* stream) { return run_pass(pass_of(s, fb, rg, PASS_ROLLOUT, fm, true), stream); }

// ------------------------------------------------------------------------------ the plan, for tests and tools
static int plan_records(const nint_seq* s, const Steps& steps, int bwd, nint_launch_rec* out, int cap) {
  if (cap > 0 && !out) return NINT_E_ARG;
  int n = 0;
  for (size_t i = 0; i < steps.size(); ++i) {
    const SeqStep& st = steps[i];
    for (int q = 0; q < st.n; ++q, ++n) {
      if (n >= cap) continue;
      nint_launch_rec r = {};
      r.index = (int)i; r.bwd = bwd ? 1 : 0; r.op = st.prob[q].op; r.layer = st.prob[q].layer; r.t = st.prob[q].t; r.dtype = s->dtype;
      r.kernel = st.kind == STEP_CONV ? (int)NINT_K_CONV_IGEMM : st.kind == STEP_MULTI ? st.multi.carrier
               : st.kind == STEP_PW ? (int)NINT_K_POINTWISE : st.gate.carrier;
      const bool in_grid = st.kind == STEP_MULTI && q < st.multi.m.n;      // (else a merged grid's pointwise problem: no body)
      if (st.kind == STEP_CONV || in_grid) {
        const ConvArgs& a = in_grid ? st.multi.m.a[q] : st.conv.a;
        const int v = in_grid ? st.multi.m.variant[q] : st.conv.variant;
        const ConvShape sh = conv_shape(v);
        r.epi = sh.epi; r.wn = sh.wn; r.wk = sh.wk; r.ntw = sh.ntw; r.mt = sh.mt;
        r.strip = a.tiles_x2 > 0; r.nt_begin = a.nt_begin;
        r.gx = in_grid ? st.multi.m.nbx[q] : st.conv.gx; r.gy = in_grid ? st.multi.m.nwg[q] / st.multi.m.nbx[q] : st.conv.gy;
      }
      out[n] = r;
    }
  }
  return n;
}

static int show_pass(const Pass& p, nint_launch_rec* out, int cap) {
  Steps steps;
  const int rc = plan_pass(p, steps);
  return rc != NINT_OK ? rc : plan_records(p.s, steps, p.bwd(), out, cap);
}
extern "C" int nint_debug_seq_plan(const nint_seq* s, int bwd, nint_launch_rec* out, int cap) { return show_pass(pass_of(s, nullptr, nullptr, bwd ? PASS_BWD : PASS_FWD), out, cap); }
extern "C" int nint_debug_seq_plan_closed(const nint_seq* s, const nint_feedback* fb, int bwd, nint_launch_rec* out, int cap) { return show_pass(pass_of(s, fb, nullptr, bwd ? PASS_BWD : PASS_FWD), out, cap); }
extern "C" int nint_debug_seq_plan_rollout(const nint_seq* s, const nint_feedback* fb, nint_launch_rec* out, int cap) {
  // made-up, aligned, non-NULL: the plan reads no pointer (a NULL dh_seq or dx is still the caller's, and refused)
  const nint_feedback_grad rg = {(float*)(uintptr_t)64, (void*)(uintptr_t)64};
  return show_pass(pass_of(s, fb, &rg, PASS_ROLLOUT), out, cap);
}
extern "C" int nint_debug_seq_plan_sampled(const nint_seq* s, const nint_feedback* fb, const nint_feedback_mask* fm, int dir, nint_launch_rec* out, int cap) {
  if (dir != PASS_FWD && dir != PASS_BWD && dir != PASS_ROLLOUT) return NINT_E_ARG;
  const nint_feedback_grad rg = {(float*)(uintptr_t)64, (void*)(uintptr_t)64};       // (made up, as in nint_debug_seq_plan_rollout)
  return show_pass(pass_of(s, fb, &rg, dir, fm), out, cap);
}
