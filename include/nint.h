/*
 * nint.h -- C ABI of the MI355X-native ConvLSTM hot path for Smart-NINT (nasa-niswan).
 *
 * The reference (smhassanerfani/nasa-niswan) has NO native/FFI interface: its boundary for
 * this path is the Python surface `model.py:ConvLSTMCell/ConvLSTM` + the `train.py` batch
 * step.  This header is the boundary the drop-in Python modules in `nasa-niswan_amd/` bind
 * with ctypes; every entry point cites the reference lines whose ATen op sequence it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer is a DEVICE pointer unless the parameter says "host".
 *   - every entry takes an explicit `stream` (hipStream_t as void*) and never synchronises.
 *   - every entry returns 0 on success, a negative NINT_E_* code for bad arguments or a
 *     positive hipError_t value; nothing throws or aborts.
 *   - the caller owns all memory (the Python side allocates through torch's caching
 *     allocator); the library keeps no state between calls, reads no environment variables and owns
 *     no streams or events: every launch goes to the caller's stream.
 *
 * Internal data layout ("slabs"), chosen for gfx950 rather than inherited from NCHW:
 *   halo slab     ET [N][Hh][Wh][Cp]   channels-last, ET = float or bf16, physical zero halo P
 *                                      on every side plus zero slack up to a multiple of 8 rows /
 *                                      32 columns, Cp = channels rounded up to KC (16 f32 / 32 bf16)
 *   compact slab  [N][H][W][Cp]        channels-last, no halo: f32 for the cell state c and dc, ET for the
 *                                      transient gradients dh, dx (written once, read once per BPTT step)
 *   gate stash    ET [N][H][W][Gc]     Gc = 4*Ch16, column n' = (cblock*4 + gate)*16 + col
 *   image index   n = t*B + b          (time-major so that one launch can span all T)
 */
#ifndef NINT_H
#define NINT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NINT_VERSION 113

enum { NINT_F32 = 0, NINT_BF16 = 1 };

enum {
  NINT_OK = 0,
  NINT_E_ARG = -1,      /* inconsistent / unsupported argument */
  NINT_E_SHAPE = -2,    /* shape not supported by any kernel instantiation */
  NINT_E_LDS = -3,      /* tile does not fit in the 160 KiB LDS */
  NINT_E_ALIGN = -4     /* pointer not 16-byte aligned */
};

/* Spatial geometry shared by all slabs of one model instance. */
typedef struct nint_geom {
  int32_t H, W;    /* grid the model runs on (100x154 = 90x144 + halo 5 in the reference, launcher.sh:24) */
  int32_t P;       /* physical zero halo of halo slabs = max_l(k_l/2) */
  int32_t Hh, Wh;  /* halo-slab rows / cols: roundup(H,8)+2P, roundup(W,32)+2P */
} nint_geom;

/* One ConvLSTMCell (reference model.py:196-231) in packed form. */
typedef struct nint_layer {
  int32_t Cx, Cxp;        /* input channels / padded to KC */
  int32_t Ch, Ch16, Chp;  /* hidden channels / padded to 16 / padded to KC */
  int32_t k;              /* odd kernel size, padding k/2 (model.py:204) */
  int32_t tile_rows;      /* rows of the gate / dgrad kernels' pixel tile: 0 = chosen per launch shape, or 4 / 8.  Tiny layers
                           * (nint_stencil_holds()) have two more gate kernels: 1 = one pixel per LANE, the vector-ALU stencil
                           * kernel (csrc/stencil.hip); 2 = the matrix pipe with a dense K (csrc/tiny_gemm.hip; also the library's
                           * choice for such layers in f32 storage).  On other layers 1 / 2 mean 0. */
  int32_t xfold;          /* 1: the x source is HORIZONTALLY FOLDED (thin inputs, first layer only): slab channel
                           * kx*Cx + c holds x[.., x + kx - k/2][c] (0 outside the image), Cxp = roundup(k*Cx, KC), and
                           * the x part of K is k vertical taps x k*Cx channels instead of k*k taps x Cx channels padded
                           * to KC each (reference layer 0: Conv2d(5+64 -> 256, k=5), model.py:207-211: 5 x-steps, not 25) */
  int32_t wide;           /* weight-gradient kernel family (csrc/wgrad.hip): 0 = the library's choice (the 8-wave kernel with a
                           * 128-gate-column output block wherever it is instantiated and the layer is wide enough, else
                           * the 4-wave 64-column kernel); 1 = always the 4-wave kernel; 2 = the 8-wave kernel wherever it is
                           * instantiated (bf16, k = 3 / 5 / 7, unfolded sources, gate columns a multiple of 128, channel
                           * counts a multiple of its channel group), whatever the layer's width.  Same sums in another f32
                           * order.  (Rounds 2-3 used this field for an 8-wave GATE kernel that measured slower everywhere
                           * and left the library in round 4: tools/experiments/.) */
  const void* Wf;         /* fwd weights, MFMA-fragment order, ET   (nint_pack_weights) */
  const void* Wd;         /* dgrad weights (transposed + flipped), ET */
  const float* bias_p;    /* bias permuted to gate-stash column order [4*Ch16] */
} nint_layer;

/* Everything one forward/backward over a (B,T) batch needs.  All pointers are device
 * workspaces allocated by the caller; sizes follow from nint_seq_workspace_sizes(). */
#define NINT_MAX_LAYERS 8
typedef struct nint_seq {
  int32_t dtype;            /* NINT_F32 | NINT_BF16: storage type ET of halo slabs / stash / weights */
  int32_t B, T, L;
  int32_t need_dx;          /* backward also produces d/dx of the input sequence */
  int32_t has_init_state;   /* 0: h0=c0=0 (reference ConvLSTM, model.py:259-262); 1: h[l][0], c0[l] given */
  int32_t n_cu;             /* CU count used to size split-K grids */
  int32_t zero_dstate;      /* backward: bit 2l = dc[l] is all-zero at entry, bit 2l+1 = dh[l] is all-zero at entry -- the first
                             * BPTT step then neither reads nor needs them zero-filled (reference: zero state grads) */
  nint_geom g;
  /* nint_seq_bwd: the first layer whose parameters are trained (fine-tuning: the layers below are frozen).
   *   0       every layer (the pass as it has always been: same launches, same bits)
   *   f > 0   dW / db are produced for layers f .. L-1 only, and BPTT stops above layer f-1: no pointwise backward, dgrad or
   *           weight-gradient launch for a layer below f, and layer f's dgrad computes no x columns (as layer 0's under
   *           need_dx = 0).  Exact, not an approximation: d/dh of a layer below f feeds only the parameters and initial
   *           states of layers < f and the input.  The pass IS the backward pass of the stack of layers f .. L-1 whose input
   *           slab is h[f-1] from image B on (h^{f-1}_t = slab t+1) with need_dx = 0: zero_dstate and an explicit fuse_bwd
   *           mask shifted down by f layers, dh_seq on the top layer, the `wave` merges of that stack ("the bottom layer" of
   *           the wave modes is layer f), wg_partial sized for layers >= f.  For l < f none of gates[l], dG[l], dh[l], dc[l],
   *           dW[l], db[l] is read: all may be NULL (and a forward pass with gates[l] == NULL writes no stash for l).
   *           nint_debug_seq_plan and the probe tags carry the real layer index.
   *   L       valid: nothing is planned (the head alone is trained).
   * NINT_E_ARG before any launch: a value outside [0, L]; f > 0 with need_dx (d/dx passes through every layer) or with
   * bwd_parts != 0 (the two-piece exchange is defined around layer 0's slice).  nint_seq_fwd does not read the field.
   * (The field takes the four bytes that were padding between g and the 8-byte aligned layer[]: no offset of the structure
   * moves and its size stays, so a caller that zero-fills the structure, as every caller must, gets 0.) */
  int32_t train_from;
  nint_layer layer[NINT_MAX_LAYERS];
  const void* xs;                      /* ET halo slab [T*B][Hh][Wh][Cxp0]: packed input sequence */
  void* h[NINT_MAX_LAYERS];            /* ET halo slab [(T+1)*B][Hh][Wh][Chp]: h[0]=initial, h[t+1]=h_t */
  float* c[NINT_MAX_LAYERS];           /* f32 compact [(T+1)*B][H][W][Chp]: c[0]=initial, c[t+1]=c_t */
  void* gates[NINT_MAX_LAYERS];        /* ET stash [T*B][H][W][4*Ch16] post-activation i,f,g,o (training only; may be NULL) */
  void* dG[NINT_MAX_LAYERS];           /* ET halo slab [T*B][Hh][Wh][4*Ch16] pre-activation gate grads */
  void* dh[NINT_MAX_LAYERS];           /* ET compact [B][H][W][Chp] running dL/dh_t (in: dL/dh_{T-1}, out: dL/dh_init) */
  float* dc[NINT_MAX_LAYERS];          /* f32 compact [B][H][W][Chp] running dL/dc_t */
  void* dx;                            /* ET compact [T*B][H][W][Cxp0] (need_dx only) */
  float* dW[NINT_MAX_LAYERS];          /* f32 OIHW (4Ch, Cx+Ch, k, k) gradient, overwritten (accumulate = 1: added to) */
  float* db[NINT_MAX_LAYERS];          /* f32 (4Ch) gradient, overwritten (accumulate = 1: added to) */
  float* wg_partial;                   /* f32 split-K slabs for wgrad: the SUM over the layers of nint_wgrad_workspace_bytes
                                        * (each rounded up to 256 bytes) -- the layers' slabs sit side by side */
  size_t wg_partial_bytes;
  int32_t fuse_bwd;                    /* backward schedule: 0 = per layer (fused BPTT step for the short-K layers), 1 = never
                                        * fused, 2 = every layer fused, 0x40000000 | masks = explicit: bit l: layer l runs the
                                        * fused step; bit 8+l: the fused layer l also runs the pointwise backward of the
                                        * classic layer l-1 on its x columns; bit 16+l: the CLASSIC layer l does that for the
                                        * classic layer l-1 (nint_cell_bwd_fused; same results up to the bf16 rounding of the
                                        * intermediate dh, which the fused step skips) */
  int32_t probe_mask;                  /* in-step timing probes (diagnostic; 0 = none): bit k brackets every launch of kind k
                                        * (NINT_PROBE_*) of nint_seq_fwd / nint_seq_bwd with two one-thread stamp launches */
  /* Boundary condition in x.
   *   0  zero padding on every side (nn.Conv2d, model.py:207-211): the pass as it has always been -- same plan, same launches,
   *      same bits.
   *   1  CYCLIC LONGITUDE: column 0 and column W-1 are neighbours in every convolution of the stack; rows keep their zero
   *      padding.  The conv, dgrad and weight-gradient kernels are the same ones: they read their taps from the physical halo,
   *      and a small copy kernel (halo_wrap_kernel, its launches steps of the plan) fills the halo COLUMNS of the interior
   *      rows with the wrapped interior columns -- of xs (unfolded) and of a given initial h at the head of the forward
   *      pass, of every h block right behind the launch that wrote it, of every dG block right behind its writer -- and
   *      writes them back to zero in a dG block right behind the dgrad that read it: the weight gradient walks the slack
   *      columns and needs dG zero there.  After nint_seq_bwd every dG image has zero halos again; xs and h stay wrapped.
   *      A horizontally folded xs (nint_layer.xfold) must have been packed with the _cyclic entries below: it has no
   *      horizontal taps for a halo to serve.  Needs W >= P.
   * Any other value, or W < P with 1: NINT_E_ARG before any launch.  nint_debug_seq_plan lists conv / pointwise problems only:
   * with 1 their `index` counts the wrap launches in between.  (A caller that zero-fills the structure, as every caller must, gets 0.
   * The field sits behind probe_mask, in front of the 8-byte aligned `probe`: the fields behind it move by 8 bytes together and
   * dh_seq stays the last one.) */
  int32_t lon_cyclic;
  unsigned long long* probe;           /* device buffer of probe_slots {tag, s_memrealtime (100 MHz)} pairs, or NULL.  nint_seq_fwd
                                        * fills slots from 0, nint_seq_bwd from probe_slots / 2; each starts with two back-to-back
                                        * calibration stamps (kind 0).  tag = kind | layer << 8 | t << 16 | end << 31 */
  int32_t probe_slots;
  /* Independent launches as ONE grid (csrc/conv_igemm.hip: conv_lstm_multi[8]_kernel, conv_bwd_multi[8]_kernel,
   * conv_dgrad_multi8_kernel; every problem of a grid runs the body its own launch would have run).
   *   0  every launch by itself, time-major order (for t: for layer).
   *   1  forward: the (t, layer) wavefront (model.py:265-271: gate(l, t) needs gate(l-1, t) and gate(l, t-1) only, so gate(0, t+1),
   *      gate(1, t), gate(2, t-1) are independent) -- each wavefront step is one grid, T + L - 1 launches instead of T * L, every
   *      layer on the tiles its own launch takes; BPTT: the bottom layer's dgrad of one step with the top layer's fused step of
   *      the next (adjacent launches that share no buffer in a stack of three or more layers).  Bit-identical to 0.
   *   2  the forward wavefront only, every layer of a grid on 8-row tiles (the first layer's tile makes the grid a two-workgroups-
   *      per-CU kernel anyway; half the weight bytes per MFMA for the narrow layers: forward pass -5 % at B = 8,
   *      profiles/r04_c_wave_repeats.txt, r04_d_wave_rows8.txt).  = the time-major order with tile_rows pinned to 8 bit for bit, the
   *      default time-major order (4-row narrow tiles: another order of the K-slice partials) to f32 rounding.
   *   3  2 + the BPTT pair of 1 with the fused step on 8-row tiles (measured +0.2 ... +0.5 %; not used).
   *   4  the forward pass of 2; BPTT as TWO grids per step (profiles/r04_f_wave4.txt):
   *      (a) the bottom layer's dgrad of time u+1 waits for layer 1's dgrad of time u: one grid, the wide launch first, so that
   *          the narrow layer's workgroups fill its last round.  Both produce a piece of the bottom layer's d/dh of time u; each
   *          stores its own (layer 1 into dh[0], the bottom layer into the head of wg_partial, idle until the weight gradients)
   *          and the bottom layer's pointwise backward adds the two: f32 = the time-major order bit for bit (the same f32 sum);
   *          bf16: each piece is rounded before the f32 add instead of the running sum after it (layer 0's gradients move by
   *          ~1e-3 relative).  Needs wg_partial_bytes >= B*H*W*Chp[0]*es and classic (unfused) steps in layers 0 and 1;
   *      (b) with a fused top layer in a stack of three or more, the bottom layer's pointwise backward of time u waits for the
   *          top layer's fused step of time u-1 (the next launch, touching layers >= 1 only): one grid, the pointwise pass as a
   *          problem of the conv kernel (the same arithmetic: bit-identical).
   *      B = 2 / 4 / 8 at 100 x 154: +4.5 / +1.8 / +0.65 % over 2; B = 12 / 16 / 32: +1 ... +2 % over 0.
   *   5  the forward pass of 1 with the BPTT of 4 (B = 1 at 100 x 154: 661 against 647 samples/s of 1 and 622 of 4).
   * A shape the merged kernels do not hold (register-heavy fused shapes, more than 4 layers, launch shapes without a case) goes out
   * as separate launches.  Probes do not change the schedule: merged grids are bracketed as such (NINT_PROBE_WAVE,
   * NINT_PROBE_BWD_PAIR, NINT_PROBE_BWD_PW).  SeqEngine picks 5 for the smallest batches and 4 above (engine.py:_set_wave). */
  int32_t wave;
  /* nint_seq_bwd in two calls, for the data-parallel exchange: 0 = everything in one call; 1 = the BPTT chain and
   * the weight / bias gradients of layers >= 1 (their fold included); 2 = the weight / bias gradient of layer 0 only (dG[0] of
   * a preceding part-1 call on the same stream is its input).  Between the two the caller starts the all-reduce of everything
   * but layer 0's slice of the gradient bucket, which then runs under layer 0's weight gradient -- the largest launches of the
   * step -- instead of after them.  Same launches, same order inside each layer: bit-identical gradients. */
  int32_t bwd_parts;
  /* nint_seq_bwd: how the weight / bias gradients of this call reach dW[l] / db[l].
   *   0  stored: dW[i] = s (the buffers need no initialisation)
   *   1  added:  dW[i] = dW[i] + s, one f32 add (round to nearest even) by the ONE thread that owns element i in the fold of
   *      the split-K slabs -- s is the very f32 sum that 0 would have stored, formed in the same fixed order.  No atomics and
   *      no second pass: the result is (float)(old + s) bit for bit, run to run, for every dW and db element the call
   *      produces (both weight-gradient families of nint_layer.wide, the bias column, and under bwd_parts the layers of
   *      that part only; the other layers' buffers are not touched).  dW / db then hold what the caller wants added to:
   *      the gradients of the window's later segments (checkpointed BPTT) or of the micro-batches
   *      before this one.
   * The BPTT chain, the launch list and dx / dh / dc do not depend on it.  Any other value: NINT_E_ARG before any launch.
   * (The field takes the four bytes that were padding between bwd_parts and the pointer behind it: no offset of the
   * structure moves and its size stays, so a caller that zero-fills the structure, as every caller must, gets 0.) */
  int32_t accumulate;
  const void* dh_seq;   /* ET compact [T*B][H][W][Chp of layer L-1], image t*B+b: dL/dh_t of the TOP layer that does not come
                         * through the recurrence (the per-step head outputs: nint_head_bwd_seq / nint_head_loss_seq_fused);
                         * NULL = none (many-to-one: the only such term is dL/dh_{T-1}, in dh[L-1]).  Non-NULL: at every t the
                         * top layer's d/dh_t is its recurrent part plus block t; at t = T-1 block T-1 is the only source and
                         * dh[L-1] is not read on entry.  The addend enters through pointers the BPTT bodies already have (the
                         * second d/dh piece of the pointwise backward, the `old` columns of the fused step), so the launch
                         * plan is the one without it, merged grids included.  16-byte aligned, else NINT_E_ALIGN. */
} nint_seq;

/* CLOSED-LOOP FORWARD: what nint_seq_fwd_closed takes beside the nint_seq.  (A structure of its own: the
 * layout and the size of nint_seq are pinned -- dh_seq is and stays its last field.)
 * The last O input channels, [c0, c0 + O) with c0 = layer[0].Cx - O, are FEEDBACK channels.  With F = min(max(from, 0), T),
 * before the gates of every step t >= F the pass stores, for every pixel of the grid,
 *     xs[t*B + b][y][x][c0 + o] = round_ET( b[o] + sum_c w[o][c] * h[L-1] slab t [b][y][x][c] )
 * -- the staged head's f32 value (nint_head_fwd, bit for bit) rounded once to ET (nint_head_feedback below; a folded xs
 * receives every value in its k places).  Slab t of h[L-1] is the top layer's hidden state after step t-1, slab 0 the
 * initial state.  SO WITH O > 0 THE PASS WRITES nint_seq.xs, which is declared const for the open-loop pass.
 * Steps t < F read what the caller packed (spin-up) and are planned as an open-loop pass of F steps; steps t >= F go out
 * time-major -- feedback(t), gate(0, t) ... gate(L-1, t), each its own launch, on the tile_rows the same `wave` gives the
 * open-loop pass -- so the pass equals, bit for bit, the open-loop pass over an input that already holds those values.
 * With lon_cyclic and an unfolded xs a halo wrap launch for xs block t follows feedback(t).
 * O = 0 (a zero-filled structure, or a NULL pointer to one): open loop -- the plan, the launches and the bits of nint_seq_fwd. */
typedef struct nint_feedback {
  const float* w;       /* f32 (O, Ch of layer L-1): the head's weight */
  const float* b;       /* f32 (O), or NULL: no bias */
  int32_t O;            /* head outputs fed back; 0 = off */
  int32_t from;         /* first fed step */
} nint_feedback;

/* ROLL-OUT BACKWARD: what nint_seq_bwd_rollout takes beside the nint_seq and the nint_feedback of the window's
 * closed-loop forward pass.  (Again a structure of its own: nint_seq and nint_feedback keep their layout and size.) */
typedef struct nint_feedback_grad {
  float* dpred;         /* f32 [T*B][O][H][W], image t*B + b.  In: l_t, the direct cotangent of p_t = head(h^{L-1} after step t)
                         * (zeros where the loss has no term).  Out: g_t = l_t + xi_{t+1} for F-1 <= t <= T-2, xi_u being
                         * d/dx of step u on the feedback channels; the other images stay.  nint_head_bwd_acc(n0 = B, N = T*B,
                         * dh = NULL) reduces the slab to the head's dw / db.  4-byte aligned. */
  void* dx_step;        /* ET compact [B][H][W][Cxp0]: where layer 0's dgrad of a fed step stores its x columns when need_dx = 0
                         * (one step's block, overwritten step after step; not read with need_dx = 1, may be NULL then).
                         * 16-byte aligned. */
} nint_feedback_grad;

/* SCHEDULED SAMPLING: a per-step, per-image feed mask beside the nint_feedback, for the _sampled entries below.
 * (A structure of its own once more: nint_seq, nint_feedback and nint_feedback_grad keep their layout and size.)
 * fed[t*B + b] = 1: image b runs step t on the fed-back prediction -- xs[t*B + b] receives round_ET(p_{t-1}[b]) on the feedback
 * channels exactly as in nint_feedback's rule; fed[t*B + b] = 0: image t*B + b of xs keeps every byte the caller packed (a
 * folded slab's k copies and a cyclic slab's halo columns included).  fed[t][b] = (t >= s) IS nint_feedback.from = s, bit for
 * bit, gradients included.  The bytes are read on the HOST while the pass is planned and reach the kernels by value, one
 * 64-bit word per feedback launch: the library keeps no copy, and a masked window holds B <= 64.
 * fed == NULL (or a NULL pointer to the structure): "use fb->from" -- every _sampled entry is then the entry it extends. */
typedef struct nint_feedback_mask {
  const uint8_t* fed;   /* HOST bytes, T*B of them, index t*B + b, each 0 or 1; NULL = none */
} nint_feedback_mask;

/* NOISE ON THE FED-BACK VALUE, beside the nint_feedback, for nint_seq_fwd_stochastic and
 * nint_head_feedback_noise.  (A structure of its own again: the structures above keep their layout and size.)  The value a fed
 * step t stores for (image b, output o, pixel) becomes
 *     round_ET( __fadd_rn( p, __fmul_rn(sigma[o], z) ) )
 * p: the f32 prediction the launch forms without it (a residual head: after the base has been added); z: the normal of
 * nint_input_noise's rule for (pixel y*W + x, channel offset o, step step0 + t, lane lane0 + b) under the key (seed, draw) --
 * the same device function, the number nint_noise_normal returns.  The product and the sum are two f32 operations.  A channel
 * with sigma[o] == 0 stores what it stores without the structure; a folded slab's k copies receive one value, keyed by the
 * source pixel; under a mask only fed images draw.  sigma == NULL (or a NULL pointer to the structure): off -- the entry is then
 * the entry it extends: same plan, same launches, same bits. */
typedef struct nint_feedback_noise {
  const float* sigma;   /* DEVICE f32 [O]; NULL = off */
  uint32_t seed, draw, step0, lane0;
} nint_feedback_noise;

/* launch kinds for nint_seq.probe_mask / the probe tags */
enum { NINT_PROBE_CAL = 0, NINT_PROBE_GATE = 1, NINT_PROBE_POINTWISE = 2, NINT_PROBE_DGRAD = 3, NINT_PROBE_FUSED = 4,
       NINT_PROBE_WGRAD = 5, NINT_PROBE_FOLD = 6,
       NINT_PROBE_WAVE = 7, /* a merged forward grid (nint_seq.wave): tag layer = number of gate launches in it, t = wavefront step */
       NINT_PROBE_BWD_PAIR = 8, /* a merged BPTT grid of two conv launches (wave = 4 / 5: the dgrad launches of layers 0 and 1; wave = 1 / 3:
                                 * the bottom dgrad with the top layer's fused step): tag layer = the second launch's layer, t = its time step */
       NINT_PROBE_BWD_PW = 9,   /* wave = 4 / 5: the top layer's fused step with the bottom layer's pointwise backward: tag layer = the
                                 * fused layer, t = its time step */
       NINT_PROBE_WRAP = 10,    /* nint_seq.lon_cyclic: a halo wrap / clear launch: tag layer = its number of jobs, t = 0 */
       NINT_PROBE_FEEDBACK = 11, /* nint_seq_fwd_closed: the feedback launch of step t: tag layer = 0, t = the step */
       NINT_PROBE_FEEDBACK_BWD = 12 /* nint_seq_bwd_rollout: the feedback backward launch of step u: tag layer = 0, t = u */ };

/* ---- library / device ---------------------------------------------------------------- */
int nint_version(void);
const char* nint_error_string(int code);
/* host out-params */
int nint_device_info(int* n_cu, int* lds_bytes_per_cu, int* wave_size, char* name, int name_len);
/* Hardware self-test used by tests: MFMA fragment maps and ds_read_b64_tr_b16 semantics.
 * out: device buffer of >= 4096 floats. */
int nint_selftest(float* out, void* stream);

/* channel padding rule: KC = 16 (f32) or 32 (bf16) channels = 64 bytes per pixel per K-step */
int nint_kc(int dtype);
int nint_geom_make(nint_geom* g /*host*/, int H, int W, int P);

/* ---- layout conversion at the boundary ------------------------------------------------- */
/* x (B,T,C,H,W) f32 contiguous (model.py:255) -> halo slab image t*B+b.  Replaces the
 * `x[:, t]` slicing of model.py:266 and torch.cat of model.py:219 (never materialised). */
int nint_pack_btchw(const float* src, void* dst, int B, int T, int C, int Cp, const nint_geom* g,
                    int dtype, void* stream);
/* the same into a HORIZONTALLY FOLDED slab (nint_layer.xfold): channel kx*C + c of pixel x holds src[.., x + kx - k/2]
 * (zero outside the image: the convolution's own zero padding), Cp >= k*C */
int nint_pack_btchw_xfold(const float* src, void* dst, int B, int T, int C, int k, int Cp, const nint_geom* g,
                          int dtype, void* stream);
/* backward of that fold: compact ET slab [N][H][W][Cp] of d/d(folded x) -> d/dx (N,C,H,W) f32,
 * dx[c][x] = sum_kx dfold[x - kx + k/2][kx*C + c] */
int nint_unfold_dx(const void* src, float* dst, int N, int C, int k, int Cp, int H, int W, int dtype, void* stream);
/* The two above for CYCLIC LONGITUDE (nint_seq.lon_cyclic): the fold reads pixel (x + kx - k/2) mod W instead of a zero outside
 * the image, and its adjoint sums over the source pixels taken mod W.  Same arguments; in addition W < k/2: NINT_E_ARG. */
int nint_pack_btchw_xfold_cyclic(const float* src, void* dst, int B, int T, int C, int k, int Cp, const nint_geom* g,
                                 int dtype, void* stream);
int nint_unfold_dx_cyclic(const void* src, float* dst, int N, int C, int k, int Cp, int H, int W, int dtype, void* stream);
/* halo slab images [n0, n0+N) -> (N,C,H,W) f32 */
int nint_unpack_halo(const void* src, float* dst, int n0, int N, int C, int Cp, const nint_geom* g,
                     int dtype, void* stream);
/* (N,C,H,W) f32 <-> compact f32 slab [N][H][W][Cp] */
int nint_pack_compact(const float* src, void* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream);   /* dtype: element type of the compact slab */
int nint_unpack_compact(const void* src, float* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream);
/* compact slab += (N,C,H,W) f32: a cotangent that arrives as a tensor joins a gradient already in slab form (the returned final
 * hidden state's cotangent on top of the head's dL/dh_{T-1} in nint_seq.dh[L-1] / the last block of nint_seq.dh_seq).  The
 * channel padding is not touched. */
int nint_pack_compact_add(const float* src, void* dst, int N, int C, int Cp, int H, int W, int dtype, void* stream);

/* ---- weights ----------------------------------------------------------------------------- */
/* 1 when horizontally folding the x source of a (first) layer lowers its number of K-steps:
 * ceil(k*Cx / KC) * k < ceil(Cx / KC) * k * k  (see nint_layer.xfold); pure host arithmetic */
int nint_xfold_pays(int Cx, int k, int dtype);
/* bytes to reserve for EACH of the packed fwd / dgrad weight images of one layer.
 * Memory contract: a buffer of exactly this size is enough -- no kernel stores outside it, and no result
 * depends on a byte outside it.  The size is the dgrad image's: a folded forward image ends short of it and the extra images of
 * tiny layers leave gaps; those bytes are never written and never read (the caller zero-fills both buffers once). */
size_t nint_packed_weight_bytes(int Cx, int Ch, int k, int dtype, int xfold);
/* W (4Ch, Cx+Ch, k, k) f32 OIHW + bias (4Ch) as nn.Conv2d stores them (model.py:207-211)
 * -> Wf, Wd (fragment order, ET) and bias_p.  Must be re-run after every optimiser step. */
int nint_pack_weights(const float* W, const float* bias, void* Wf, void* Wd, float* bias_p,
                      int Cx, int Ch, int k, int xfold, int dtype, void* stream);

/* the same for every layer of a model in ONE launch: W[l] / bias[l] (host arrays of device pointers; bias[l] may be
 * NULL) into layers[l].Wf / .Wd / .bias_p */
int nint_pack_weights_layers(const float* const* W /*host*/, const float* const* bias /*host*/,
                             const struct nint_layer* layers /*host*/, int L, int dtype, void* stream);

/* ---- the hot path: one cell step ----------------------------------------------------------- */
/* ConvLSTMCell.forward (model.py:216-231): gates = conv(cat[x,h]) ; sigmoid/tanh ; c,h update,
 * fused.  x_slab/h_prev halo slabs (image n0x.. / n0h..), c_prev/c_out compact, h_out halo slab,
 * gates_out stash (NULL in inference).  h_prev == NULL means h_prev = 0 (skips that half of K). */
int nint_cell_fwd(const nint_layer* ly /*host*/, const nint_geom* g /*host*/, int dtype, int N,
                  const void* x_slab, const void* h_prev, const float* c_prev,
                  void* h_out, float* c_out, void* gates_out, void* stream);

/* 1 when the vector-ALU STENCIL kernel (csrc/stencil.hip) holds this layer's gate step: tiny hidden widths (Ch <= 8: at most
 * 32 gate columns, no dense contraction), k = 3, thin input (<= 16 channels, or a folded first-layer input of <= 64 folded
 * channels).  nint_cell_fwd runs it for nint_layer.tile_rows == 1.  One lane per pixel, LDS-staged halo tile, DPP row
 * shifts for the horizontal taps, scalar-operand weights, the same LSTM epilogue.  Pure host arithmetic. */
int nint_stencil_holds(const nint_layer* ly /*host*/);

/* autograd backward of model.py:223-229 (pointwise part): consumes dh, dc (in place -> dc_prev),
 * the stashed gates and c_prev / c_new; writes pre-activation gate grads into the dG halo slab. */
int nint_cell_bwd_pointwise(const nint_layer* ly, const nint_geom* g, int dtype, int N,
                            const void* gates, const float* c_prev, const float* c_new,
                            const void* dh, float* dc, void* dG, void* stream);

/* conv backward-data of model.py:220: d cat[x,h] = W^T (*) dG.  h columns are STORED to dh_prev,
 * x columns are ACCUMULATED (+=) into dx_accum (the layer below's dh, or dx); either may be NULL. */
int nint_conv_dgrad(const nint_layer* ly, const nint_geom* g, int dtype, int N,
                    const void* dG, void* dx_accum, void* dh_prev, void* stream);

/* One fused BPTT step of a cell: conv backward-data of time t+1 AND the pointwise backward of time t.
 *   d cat[x,h]_{t+1} = W^T (*) dG_next;  x columns are STORED to dx (compact, may be NULL: not computed);
 *   d/dh_t = (h columns) + dh_above  never goes to memory: it feeds the pointwise backward of time t (gates / c_prev /
 *   c_new = the stash of time t; c_prev == NULL means c_{t-1} = 0), which overwrites dc in place (-> d/dc_{t-1}) and
 *   writes the dG halo slab of time t.  dh_above: d/dh_t from the layer above (its x columns) or the head, compact
 *   [N][H][W][Chp] ET; NULL = 0.  Same results as nint_conv_dgrad + nint_cell_bwd_pointwise up to the bf16 rounding of
 *   the intermediate dh, which this entry skips. */
int nint_cell_bwd_fused(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* dG_next, void* dx,
                        const void* gates, const float* c_prev, const float* c_new, const void* dh_above,
                        float* dc, void* dG, void* stream);

/* conv backward-weight of model.py:220 over N = T*B images in ONE launch (all time steps):
 * dW[o][c][ky][kx] = sum_n,y,x dG[n,y,x,o] * cat[n,y+ky-p,x+kx-p,c] ; db[o] = sum dG.
 * partial: split-K workspace of nint_wgrad_workspace_bytes().
 * Memory contract: a workspace of exactly this size is enough for every N and grid (the split count the
 * query assumes is an upper bound; a smaller workspace is NINT_E_ARG before any launch) -- no kernel stores outside it, and
 * no result depends on a byte outside it or on its prior contents. */
size_t nint_wgrad_workspace_bytes(const nint_layer* ly, int dtype, int n_cu);
int nint_conv_wgrad(const nint_layer* ly, const nint_geom* g, int dtype, int N,
                    const void* dG, const void* x_slab, const void* h_slab,
                    float* dW, float* db, float* partial, size_t partial_bytes, int n_cu, void* stream);
/* db rides along with the x source's weight gradient: the dG fragments are multiplied with an all-ones fragment on the
 * matrix pipe (one extra column of the split-K slab), so there is no separate pass over dG. */

/* ---- whole-sequence drivers (model.py:253-274 and its BPTT), all launches from C++ ---------- */
int nint_seq_fwd(const nint_seq* s /*host*/, void* stream);
int nint_seq_bwd(const nint_seq* s /*host*/, void* stream);
/* The same two passes for a CLOSED-LOOP window (struct nint_feedback above; fb == NULL or fb->O == 0: exactly the entries above).
 * nint_seq_fwd_closed runs the forward pass with the feedback steps in its plan.  nint_seq_bwd_closed exists to refuse, in the
 * library, what is not defined: the backward pass of a window in which something was fed back (fb->O > 0 with fb->from < T) is
 * NINT_E_ARG before any launch -- d/dx of a fed step would have to re-enter the top layer's d/dh of the step before, which
 * re-plans BPTT; a window in which nothing was fed back (fb->from >= T) trains as ever.
 * NINT_E_ARG before any launch (both, and nint_debug_seq_plan_closed): fb->O < 0, fb->O > layer[0].Cx, fb->O > 0 with
 * fb->w == NULL, fb->from < 0, fb->from == 0 without has_init_state (step 0 can only be fed from a state that was handed in).
 * NINT_E_SHAPE before anything is enqueued: a head the feedback kernel does not hold (nint_head_feedback). */
int nint_seq_fwd_closed(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, void* stream);
int nint_seq_bwd_closed(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, void* stream);

/* BPTT THROUGH THE FED-BACK PREDICTION: the backward pass of a window whose forward pass was
 * nint_seq_fwd_closed(s, fb) with 1 <= F = fb->from < T.  The rounding of the fed value is straight-through (derivative 1).
 *   for u = T-1 ... 0:  for l = L-1 ... 0: pointwise backward (l, u), then conv backward-data (l, u), each its own launch
 *                       (the arithmetic of fuse_bwd = 1 with wave = 0, whatever the two fields say: xi_u exists only after
 *                       layer 0's dgrad of step u and the top layer's pointwise backward of step u-1 needs it);
 *                       layer 0's dgrad stores its x columns for every u >= F (need_dx: for every u, into dx block u);
 *                       F <= u <= T-1: nint_head_feedback_bwd -- dpred images of step u-1 += xi_u, dh_seq block u-1 = W^T g_{u-1}
 *   then the weight / bias gradients as in nint_seq_bwd (layer 0's x source is xs, which holds the fed values).
 * dh_seq is REQUIRED: on entry block t holds W^T l_t for t < F-1 and t = T-1 (zeros where the loss has no term: the caller
 * clears or writes them, nint_head_bwd_acc with dw = NULL does); blocks F-1 ... T-2 are overwritten and need no initialisation.
 * dx (need_dx) receives the chain's d/dx of every step, fed channels of fed steps included: those values are xi, not a gradient of
 * the caller's x (which the forward pass overwrote there) -- the caller zeroes them.  accumulate: as in nint_seq_bwd.
 * fb->O == 0 or fb->from >= T: nothing was fed back -- exactly nint_seq_bwd(s), rg is not read.
 * NINT_E_ARG before any launch (fed windows): fb->from == 0, train_from > 0, bwd_parts != 0, a NULL rg, rg->dpred or dh_seq, a
 * NULL rg->dx_step with need_dx = 0, and everything nint_seq_bwd and nint_seq_fwd_closed refuse.  NINT_E_ALIGN: rg->dpred not
 * 4-byte, rg->dx_step / dx not 16-byte aligned.  NINT_E_SHAPE before anything is enqueued: a head nint_head_feedback_bwd
 * does not hold.  nint_seq_bwd_closed keeps refusing every fed window. */
int nint_seq_bwd_rollout(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, const nint_feedback_grad* rg /*host*/,
                         void* stream);

/* The closed-loop forward and the roll-out backward under a FEED MASK (struct nint_feedback_mask above).
 * fm == NULL or fm->fed == NULL, or fb->O == 0: exactly nint_seq_fwd_closed / nint_seq_bwd_rollout.  With a mask fb->from is
 * ignored and F is the first step with a fed image (T: none -- the open loop).
 *   forward   steps [0, F) are the open-loop pass of F steps; steps [F, T) go out time-major, and the feedback launch (behind
 *             it the xs wrap of cyclic longitude with a plain slab) only at steps with a fed image; it writes the fed images only.
 *   backward  time-major as nint_seq_bwd_rollout; layer 0's dgrad stores its x columns for u >= F, and the feedback backward of
 *             step u goes out for EVERY u in [F, T-1]: g_{u-1}[b] = l_{u-1}[b] + (xi_u[b] if fed[u][b] else 0), dh_seq block u-1 =
 *             W^T g_{u-1} -- so dh_seq blocks t < F-1 and T-1 are the caller's and blocks F-1 ... T-2 the chain's, as before.
 *             dx (need_dx) holds xi on the fed channels of fed (t, b) only -- the caller zeroes those; on an unfed image of a
 *             step it is the input's gradient.
 * The mask's checks sit where the feedback's do (step 2 of the one check; the roll-out looks at the feedback
 * after the backward fields): NINT_E_ARG for a byte other than 0 or 1, a fed image at step 0 without has_init_state and, in
 * the roll-out, any fed image at step 0; then, with everything else in order, NINT_E_SHAPE for B > 64 -- before any launch. */
int nint_seq_fwd_sampled(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, const nint_feedback_mask* fm /*host*/,
                         void* stream);
int nint_seq_bwd_rollout_sampled(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, const nint_feedback_mask* fm /*host*/,
                                 const nint_feedback_grad* rg /*host*/, void* stream);

/* The two _sampled entries for the RESIDUAL HEAD: p_t = x_t[feedback channels] + head(h_t), x_t as the model
 * saw it -- on a teacher-forced step what the caller packed, on a fed step round_ET(p_{t-1}).  They ARE nint_seq_fwd_sampled
 * and nint_seq_bwd_rollout_sampled (fm == NULL or fm->fed == NULL: "use fb->from") with the residual feedback launches in the
 * same places of the same plan: same launch list, same `index` numbering of the debug plans, same wrap launches.
 *   forward   the feedback launch of step t reads its base from block t-1 of xs (nint_head_feedback_res): the fed value is
 *             round_ET( head(h after step t-1) + x_{t-1}[feedback channels] ).  So the pass equals, bit for bit, the open-loop
 *             pass over an input that already holds the fed values, and its per-step outputs are nint_head_fwd_seq_res of it.
 *   backward  the feedback backward launch of step u (nint_head_feedback_bwd_res) also adds g_u, final in dpred block u:
 *             g_{u-1}[b] = l_{u-1}[b] + fed[u][b] * (xi_u[b] + g_u[b]), dh_seq block u-1 = W^T g_{u-1}.  dpred comes back
 *             holding the total cotangent g_t of every p_t; the caller adds it to its d/dx on the feedback channels of
 *             the unfed (t, b) -- the skip path into its own input -- and zeroes the fed ones, as before.
 * Additionally refused with NINT_E_ARG, before any launch, where the feedback is looked at: a fed image at step 0 -- p_{-1}
 * has no base, even with an initial state.  fb->O == 0 or nothing fed: the open-loop entries, as ever. */
int nint_seq_fwd_residual(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, const nint_feedback_mask* fm /*host*/,
                          void* stream);
int nint_seq_bwd_rollout_residual(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, const nint_feedback_mask* fm /*host*/,
                                  const nint_feedback_grad* rg /*host*/, void* stream);

/* The closed-loop forward with noise on the fed-back value (nint_feedback_noise above; forward only: there is no backward
 * entry).  It IS nint_seq_fwd_sampled (residual == 0) / nint_seq_fwd_residual (residual == 1) with the feedback launch of step t
 * drawing its noise for step step0 + t, lanes lane0 + b: no launch is added, and fn == NULL or fn->sigma == NULL gives that
 * entry's plan, launches and bits.  The closed-loop contract carries over: the pass equals, bit for bit, the open-loop pass over
 * an input that already holds the stored values.  Additionally refused before any launch: residual not 0 / 1 (NINT_E_ARG), a
 * sigma that is not 4-byte aligned (NINT_E_ALIGN, where the feedback is looked at). */
int nint_seq_fwd_stochastic(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, const nint_feedback_mask* fm /*host*/,
                            int residual, const nint_feedback_noise* fn /*host*/, void* stream);

/* The launch plan of a pass, for tests and tools (host only: nothing is enqueued, no pointer is dereferenced).  Both drivers
 * first PLAN a pass into an ordered list of launches and then enqueue that list; this entry runs the same argument checks and
 * the same planner as nint_seq_fwd (bwd = 0) / nint_seq_bwd (bwd = 1: the BPTT chain, without the weight-gradient
 * reductions behind it: nint_debug_wgrad_plan) and writes one record per conv / pointwise problem in enqueue order into out[0 .. cap).  Returns the
 * number of problems of the pass (which may exceed cap) or a negative NINT_E_* code. */
enum { NINT_K_CONV_IGEMM = 0, NINT_K_CONV_LSTM_MULTI = 1, NINT_K_CONV_LSTM_MULTI8 = 2, NINT_K_CONV_BWD_MULTI = 3,
       NINT_K_CONV_BWD_MULTI8 = 4, NINT_K_CONV_DGRAD_MULTI8 = 5, NINT_K_STENCIL = 6, NINT_K_TINY = 7, NINT_K_POINTWISE = 8 };
enum { NINT_OP_GATE = 0, NINT_OP_DGRAD = 1 /* conv backward-data, also with the layer below's pointwise backward on its x columns */,
       NINT_OP_FUSED = 2 /* conv backward-data + the layer's own pointwise backward */, NINT_OP_POINTWISE = 3 };
typedef struct nint_launch_rec {
  int32_t index;            /* enqueue index: the problems of one merged grid share it */
  int32_t bwd;              /* 0 = forward pass, 1 = BPTT */
  int32_t op, layer, t;     /* NINT_OP_*; t = the time step of the launch's own data */
  int32_t kernel;           /* NINT_K_*: the host kernel that carries the problem */
  int32_t dtype;
  /* the conv_igemm body (0 in all of them for the stencil, dense-K and pointwise kernels, which have none): */
  int32_t epi, wn, wk, ntw, mt;   /* epilogue (0 gates, 1 backward-data, 2 backward-data + pointwise backward), waves along N / K,
                                   * n-tiles per wave, tile rows */
  int32_t strip;            /* 1: the leftover rows run as merged tiles of mt/2 rows x 32 pixels */
  int32_t gx, gy;           /* the problem's own grid: pixel tiles x column groups */
  int32_t nt_begin;         /* first n-tile it computes */
} nint_launch_rec;
int nint_debug_seq_plan(const nint_seq* s /*host*/, int bwd, nint_launch_rec* out /*host*/, int cap);
/* ... of a closed-loop window (nint_seq_fwd_closed / nint_seq_bwd_closed).  Conv / pointwise problems only, as above: their
 * `index` counts the feedback launches in between, as it counts the halo wraps of cyclic longitude. */
int nint_debug_seq_plan_closed(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, int bwd, nint_launch_rec* out /*host*/,
                               int cap);
/* ... of nint_seq_bwd_rollout (the BPTT chain; the nint_feedback_grad pointers are made up inside: the plan reads none).  `index`
 * counts the feedback backward launches in between. */
int nint_debug_seq_plan_rollout(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, nint_launch_rec* out /*host*/, int cap);
/* ... of a pass under a feed mask.  dir: 0 = nint_seq_fwd_sampled, 1 = the plain backward entry (which refuses every fed window,
 * as nint_seq_bwd_closed does), 2 = nint_seq_bwd_rollout_sampled; any other value: NINT_E_ARG.  A step without a fed image
 * shows as a missing feedback launch in `index`. */
int nint_debug_seq_plan_sampled(const nint_seq* s /*host*/, const nint_feedback* fb /*host*/, const nint_feedback_mask* fm /*host*/,
                                int dir, nint_launch_rec* out /*host*/, int cap);
/* The merged-grid rule alone, for tests (host arithmetic only): the NINT_K_* kernel that would carry n independent launches of
 * the conv_igemm bodies shapes[5 * i .. 5 * i + 5) = (epi, wn, wk, ntw, mt) as ONE grid, with_pw != 0: together with one
 * pointwise backward pass -- or NINT_E_SHAPE where no merged kernel holds them all (also n outside [1, 4], or a tuple that is
 * no body).  It is the planner's own choice: the drivers' plans go through the same function. */
int nint_debug_multi_carrier(const int32_t* shapes /*host, n x 5*/, int n, int with_pw);
/* The weight-gradient plan of ONE layer, for tests and tools (host arithmetic only, like nint_debug_seq_plan): the planner of
 * nint_conv_wgrad / nint_seq_bwd run for N images, the h source skipping the first h_skip of them, against a made-up workspace
 * of exactly nint_wgrad_workspace_bytes.  Returns NINT_OK or the planner's own NINT_E_* code (*out is then unspecified). */
typedef struct nint_wgrad_src_rec {       /* one source (x or h) of a launch */
  int32_t CB, JG, TG;                     /* channel blocks, columns per block slab (incl. the db column), column groups */
  int32_t nblk, ntiles, tiles_per_split, want_db;
  int32_t is_h;
  int64_t off;                            /* its split-K slabs: float offset from the workspace base */
} nint_wgrad_src_rec;
typedef struct nint_wgrad_launch_rec {
  int32_t family;                         /* waves per workgroup: 4 (wgrad_kernel) or 8 (wgrad_wide_kernel) */
  int32_t KS, NTC, JW, KX;                /* the instance: kernel size, channel tiles per block (8-wave: per workgroup),
                                           * columns per wave (8-wave: 0), horizontal taps */
  int32_t nparts;                         /* sources in this launch: src[0 .. nparts) */
  int32_t gx, gy, block, lds;             /* grid (gx = splits), threads, dynamic LDS bytes */
  nint_wgrad_src_rec src[2];
} nint_wgrad_launch_rec;
typedef struct nint_wgrad_plan_rec {
  int32_t n_launch, n_fold;
  int32_t fold_grid, fold_block;          /* the one launch that folds every slab */
  nint_wgrad_launch_rec launch[2];
  struct { int32_t blk_begin, splits, waves; } fold[2];
} nint_wgrad_plan_rec;
int nint_debug_wgrad_plan(const nint_layer* ly, const nint_geom* g, int dtype, int N, int h_skip, int n_cu,
                          nint_wgrad_plan_rec* out /*host*/);

/* ---- 1x1 head (model.py:251,274) ------------------------------------------------------------ */
/* ONE rule decides which arithmetic every head entry below runs.  The "staged" bodies (weights zero-padded to [O][CHV] in
 * LDS, CHV = 32 / 64 / 128 by Chp, the channels of a pixel in registers) hold a head with
 *     Chp <= 128,  Chp % 4 == 0  and  (O * CHV + min(O, 64) * 64) * 4 + 8192 <= 160 KiB
 * -- the weight image, one 64-output chunk of d loss / d pred of 64 pixels and 8 KiB of static LDS: what the fused passes
 * keep in a CU's LDS (above 64 KiB with the dynamic-LDS opt-in).  nint_head_fwd[_seq] and the dh pass of nint_head_bwd[_seq]
 * run their staged kernels under exactly this condition, although they keep the weights alone, and generic one-thread-per-
 * element kernels (a plain chain over c < Ch: other roundings) beyond it; the fused entries (nint_head_loss_fused,
 * nint_head_loss_seq_fused, their _weighted twins, nint_head_skill_accum) return NINT_E_SHAPE beyond it.  So wherever a fused
 * entry runs, its separate launches run the same bodies, and "bit for bit" below holds for every shape a fused entry accepts
 * (O = 200 on 128 channels included: a 100 KiB weight image).
 * The staged dot product (normative; every staged body -- nint_head_fwd[_seq], every fused loss entry, nint_head_skill_accum --
 * gives these bits): in f32, the accumulator starts from b[o] (0 without a bias); the CHV staged channels (zeros past Ch) join
 * it in channel order; each of the first CHV - 12 by one fused multiply-add, each of the last 12 as a rounded product
 * followed by a rounded add.  (The library's source writes out the unfused tail; that the other products are fused is the
 * compiler's contraction, held by the bit tests of tests/, which carry data in the last 12 staged channels at every CHV.) */
/* pred (N,O,H,W) f32 = w (O,Ch) . h + b  from halo-slab images [n0, n0+N) */
int nint_head_fwd(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                  float* pred, const nint_geom* g, int dtype, void* stream);
/* dh (compact ET [N][H][W][Chp], overwritten) ; dw (O,Ch), db (O) overwritten */
int nint_head_bwd(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                  const float* dpred, void* dh, float* dw, float* db, const nint_geom* g, int dtype,
                  float* scratch, size_t scratch_bytes, void* stream);
/* scratch (may be NULL): >= 256*O*(Ch+1) floats enables the tiled two-stage weight-gradient path. */
/* nint_head_bwd with nint_seq.accumulate's switch for dw / db: accumulate = 0 is nint_head_bwd (which calls this entry with 0);
 * accumulate = 1 writes dw[i] = dw[i] + s and db[o] = db[o] + s, one f32 add by the thread that owns the element in the last
 * stage of whichever weight-gradient path the shape takes (the one-workgroup-per-output kernel or the fold of the tiled
 * paths' partials), s being the sum that 0 stores.  dh is overwritten either way.  Any other value: NINT_E_ARG. */
int nint_head_bwd_acc(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w,
                      const float* dpred, void* dh, float* dw, float* db, int accumulate, const nint_geom* g, int dtype,
                      float* scratch, size_t scratch_bytes, void* stream);

/* The head over the WHOLE sequence (model.py:264,272,274 commented code, test.ipynb:273): the top layer's h slab holds h_t in
 * slot t+1, image (t+1)*B + b; seq / dseq are (B, T*O, H, W) f32 contiguous with channel t*O + o (torch.cat of the per-step
 * head outputs on the channel axis).  The (b, t) <-> image index math is done inside the kernels.
 * nint_head_fwd_seq: one launch; per element the arithmetic of nint_head_fwd in the same order (= T calls of it, bit for bit). */
int nint_head_fwd_seq(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                      float* seq, const nint_geom* g, int dtype, void* stream);
/* The FEEDBACK step of the closed-loop forward (nint_seq_fwd_closed), by itself: the head of images [n0, n0 + N)
 * of the top layer's halo slab, rounded once to ET (round to nearest even, as the pack entries round) and stored into channels
 * [c0, c0 + O) of images [x_n0, x_n0 + N) of the input halo slab xs (Cx channels padded to Cxp per pixel).  The f32 value is
 * nint_head_fwd's bit for bit: the same staged body pieces in the same order.
 *   xfold_k = 0   plain slab: channels [c0, c0 + O) of the INTERIOR pixels are stored and nothing else -- no halo pixel, no
 *                 slack column, no pad channel, no other channel.  (Cyclic longitude: the halo columns of these images are
 *                 the caller's to refresh; nint_seq_fwd plans a wrap launch right behind.)  lon_cyclic is only checked.
 *   xfold_k = k   horizontally folded slab (nint_layer.xfold): slab channel kx*Cx + c0 + o of pixel x receives the value of
 *                 pixel x + kx - k/2 -- 0 outside the image, or that pixel mod W with lon_cyclic -- exactly what
 *                 nint_pack_btchw_xfold[_cyclic] stores for the same f32 value.  Every other channel stays.
 * One workgroup per image row: the row's predictions are formed once, staged in LDS, and every destination pixel gathers
 * its own; stores go out in whole dwords wherever both halves are fed.
 * Shapes: the staged head only.  Where the rule above (Chp <= 128, ...) does not hold, or the row's predictions (W * O f32)
 * do not fit beside the weights in 160 KiB of LDS: NINT_E_SHAPE before any launch (nint_seq_fwd: before anything is enqueued).
 * NINT_E_ARG before any launch: a NULL h_slab / w / xs_slab / g; N, O, Ch < 1; Chp < Ch or not a multiple of KC; c0 < 0 or
 * c0 + O > Cx; xfold_k negative or even (1 is a plain slab); Cxp < Cx (plain) or < xfold_k * Cx (folded), or a pixel of Cxp
 * elements that is no multiple of 16 bytes;
 * lon_cyclic not 0 / 1, or 1 with g->W < g->P or g->W < xfold_k / 2; a bad dtype or geometry.  NINT_E_ALIGN: a slab that is
 * not 16-byte aligned. */
int nint_head_feedback(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                       void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g,
                       int dtype, void* stream);
/* The adjoint of nint_head_feedback (nint_seq_bwd_rollout), by itself.  dx: ET compact [..][H][W][Cxp], the
 * gradient of the input slab (plain or folded) of a fed step, images [dx_n0, dx_n0 + N); dpred: f32 [..][O][H][W], images
 * [p_n0, p_n0 + N), the cotangent of the head outputs that were fed; dh: ET compact [..][H][W][Chp], images [dh_n0, dh_n0 + N).
 * One thread per pixel, a fixed sequence:
 *     xi[o]  = dx[pixel][c0 + o]  (plain)  |  sum over kx = 0 .. k-1, in that order from 0.f, of
 *              dx[pixel x - kx + k/2][kx*Cx + c0 + o], terms outside the row dropped or taken mod W with lon_cyclic (folded:
 *              the arithmetic of nint_unfold_dx[_cyclic])
 *     g[o]   = dpred[o] + xi[o]  in f32, stored back into dpred by the one thread that owns the element
 *     dh[c]  = sum_o w[o][c] * g[o]  with the staged body of nint_head_bwd's dh pass, rounded to ET; the whole Chp record is stored
 * so dpred and dh equal nint_unpack_compact / nint_unfold_dx[_cyclic] of the fed channels -> f32 add -> nint_head_bwd(dh only)
 * bit for bit.  No store outside those dpred images and dh images; nothing else of dx is read than the fed channels.
 * Shapes: exactly nint_head_feedback's (NINT_E_SHAPE beyond).  NINT_E_ARG / NINT_E_ALIGN before any launch: its checks on
 * (N, O, Ch, Chp, Cx, Cxp, c0, xfold_k, lon_cyclic, g, dtype), a NULL dx / dpred / dh / w, a negative image index; dx or dh
 * not 16-byte, dpred not 4-byte aligned. */
int nint_head_feedback_bwd(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch, int Chp, int O,
                           const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, const nint_geom* g, int dtype,
                           void* stream);
/* The two launches above under a FEED MASK (scheduled sampling).  fed: HOST bytes, one per image, each 0 or
 * 1; it reaches the kernel by value, as one 64-bit word (bit i = image i of the N), so N <= 64.
 * nint_head_feedback_sel: the workgroups of an unfed image return before they touch anything -- no byte of that xs image
 *     changes; a fed image receives what nint_head_feedback stores.  No image fed: no launch.
 * nint_head_feedback_bwd_sel: a fed image behaves as in nint_head_feedback_bwd; for an unfed image xi is 0 without a read of
 *     dx, dpred is not stored (its bits stay) and dh = W^T dpred is still written as the whole Chp record, which is
 *     nint_head_bwd(dh only) of that image bit for bit.  A mask of zeros is legal.
 * Arguments, checks and their order: those of nint_head_feedback / nint_head_feedback_bwd; then NINT_E_ARG for a NULL fed or
 * a byte other than 0 or 1, then NINT_E_SHAPE for N > 64; all before any launch. */
int nint_head_feedback_sel(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                           void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic,
                           const uint8_t* fed /*host, N bytes*/, const nint_geom* g, int dtype, void* stream);
int nint_head_feedback_bwd_sel(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch, int Chp,
                               int O, const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic,
                               const uint8_t* fed /*host, N bytes*/, const nint_geom* g, int dtype, void* stream);
/* ---- RESIDUAL HEAD: the head predicts the tracer's tendency ------------------------------------------------
 * p = fl32( d + base ): d is the staged head's f32 dot product as defined above (accumulator from b[o], same order, same fused /
 * unfused tail), base the value STORED in the input halo slab xs at the pixel's feedback channel c0 + o, converted to f32 exactly
 * (a bf16 value is exact in f32).  A horizontally folded slab (nint_layer.xfold) is read at the pixel's own copy, slab channel
 * (k/2)*Cx + c0 + o.  ONE f32 add behind the dot product; the base never enters the accumulator.  Everything downstream -- the
 * loss, d loss / d pred, dL/dh, the value fed to the next step -- sees p.  The base is read from interior pixels only: no halo,
 * no slack, no pad channel, and nothing of xs but the O channels of every pixel the twin's body visits.
 * Every _res entry below takes its twin's arguments, runs its twin's body (ONE body per kernel: the operand is a template
 * parameter of it, and the instantiation without a base is the kernel the twin has always launched) and makes its twin's checks
 * in its twin's order, then the base's: NINT_E_ARG for x_n0 < 0, Cx < 1, c0 < 0 or c0 + O > Cx, xfold_k negative or even, Cxp
 * below Cx (xfold_k * Cx for a folded slab) or a pixel of Cxp elements that is no multiple of 16 bytes; NINT_E_ALIGN for an xs
 * that is not 16-byte aligned.  The memory contracts are the twins': no kernel stores anywhere its twin does not.
 * The twins themselves are the _res entries with a NULL base.
 * Gradients (straight-through, as in nint_seq_bwd_rollout): d p / d d = 1, so dpred, dh = W^T dpred, dw and db are formed from
 * the same dpred by the same entries; d p / d base = 1, which is the caller's to add where the base was its own input
 * (SeqEngine.backward) and nint_head_feedback_bwd_res's where the base was a fed value. */
typedef struct nint_head_base {   /* host; xs == NULL (or a NULL pointer to the struct): no base -- the twin entry, bit for bit */
  const void* xs;                 /* ET input halo slab */
  int32_t x_n0;                   /* image of xs that pairs with the first head image (SEQ entries: image t*B + b pairs with h slot t+1) */
  int32_t Cx, Cxp, c0, xfold_k;   /* as in nint_head_feedback */
} nint_head_base;
/* nint_head_fwd / nint_head_fwd_seq with the base added.  Staged heads only: where the rule above the head entries does not
 * hold, the generic wide kernels have no residual form and the entry returns NINT_E_SHAPE before any launch (with a base). */
int nint_head_fwd_res(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b, float* pred,
                      const nint_geom* g, int dtype, const nint_head_base* base /*host*/, void* stream);
int nint_head_fwd_seq_res(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b, float* seq,
                          const nint_geom* g, int dtype, const nint_head_base* base /*host*/, void* stream);
/* nint_head_feedback[_sel] with the base: image x_n0 + i of xs receives round_ET( dot + base ), the base read from image
 * base_n0 + i of the same slab (the step before), the same pixel's own channel as above.  base_n0 < 0: no base.  fed (HOST, N
 * bytes): NULL = every image, else the mask of nint_head_feedback_sel (its checks, its behaviour: N <= 64, an unfed image keeps
 * every byte, no image fed = no launch).  The base is gathered by the thread that forms the pixel's dot products, in the pass
 * that loads h: no second sweep over the row.  Checks: nint_head_feedback's, then NINT_E_ARG where the images
 * [base_n0, base_n0 + N) and [x_n0, x_n0 + N) overlap, then the mask's. */
int nint_head_feedback_res(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                           void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, int base_n0,
                           const uint8_t* fed /*host, NULL = every image*/, const nint_geom* g, int dtype, void* stream);
/* nint_head_feedback_res with noise on the stored value (nint_feedback_noise): image x_n0 + i draws for (step, lane0 + i).
 * fn == NULL or fn->sigma == NULL: nint_head_feedback_res.  Checks: its checks, then NINT_E_ALIGN for a sigma that is not
 * 4-byte aligned. */
int nint_head_feedback_noise(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                             void* xs_slab, int x_n0, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, int base_n0,
                             const uint8_t* fed /*host, NULL = every image*/, const nint_geom* g, int dtype, void* stream,
                             const nint_feedback_noise* fn /*host*/, uint32_t step);
/* nint_head_feedback_bwd[_sel] with the skip term: on a fed image g = fl32( fl32(dpred + xi) + dpred[pnext_n0 + i] ), stored
 * back and handed to the dh body; an unfed image as in nint_head_feedback_bwd_sel.  The images [pnext_n0, pnext_n0 + N) of the
 * dpred slab -- the total cotangent of the fed step's own prediction -- are read, never written, and must lie apart from
 * [p_n0, p_n0 + N) (else NINT_E_ARG).  pnext_n0 < 0: no such term.  fed: as above (a mask of zeros is legal). */
int nint_head_feedback_bwd_res(const void* dx, int dx_n0, float* dpred, int p_n0, void* dh, int dh_n0, int N, int Ch, int Chp,
                               int O, const float* w, int Cx, int Cxp, int c0, int xfold_k, int lon_cyclic, int pnext_n0,
                               const uint8_t* fed /*host, NULL = every image*/, const nint_geom* g, int dtype, void* stream);
/* dseq (B, T*O, H, W) and dpred_last (B, O, H, W: the cotangent of pred = head(h_{T-1}), added to step T-1 inside the
 * kernels); either may be NULL, not both.  dh_seq: compact ET [T*B][H][W][Chp], image t*B+b, padding channels zero
 * (nint_seq.dh_seq; may be NULL: not written); dw (O,Ch), db (O): summed over all T*B images in a fixed order (overwritten;
 * both NULL: not computed).  scratch as in nint_head_bwd. */
int nint_head_bwd_seq(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* dseq,
                      const float* dpred_last, void* dh_seq, float* dw, float* db, const nint_geom* g, int dtype,
                      float* scratch, size_t scratch_bytes, void* stream);
/* nint_head_bwd_seq with the same switch (nint_head_bwd_seq calls it with 0) */
int nint_head_bwd_seq_acc(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* dseq,
                          const float* dpred_last, void* dh_seq, float* dw, float* db, int accumulate, const nint_geom* g,
                          int dtype, float* scratch, size_t scratch_bytes, void* stream);

/* ---- INPUT NOISE: seeded Gaussian noise on a span of the input's channels, drawn on the device ---------------
 * THE RULE.  For the noise span, channels [c0, c0 + n) of the model's input, the element at channel offset o in [0, n), pixel
 * (y, x) of the H x W model grid, window step t and batch lane b draws from one Philox4x32-10 block (Salmon et al., SC'11):
 *     ctr = (y*W + x,  o / 4,  step0 + t,  lane0 + b)      key = (seed, draw)        all u32, sums mod 2^32
 *     (w0, w1, w2, w3) = philox4x32_10(ctr, key)
 *     pair A = (w0, w1) serves o % 4 = 0, 1;   pair B = (w2, w3) serves o % 4 = 2, 3;   (wa, wb) the pair's words
 *     u  = (float(wa >> 9) + 0.5f) * 2^-23          in [2^-24, 1 - 2^-24]: never 0, exact in f32
 *     a  = float(wb >> 8) * 2^-23                   in [0, 2), exact
 *     r  = sqrtf(-2.f * logf(u));  (s, c) = sincospif(a)        the precise forms, never the fast-math ones
 *     z  = r * c  (even o)   |   r * s  (odd o)                 |z| <= 5.77
 *     stored' = round_ET( __fadd_rn( f32(stored), __fmul_rn(sigma[o], z) ) )
 * The product and the sum are two f32 operations, never one FMA: given z, a float32 model reproduces the update bit for bit.
 * round_ET is the pack entries' round-to-nearest-even to the storage type (the identity in f32).  A channel with sigma[o] == 0
 * is SKIPPED, not multiplied: its bytes stay, -0.0 included.  The noise of an element is a pure function of (seed, draw, lane,
 * step, o, pixel): whatever launch produces it -- the sweep or the recompute of a segmented window, a plain or a folded slab,
 * any batch split over ranks -- it is the same number.
 *
 * nint_input_noise applies the rule to images [x_n0, x_n0 + T*B) of an input halo slab, image order t*B + b (Cx channels
 * padded to Cxp per pixel, sigma: n DEVICE floats).  It writes exactly the bytes nint_head_feedback may write:
 *   xfold_k = 0   plain slab: channels [c0, c0 + n) of the INTERIOR pixels and nothing else -- no halo pixel, no slack column,
 *                 no pad channel, no other channel.  (Cyclic longitude: the halo columns are refreshed by the wrap launch that
 *                 heads nint_seq_fwd.)  lon_cyclic is only checked.
 *   xfold_k = k   folded slab: slab channel kx*Cx + c0 + o of pixel x holds pixel x' = x + kx - k/2 and receives THAT pixel's
 *                 noisy value, keyed by x' (x' mod W with lon_cyclic); where x' lies outside the row of a zero-padded slab the
 *                 copy stays 0.  Each copy reads its own stored value: the k copies of a pixel held the same bits before, so they
 *                 hold the same bits after.
 *   bf16          every dword is read, merged and stored whole by ONE lane, also a dword that holds one span element and one
 *                 foreign one (an odd first channel, an odd n): no two lanes write halves of one dword.
 * One Philox block feeds four channels of a pixel; a workgroup forms a row's addends once, stages them in LDS, and every fold
 * copy gathers its own.  Plain vector loads and stores only.
 * NINT_E_ARG before any launch, in nint_head_feedback's order: a NULL xs_slab / sigma / g, x_n0 < 0; B, T, n, Cx < 1; a bad dtype
 * or geometry; c0 < 0 or c0 + n > Cx; xfold_k negative or even; Cxp < Cx (xfold_k * Cx folded) or a pixel that is no multiple
 * of 16 bytes; lon_cyclic not 0 / 1, or 1 with g->W < g->P or g->W < xfold_k / 2.  NINT_E_ALIGN: a slab that is not 16-byte
 * or a sigma that is not 4-byte aligned.  No shape limit on n, W, Cx (a span or a row too long for one staged window is cut
 * into workgroups and, in whole Philox blocks, into launches); NINT_E_SHAPE only for xfold_k > 4095. */
int nint_input_noise(void* xs_slab, int x_n0, int B, int T, int Cx, int Cxp, int c0, int n, const float* sigma /*device, n*/,
                     int xfold_k, int lon_cyclic, uint32_t seed, uint32_t draw, uint32_t step0, uint32_t lane0,
                     const nint_geom* g, int dtype, void* stream);
/* z alone, f32 [T*B][n][H][W], through the device function the slab kernel inlines: the hook that separates the generator from
 * the layout, and an ensemble caller's source of perturbations.  Only g->H and g->W are used.  NINT_E_ARG: a NULL out / g, B,
 * T, n < 1, a bad geometry; NINT_E_ALIGN: out not 4-byte aligned. */
int nint_noise_normal(float* out, int B, int T, int n, uint32_t seed, uint32_t draw, uint32_t step0, uint32_t lane0,
                      const nint_geom* g, void* stream);

/* ---- loss (train.py:102,105) ------------------------------------------------------------------ */
/* pred (N,O,H,W) f32, y (N,O,Hc,Wc) f32; crop window [oy,oy+Hc) x [ox,ox+Wc).
 * loss_out: NINT_LOSS_SCRATCH_FLOATS floats, 8-byte aligned; [0] = mean((y-p)^2) + mean(|y-p|), the
 * rest is reduction scratch (4 doubles per workgroup of the partial-sum launch, up to 1024 workgroups); dpred (N,O,H,W) = d loss / d pred (0 outside the
 * crop), may be NULL; stats (NINT_LOSS_STATS doubles, accumulated, caller zeroes): [0..4] pooled sums
 * sum (y-p)^2, sum |y-p|, sum y, sum y^2, count; [5..7] the reference's per-batch statistics: sum over calls
 * of the loss, sum over calls of sklearn-style r2_score(y, pred) of that call, number of calls -- the
 * device-side accumulators replacing loss.item() / r2_score(...cpu()) of train.py:113-117, utils.py:73-75.
 * Memory contract: loss_out of exactly NINT_LOSS_SCRATCH_FLOATS floats is enough -- no kernel stores outside
 * it, and no result depends on a byte outside it or on its prior contents. */
#define NINT_LOSS_SCRATCH_FLOATS 8194
#define NINT_LOSS_STATS 8
int nint_loss_mse_l1_crop(const float* pred, const float* y, float* dpred, float* loss_out, double* stats,
                          int N, int O, int H, int W, int oy, int ox, int Hc, int Wc, void* stream);

/* Training fast path: head forward + crop + loss + d loss/d pred + head backward-data in ONE pass over the pixels
 * (train.py:96-109 around model.py:274); the same arithmetic in the same order as nint_head_fwd ->
 * nint_loss_mse_l1_crop -> nint_head_bwd(dh).  pred is not materialised; dpred (N,O,H,W) is written for
 * nint_head_bwd(dh = NULL) to form dw / db.  Beyond the staged bodies' limit (the rule above the head entries: Chp > 128, or
 * the weight image beyond the LDS) NINT_E_SHAPE: use the three separate entries. */
int nint_head_loss_fused(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                         const float* y, float* dpred, void* dh, float* loss_out, double* stats, const nint_geom* g,
                         int oy, int ox, int Hc, int Wc, int dtype, void* stream);

/* The same over every time step: y (B, T, O, Hc, Wc) f32 (the index convention of seq, on the crop); the loss is
 * mean((y-p)^2) + mean(|y-p|) over all B*T*O*Hc*Wc elements (= nint_loss_mse_l1_crop(seq, y, N = B, O' = T*O)), stats
 * accumulate over all elements of the call.  dh_seq: compact ET [T*B][H][W][Chp], image t*B+b (nint_seq.dh_seq); dpred
 * (T*B, O, H, W) f32, image t*B+b: what nint_head_bwd(h_slab, n0 = B, N = T*B, dh = NULL) reduces to dw / db.  Same limits
 * as nint_head_loss_fused (NINT_E_SHAPE beyond: nint_head_fwd_seq + nint_loss_mse_l1_crop + nint_head_bwd_seq). */
int nint_head_loss_seq_fused(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                             const float* y, float* dpred, void* dh_seq, float* loss_out, double* stats, const nint_geom* g,
                             int oy, int ox, int Hc, int Wc, int dtype, void* stream);

/* ---- the same loss with a weight per crop cell: cos-latitude area weights, masks, or their product ---------- */
/* wgt: f32 [Hc][Wc] on the device, 4-byte aligned, shared by every sample, output and time step of the call; every value
 * finite and >= 0, at least one > 0 (the caller validates the values: the library reads them on the device only).  A mask is
 * a map of 0 / 1; cos-latitude weights are cos(deg2rad(lat[cy])) along row cy.  wsum: the f64 sum of the map AS STORED in
 * f32, formed on the host by the caller; cnt = N * O * wsum (T * B * O * wsum for the sequence entry) stands where the
 * unweighted entries have N * O * Hc * Wc.
 *   per crop cell, w = wgt[cy][cx], d = p - y in f32 (as in the unweighted entries):
 *   loss   = (sum w d^2) / cnt + (sum w |d|) / cnt, the sums in f64 with (double)w, the same two-stage fixed-order
 *            reduction as the unweighted entries
 *   dpred  = (float)(((2.0 * d + sgn(d)) * (1.0 / cnt)) * (double)w), evaluated left to right in f64, rounded once;
 *            +0 outside the crop
 *   w == 0 : the cell is skipped -- target and prediction enter no sum, dpred = +0; a NaN target under a zero weight is
 *            harmless (this is how missing data is masked)
 *   stats  : [0..4] += sum w d^2, sum w |d|, sum w y, sum w y^2, cnt; [5] += loss; [6] += the weighted R2
 *            1 - S0 / (S3 - S2^2 / cnt) = sklearn r2_score(y, p, sample_weight = w), the constant-target convention of
 *            the unweighted entries applied to the weighted ss_tot; [7] += 1
 * wgt = 1 everywhere and wsum = Hc * Wc give the unweighted entries' results bit for bit.
 * Each entry mirrors its twin above (arguments, limits, checks before any launch, the fused entries bit-identical to
 * nint_head_fwd[_seq] -> nint_loss_mse_l1_crop_weighted -> nint_head_bwd[_seq]); in addition wgt == NULL, !(wsum > 0) or a
 * non-finite wsum: NINT_E_ARG; wgt not 4-byte aligned: NINT_E_ALIGN.  The map is read from global memory: no LDS on top. */
int nint_loss_mse_l1_crop_weighted(const float* pred, const float* y, const float* wgt, double wsum, float* dpred,
                                   float* loss_out, double* stats, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc,
                                   void* stream);
int nint_head_loss_fused_weighted(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                                  const float* y, const float* wgt, double wsum, float* dpred, void* dh, float* loss_out,
                                  double* stats, const nint_geom* g, int oy, int ox, int Hc, int Wc, int dtype, void* stream);
int nint_head_loss_seq_fused_weighted(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                      const float* y, const float* wgt, double wsum, float* dpred, void* dh_seq,
                                      float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc, int Wc,
                                      int dtype, void* stream);

/* ---- the configurable loss: an MSE / L1 / Huber mix with a weight per output and per step -------------------- */
/* The twins of the three entries above and of their _weighted forms with the per-element term and weight opened up:
 *     loss = a * mean_w(d^2) + b * mean_w(|d|) + c * mean_w(H(d)),     H = torch.nn.HuberLoss(delta = delta),
 * a weighted mean whose weight is the product of the cell's (the map of the _weighted entries, optional) and the output's
 * (ow, optional; in the sequence entry one weight per (step, output): spin-up steps are discounted or dropped there).
 * nint_loss_spec is plain data read on the host at the call; ow is read on the device. */
typedef struct nint_loss_spec {
  double mse, l1, huber;  /* coefficients a, b, c: finite, >= 0, not all zero */
  double delta;           /* Huber threshold: finite, > 0 when huber != 0; not read otherwise */
  const float* ow;        /* device f32 [now], 4-byte aligned: weight per output, finite and >= 0 (the caller validates the
                           * values); NULL = 1 */
  int32_t now;            /* 0 with ow == NULL; else O (plain / fused entry) or T*O (sequence entry, index t*O+o) */
  double osum;            /* f64 sum of ow AS STORED in f32, formed by the caller; not read with ow == NULL */
} nint_loss_spec;
/* Per crop element of sample n (sequence entry: of step t of sample b), output o, cell (cy, cx):
 *   w  = wgt[cy][cx], or 1 without a map (wgt == NULL; wsum is then not read);  q = ow[o] (ow[t*O+o] in the sequence entry),
 *        or 1 with ow == NULL;  Wd = (double)q * (double)w, exact in f64;  d = p - y in f32, as in the entries above
 *   cnt    = N * osum * wsum, evaluated left to right in f64 with N as a double (sequence entry with ow: B * osum * wsum).
 *            Without ow, O stands for osum (sequence entry: (T*B) * O * wsum); without a map, Hc * Wc (an exact integer)
 *            for wsum: the expressions of the entries above.
 *   H(d)   = 0.5*d*d if |d| <= delta, else delta*(|d| - 0.5*delta), in f64 from (double)d
 *   C(d)   = d > delta ? delta : (d < -delta ? -delta : d): dH/dd, written as comparisons so that a NaN d stays NaN
 *            (fmin / fmax would return delta)
 *   S2 = sum Wd d^2, S1 = sum Wd |d|, SH = sum Wd H(d): f64, every term joined to its running sum by one fused multiply-add
 *            fma(Wd, term, S) (so do the entries above), the two-stage fixed-order reduction of those entries with a fifth
 *            partial for SH; SH is formed only when c != 0
 *   loss   = a*(S2/cnt) + b*(S1/cnt) + c*(SH/cnt), left to right, each product and sum rounded.  A coefficient that is
 *            exactly 0 takes its term OUT instead of multiplying it by 0: with b alone an inf prediction gives loss = +inf,
 *            not 0 * inf = NaN, and a term nobody asked for cannot poison the loss.
 *   dpred  = (float)(((a*(2.0*d) + b*sgn(d) + c*C(d)) * (1.0/cnt)) * Wd), f64, left to right, each operation rounded (no
 *            fused multiply-add), terms omitted as in the loss, rounded to f32 once; sgn(0) = sgn(NaN) = 0; +0 outside the crop
 *   Wd == 0: the element is skipped -- its target is not read (a NaN target is harmless), it enters no sum, dpred = +0
 *   stats  : [0..4] += S2, S1, sum Wd y, sum Wd y^2, cnt, whatever the coefficients (the R2 needs them); [5] += loss;
 *            [6] += the weighted R2 of the _weighted entries with Wd for w; [7] += 1
 * Spec (1, 1, 0) with ow == NULL gives the bits of the unweighted entry (no map) and of the _weighted entry (with one):
 * loss_out[0], dpred, dh and all eight stats; so does an all-ones ow with osum = O (T*O).  The spec entries always run this
 * general body; the fused ones are bit-identical to nint_head_fwd[_seq] -> nint_loss_crop_spec -> nint_head_bwd[_seq]
 * (sequence: N = B, O' = T*O and the same ow).
 * loss_out: NINT_LOSS_SPEC_SCRATCH_FLOATS floats, 8-byte aligned ([0] = loss, then 5 doubles per workgroup).
 * Checks before any launch -- NINT_E_ARG: the twin's argument checks; spec == NULL; a coefficient negative or not finite, or
 * all three zero; huber != 0 with !(delta > 0) or a non-finite delta; ow with now != O (T*O), !(osum > 0) or a non-finite
 * osum; now != 0 with ow == NULL; a map with !(wsum > 0) or a non-finite wsum.  NINT_E_ALIGN: the twin's alignment checks;
 * ow not 4-byte aligned.  NINT_E_SHAPE: the fused entries, exactly where their twins return it.  ow and the map are read
 * from global memory: no LDS on top of the twins'.
 * Memory contract: loss_out of exactly NINT_LOSS_SPEC_SCRATCH_FLOATS floats is enough -- no kernel stores
 * outside it, and no result depends on a byte outside it or on its prior contents. */
#define NINT_LOSS_SPEC_SCRATCH_FLOATS 10242
int nint_loss_crop_spec(const float* pred, const float* y, const float* wgt, double wsum, const nint_loss_spec* spec,
                        float* dpred, float* loss_out, double* stats, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc,
                        void* stream);
int nint_head_loss_fused_spec(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                              const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred, void* dh,
                              float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc, int Wc, int dtype,
                              void* stream);
int nint_head_loss_seq_fused_spec(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                  const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred,
                                  void* dh_seq, float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc,
                                  int Wc, int dtype, void* stream);
/* The two fused _spec entries for the RESIDUAL HEAD (nint_head_base above): the same pass with p = dot + base in the place of
 * the dot product -- the loss, d loss / d pred and dL/dh = W^T dpred are formed from it; bit-identical to
 * nint_head_fwd[_seq]_res -> nint_loss_crop_spec -> nint_head_bwd[_seq].  They keep the optional map and the spec and always
 * run the general body; the plain and _weighted forms need no residual twin (the default spec reproduces their bits).  Checks:
 * the _spec entry's in its order, then the base's.  A NULL base (or xs): the _spec entry, which calls these. */
int nint_head_loss_fused_res(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                             const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred, void* dh,
                             float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc, int Wc, int dtype,
                             const nint_head_base* base /*host*/, void* stream);
int nint_head_loss_seq_fused_res(const void* h_slab, int B, int T, int Ch, int Chp, int O, const float* w, const float* b,
                                 const float* y, const float* wgt, double wsum, const nint_loss_spec* spec, float* dpred,
                                 void* dh_seq, float* loss_out, double* stats, const nint_geom* g, int oy, int ox, int Hc,
                                 int Wc, int dtype, const nint_head_base* base /*host*/, void* stream);

/* ---- evaluation: skill sums (test.ipynb:377-385, :462-485, :605, :630, :684-693, :796-803) ------------ */
/* Everything the analysis notebook derives from the gathered test-period predictions -- one R2 per window, one R2 per grid
 * cell over time, time-mean maps, cos-latitude weighted means -- follows from running f64 sums, formed on the device in one
 * pass and read once (inference.skill_from_sums turns them into the report).  Evaluation runs in z-score units.
 *   pix     [nslots][NINT_SKILL_PIX][O][Hc][Wc] f64, ACCUMULATED (the caller zeroes it once).  slot[n] (host) picks the
 *           accumulator set of sample n: the slots partition the samples (by month, say), a union is the sum of its slots'
 *           planes; slot[n] = -1 leaves sample n out of the maps (its `sample` row is still written).  slot == NULL: all 0.
 *   sample  [N][O][NINT_SKILL_SAMPLE] f64, OVERWRITTEN: the sums of each (sample, output) over the crop; row_w (device,
 *           [Hc] f64, NULL = 1) weights the rows of the last two (cos latitude, test.ipynb:796).  (f64: weights rounded
 *           to f32 would put the weighted means 5e-9 relative from the notebook's f64 expression.)
 *   scratch nint_skill_scratch_bytes(N, O, Hc, Wc) bytes, 8-byte aligned: the per-wave partial rows of `sample`.
 * d = (double)p - (double)y, products and sums in f64.  No atomics: one thread owns a (slot, o, cy, cx) cell for the whole
 * call and adds the call's samples in order n = 0, 1, ..., so pix is bit-identical run to run and under any split of the
 * same samples into consecutive calls; a sample's row is reduced by a tree that depends on (O, Hc, Wc) only, so it does not
 * depend on N or on the sample's position in the call either.  N beyond NINT_SKILL_MAX_N is split internally.
 * NINT_E_ARG: a NULL pix / sample / y / scratch, a scratch that is too small, nslots < 1, a slot outside [-1, nslots), a
 * crop outside the grid, a bad dtype; NINT_E_ALIGN: pix / sample / scratch not 8-byte, h_slab not 16-byte aligned --
 * all before any launch. */
#define NINT_SKILL_PIX 5      /* f64 planes per slot: sum y, sum p, sum y^2, sum p^2, sum (y-p)^2 */
#define NINT_SKILL_SAMPLE 8   /* f64 per (sample, output): sum (y-p)^2, sum |y-p|, sum y, sum y^2, sum p, sum p^2,
                                 sum row_w*y, sum row_w*p */
#define NINT_SKILL_MAX_N 64   /* samples per launch; larger N is split internally, as NINT_PRE_MAX_B is */
/* Memory contract: a scratch of exactly nint_skill_scratch_bytes is enough (N beyond NINT_SKILL_MAX_N
 * included) -- no kernel stores outside it, and no result depends on a byte outside it or on its prior contents. */
size_t nint_skill_scratch_bytes(int N, int O, int Hc, int Wc);            /* host arithmetic only */
/* pred (N,O,H,W) f32 already in memory; y (N,O,Hc,Wc) f32 and the crop window as in nint_loss_mse_l1_crop */
int nint_skill_accum(const float* pred, const float* y, const int32_t* slot /*host, N entries, or NULL = all 0*/,
                     int nslots, const double* row_w /*device [Hc] or NULL = 1*/, double* pix, double* sample,
                     double* scratch, size_t scratch_bytes, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc,
                     void* stream);
/* fast path: the 1x1 head on halo-slab images [n0, n0+N) + crop + the same accumulation in one pass; pred never goes to
 * memory unless pred_out (N,O,Hc,Wc) is given (= the crop of nint_head_fwd bit for bit).  pix and sample equal nint_head_fwd
 * followed by nint_skill_accum bit for bit.  Same limits as nint_head_loss_fused, NINT_E_SHAPE beyond. */
int nint_head_skill_accum(const void* h_slab, int n0, int N, int Ch, int Chp, int O, const float* w, const float* b,
                          const float* y, const int32_t* slot /*host*/, int nslots, const double* row_w, double* pix,
                          double* sample, float* pred_out, double* scratch, size_t scratch_bytes, const nint_geom* g,
                          int oy, int ox, int Hc, int Wc, int dtype, void* stream);

/* ---- evaluation: ensemble sums -------------------------------------------------------- */
/* M member predictions of each sample against one target, in one pass over the members where they lie.  Member i of sample
 * n is an (O, H, W) f32 image at pred + sample_off[n] + i * member_stride (elements; the offsets need be neither ordered nor
 * disjoint, so the (lanes, T, O, H, W) head output of a roll-out whose lanes are start * M + member is read in place: sample
 * (start, lead j) at ((start * M) * T + spinup + j) * O*H*W, member stride T * O*H*W).  y (N,O,Hc,Wc), the crop window, slot,
 * nslots and row_w are nint_skill_accum's.
 * Per cell (sample, output, crop pixel), in f64, every product and every sum its own operation, NO division:
 *   x_i = (double)member i, t = (double)y, dM = (double)M;   S = x_0 + ... + x_{M-1} in that order;   E = S - dM*t;
 *   A = sum_i |x_i - t| and V = sum_i (dM*x_i - S)^2, i ascending;   D = sum_{i<j} |x_i - x_j|, (i, j) in lexicographic order.
 *   pix       [nslots][NINT_ENS_PIX][O][Hc][Wc] f64, ACCUMULATED: sum E^2, sum V, sum A, sum D, sum E, sum t, sum t^2 over
 *             the slot's samples; one thread owns a cell for the whole call and adds the call's samples in ascending n, so
 *             pix is bit-identical run to run and under any split of the samples into consecutive calls.
 *   sample    [N][O][NINT_ENS_SAMPLE] f64, OVERWRITTEN: sum E^2, sum V, sum A, sum D, sum row_w*E^2, sum row_w*V,
 *             sum row_w*A, sum row_w*D over the crop; the reduction tree depends on (O, Hc, Wc) only.
 *   rank_hist [nslots][O][M + 2] int64, ACCUMULATED: bin r = #{i : x_i < t} (ties go low) counts the cells of the samples
 *             with slot >= 0; bin M + 1 counts instead the cells whose target or any member is NaN (such a cell still adds
 *             what the arithmetic gives to the f64 sums: masking is the caller's, through slot = -1).  Integer atomics.
 *   mean_out  (N,O,Hc,Wc) f32 or NULL: (float)(S / dM), the one division, outside every sum.
 *   scratch   nint_ens_scratch_bytes(N, M, O, Hc, Wc) bytes, 8-byte aligned.  Memory contract: exactly that
 *             many suffice (N beyond NINT_ENS_MAX_N included), no store goes outside the named extents and no result depends
 *             on a byte the library did not write.
 * The host derives the ensemble mean's MSE (sum E^2 / M^2 / n), the mean variance (sum V / (M^2 (M-1)) / n), the CRPS
 * (fair: A/M - D/(M(M-1)); plain: A/M - D/M^2), the bias and R2 (inference.ensemble_from_sums).  The sums are additive: a
 * data-parallel reduction adds the ranks' pix and rank_hist.
 * NINT_E_ARG: a NULL pred / sample_off / y / pix / sample / rank_hist / scratch, M outside [2, NINT_ENS_MAX_M], N or O < 1,
 * a negative offset or stride, nslots < 1, a slot outside [-1, nslots), a crop outside the grid, a scratch that is too
 * small; then NINT_E_ALIGN: pix / sample / rank_hist / scratch / row_w not 8-byte, pred / y / mean_out not 4-byte aligned --
 * all before any launch. */
#define NINT_ENS_MAX_M 64
#define NINT_ENS_MAX_N 64     /* samples per launch; larger N is split internally, as NINT_SKILL_MAX_N is */
#define NINT_ENS_PIX 7        /* f64 planes per slot: sum E^2, sum V, sum A, sum D, sum E, sum t, sum t^2 */
#define NINT_ENS_SAMPLE 8     /* f64 per (sample, output) */
size_t nint_ens_scratch_bytes(int N, int M, int O, int Hc, int Wc);       /* host arithmetic only */
int nint_ens_accum(const float* pred, const int64_t* sample_off /*host, N*/, int64_t member_stride, int M, const float* y,
                   const int32_t* slot /*host, N, or NULL = all 0*/, int nslots, const double* row_w /*device [Hc] or NULL = 1*/,
                   double* pix, double* sample, int64_t* rank_hist, float* mean_out /*(N,O,Hc,Wc) or NULL*/, double* scratch,
                   size_t scratch_bytes, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc, void* stream);

/* ---- training: the almost-fair CRPS of an ensemble's member lanes --------------------------------------- */
/* The loss that couples the M members of a sample, d loss / d pred of every member and the epoch statistics, in one pass over
 * the members where they lie.  Addressing is nint_ens_accum's, once for reading and once for writing: member i of sample n is
 * the (O, H, W) f32 image at pred + pred_off[n] + i * pred_stride, its gradient image is written at dpred + dpred_off[n] +
 * i * dpred_stride (elements; host arrays of N offsets, read at the call).  So the (lanes, T, O, H, W) output of
 * nint_head_fwd_seq with lanes n*M + m is read in place -- sample (n, t) at ((n*M)*T + t) * O*H*W, member stride T * O*H*W --
 * and the roll-out slab (T*B, O, H, W) of nint_feedback_grad is written in place -- sample (n, t) at (t*B + n*M) * O*H*W,
 * member stride O*H*W.  y (N, O, Hc, Wc) f32 and the crop window as in every loss entry.
 * Weights, with nint_loss_crop_spec's conventions: wgt, the optional cell map [Hc][Wc] with its f64 sum wsum (not read
 * without a map); spec->ow, an optional DEVICE table [nrows][O] of output weights of which spec->ow_row[n] (HOST, N entries;
 * NULL: row 0) picks the row of sample n -- step weights and spin-up discounts arrive as one row per step.
 *   w = wgt[cy][cx] or 1, q = ow[ow_row[n]][o] or 1, Wd = (double)q * (double)w.
 *   spec->cnt, formed by the caller in f64: the sum of q AS STORED over the listed samples and outputs, times wsum (N * O
 *   without a table, Hc * Wc without a map).
 *   Wd == 0: the element is skipped -- its target is not read (a NaN target is harmless), it enters no sum, dpred = +0 for
 *   all M members.
 * Per cell, all in f64, every operation rounded once (no contraction); x_i = (double)member i, t = (double)y, dM = (double)M:
 *   A = sum_i |x_i - t| (i ascending);  D = sum_{i<j} |x_i - x_j| ((i, j) lexicographic);  S = x_0 + ... + x_{M-1};
 *   V = sum_i (dM*x_i - S)^2;  m = S / dM (the one division, for the statistics only);
 *   sgn(d) = d > 0 ? 1 : (d < 0 ? -1 : d): sgn(0) = 0, a NaN stays NaN;   R_i = sum_{j != i} sgn(x_i - x_j), j ascending
 *   kp = (M - 1 + alpha) / (M^2 (M - 1)), formed on the host in f64 from spec->alpha in [0, 1]: alpha = 1 the fair CRPS
 *   (kp = 1 / (M (M - 1))), alpha = 0 the plain one (1 / M^2), in between the "almost fair" mix.
 *   Over the cells of the call: SA = sum Wd*A, SD = sum Wd*D, SV = sum Wd*V, S2 = sum Wd*(m-t)^2, S1 = sum Wd*|m-t|,
 *   Sy = sum Wd*t, Syy = sum Wd*t^2 -- a fixed-order reduction without floating-point atomics: a tree per (sample, output) that
 *   depends on (H, W) only, then the (sample, output) rows in ascending order; bit-identical run to run and under any
 *   internal cut (N beyond NINT_ENS_MAX_N runs in pieces).
 *   loss    = (SA / dM - kp * SD) / cnt, left to right; loss_out[0] = (float)loss, on the device.
 *   dpred_i = (float)(((sgn(x_i - t) / dM - kp * R_i) * (1.0 / cnt)) * Wd), left to right, rounded to f32 once; +0 at every
 *             pixel outside the crop.  Whole (O, H, W) images of the M members of the listed samples are written; images of
 *             samples that are not listed are the caller's to zero.
 *   stats   : NINT_LOSS_STATS doubles, ACCUMULATED, with the ENSEMBLE MEAN m as the prediction: [0..4] += S2, S1, Sy, Syy, cnt;
 *             [5] += loss; [6] += the weighted R2 of the mean (the _spec entries' expression); [7] += 1.
 *   ens_out : NINT_ENS_LOSS_OUT doubles, ACCUMULATED: += SA, SD, SV, cnt.  Mean CRPS (SA/M - kp SD) / cnt, spread
 *             sqrt(SV / (M^2 (M-1)) / cnt), RMSE of the mean sqrt(stats[0] / stats[4]).
 *   scratch : nint_ens_loss_scratch_bytes(N, M, O, H, W) bytes, 8-byte aligned.  Memory contract: exactly that
 *             many suffice, no store goes outside the named extents and no result depends on a byte the library did not write.
 * NINT_E_ARG before any launch: a NULL pred / pred_off / dpred / dpred_off / y / spec / loss_out / stats / ens_out / scratch; M
 * outside [2, NINT_ENS_MAX_M]; N or O < 1; a negative offset or stride; alpha outside [0, 1] or not finite; !(cnt > 0) or a
 * non-finite cnt; a map with !(wsum > 0) or a non-finite wsum; ow_row (or nrows != 0) without ow, ow with nrows < 1, a row
 * outside the table; a crop outside the grid; a scratch that is too small.  Then NINT_E_ALIGN: stats / ens_out / scratch not
 * 8-byte, pred / dpred / y / wgt / ow / loss_out not 4-byte aligned. */
#define NINT_ENS_LOSS_OUT 4
typedef struct nint_ens_loss_spec {
  double alpha;           /* 1 = fair CRPS, 0 = plain, between: almost fair */
  double cnt;             /* the normaliser (above) */
  const float* ow;        /* device f32 [nrows][O], 4-byte aligned, finite and >= 0 (the caller validates); NULL = 1 */
  const int32_t* ow_row;  /* host, N entries in [0, nrows); NULL = row 0 */
  int32_t nrows;          /* rows of ow; 0 with ow == NULL */
} nint_ens_loss_spec;
size_t nint_ens_loss_scratch_bytes(int N, int M, int O, int H, int W);    /* host arithmetic only */
int nint_ens_loss(const float* pred, const int64_t* pred_off /*host, N*/, int64_t pred_stride, float* dpred,
                  const int64_t* dpred_off /*host, N*/, int64_t dpred_stride, int M, const float* y, const float* wgt, double wsum,
                  const nint_ens_loss_spec* spec, float* loss_out, double* stats, double* ens_out, double* scratch,
                  size_t scratch_bytes, int N, int O, int H, int W, int oy, int ox, int Hc, int Wc, void* stream);

/* ---- evaluation: zonal power spectra --------------------------------------------------------------------- */
/* The along-longitude power spectrum of M member predictions and of the target, their cross spectrum and the spectrum of the
 * member sum, per slot (lead time), output and wavenumber, in one pass over the members where they lie.  pred, sample_off,
 * member_stride, y (N,O,Hc,Wc), the crop window, slot, nslots and row_w are nint_ens_accum's; M lies in [1, NINT_ENS_MAX_M]
 * (M = 1: a deterministic roll-out).  K = Wc / 2 + 1 wavenumbers (integer division: an odd width has no Nyquist line).
 * The transform uses the CALLER'S table tw [Wc][2] f64 on the device -- the kernel computes no sine: for a crop row f[0..Wc)
 * converted to f64,   F_k = sum_x f[x] * (tw[j][0] + i tw[j][1]),  j = (k x) mod Wc,  0 <= k < K.
 * nint_spec_twiddles (host arithmetic only) writes tw[j] = (cos(2 pi j / Wc), -sin(2 pi j / Wc)) into a HOST array, every
 * component within 1 ulp, exactly 0 and +-1 at whole quarter turns, tw[Wc - j] = conj(tw[j]) bit for bit, no negative zero;
 * the caller uploads it once.  Any other table makes the kernel that other linear map (an integer table: exact integers).
 * With Y_k the transform of target row r, P_{i,k} that of member i, S_k = sum_i P_{i,k} and w = row_w[r] (1 without a table),
 * every row of every sample with slot s >= 0 adds to
 *   spec [nslots][NINT_SPEC_PLANES][O][K] f64, ACCUMULATED, entry (s, plane, o, k):
 *     YY: w |Y_k|^2     PP: w sum_i |P_{i,k}|^2     CR: w Re(S_k conj Y_k)     CI: w Im(S_k conj Y_k)     SS: w |S_k|^2
 * No division and no normalisation (inference.spectrum_from_sums has them).  The error power follows: sum_i |P_i - Y|^2 =
 * PP + M YY - 2 CR; of the ensemble mean: SS / M^2 + YY - 2 CR / M.  A NaN goes where the arithmetic takes it (masking is the
 * caller's: slot = -1, such a sample adds nothing and is not read).
 * THE ORDER, a function of (M, O, Hc, Wc) only; f64 throughout, contraction off except where a fused multiply-add is named:
 *   F_k: re = fma(f[x], tw[j][0], re), im = fma(f[x], tw[j][1], im), x = 0 .. Wc-1 ascending from 0.0 -- Wc roundings each;
 *   S = (0.0 + P_0) + P_1 + ..., pp = (0.0 + (Pr_0^2 + Pi_0^2)) + ..., i ascending (every product and sum one operation);
 *   the row's terms  w * (Yr Yr + Yi Yi),  w * pp,  w * (Sr Yr + Si Yi),  w * (Si Yr - Sr Yi),  w * (Sr Sr + Si Si);
 *   rows: with Kt = min(K, 256) and R = min(Hc, max(1, 256 / Kt)), the rows r = rl, rl + R, rl + 2R, ... are added in that
 *   order from 0.0 for each rl < R, then the R sums in ascending rl: the value of (sample, output, plane, k), kept in scratch;
 *   samples: one owner per (slot, plane, o, k) adds the call's samples of the slot to the stored value in ascending n.
 *   So an entry carries at most 2 Wc + 2 M + 3 roundings inside a row term, ceil(Hc / R) + R - 1 <= Hc additions over the
 *   rows and one per sample.  No floating-point atomics: spec is bit-identical run to run, under any split of the samples
 *   into consecutive calls, and for N beyond NINT_SPEC_MAX_N (run in pieces).
 *   scratch   nint_spec_scratch_bytes(N, M, O, Hc, Wc) = min(N, NINT_SPEC_MAX_N) * O * NINT_SPEC_PLANES * K * 8 bytes, 8-byte
 *             aligned.  Memory contract: exactly that many suffice, no store goes outside spec and scratch,
 *             and no result depends on a byte the library did not write, nor on a pixel outside the crop.
 * Before any launch -- NINT_E_ARG: a NULL pred / sample_off / y / tw / spec / scratch, M outside [1, NINT_ENS_MAX_M], N, O or
 * nslots < 1, a negative offset or stride, a slot outside [-1, nslots), a crop outside the grid, Wc < 2, a scratch that is too
 * small; NINT_E_SHAPE: Wc > NINT_SPEC_MAX_W; then NINT_E_ALIGN: spec / scratch / row_w / tw not 8-byte, pred / y not 4-byte
 * aligned.  nint_spec_twiddles: NINT_E_ARG for a NULL table or Wc < 2, NINT_E_SHAPE for Wc > NINT_SPEC_MAX_W. */
#define NINT_SPEC_PLANES 5    /* per (slot, output, wavenumber): YY, PP, CR, CI, SS */
#define NINT_SPEC_MAX_W  512  /* crop width; NINT_E_SHAPE beyond */
#define NINT_SPEC_MAX_N  64   /* samples per launch; larger N split internally, as NINT_ENS_MAX_N is */
size_t nint_spec_scratch_bytes(int N, int M, int O, int Hc, int Wc);      /* host arithmetic only */
int nint_spec_twiddles(int Wc, double* tw /*HOST [Wc][2]*/);              /* host arithmetic only */
int nint_spec_accum(const float* pred, const int64_t* sample_off /*host, N*/, int64_t member_stride, int M, const float* y,
                    const int32_t* slot /*host, N, or NULL = all 0*/, int nslots, const double* row_w /*device [Hc] or NULL = 1*/,
                    const double* tw /*device [Wc][2]*/, double* spec, double* scratch, size_t scratch_bytes, int N, int O, int H,
                    int W, int oy, int ox, int Hc, int Wc, void* stream);

/* ---- optimiser (train.py:71,110) ---------------------------------------------------------------- */
/* torch.optim.Adam (eps 1e-8, no weight decay / amsgrad) on one flat f32 buffer.
 * grad_scale multiplies g first (1/world_size after the RCCL all-reduce). step is 1-based. */
int nint_adam_flat(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1,
                   double beta2, double eps, int step, float grad_scale, void* stream);

/* Global L2 norm of the flat gradient bucket, on the caller's stream, no host read: S = sum (double)g[i]^2 in f64,
 * out[0] = S, out[1] = (double)grad_scale * sqrt(S) (the norm of the SCALED gradient).  Two launches: a fixed number of
 * workgroups (NINT_GRAD_NORM_BLOCKS, whatever the device) each reduce a grid-stride share in a fixed order, one workgroup
 * folds their partials; no atomics, so S depends on (g, n) only -- bit-identical run to run and on every rank that holds
 * the same bucket.  g needs 4-byte alignment only (dword loads).  scratch: nint_grad_norm_scratch_bytes() bytes, 8-byte
 * aligned.  n == 0: S = 0.  NINT_E_ARG: NULL g / out / scratch, a scratch that is too small; NINT_E_ALIGN: out or scratch
 * not 8-byte aligned -- both before any launch.
 * Memory contract: a scratch of exactly nint_grad_norm_scratch_bytes() is enough, here and in the guarded
 * Adam entries -- no kernel stores outside it, and no result depends on a byte outside it or on its prior contents. */
#define NINT_GRAD_NORM_BLOCKS 256
size_t nint_grad_norm_scratch_bytes(void);
int nint_grad_norm_flat(const float* g, size_t n, float grad_scale, double* out, double* scratch, size_t scratch_bytes,
                        void* stream);

/* nint_adam_flat behind a gradient-norm guard decided on the device: torch.nn.utils.clip_grad_norm_(max_norm) and,
 * optionally, dropping a step whose gradient is not finite.  Three launches: the norm partials above, a one-workgroup
 * control kernel that folds them and writes the step's scalars into `state`, and the Adam body, which reads them there.
 *   gs        = grad_scale (1/world_size after the all-reduce: every rank decides from the same bits)
 *   norm      = (double)gs * sqrt(S)
 *   coef      = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1       (clip_grad_norm_'s formula; 1 for a NaN norm)
 *   s         = (float)((double)gs * coef)       rounded once; the body's gradient is g[i] * s.  coef == 1: s == gs exactly
 *   apply     = isfinite(S) || !skip_nonfinite
 *   step      = applied + 1;  bc1 = 1 - pow(beta1, step);  bc2 = 1 - pow(beta2, step)
 *   step_size = (float)(lr / bc1);  sqrt_bc2 = (float)sqrt(bc2)            (nint_adam_flat's host expressions, in f64)
 * apply == 0: no thread stores to p, m or v and `applied` stays, so the bias correction counts applied steps only.
 * With coef == 1 the body is nint_adam_flat(step = applied + 1) bit for bit.  max_norm == 0: no clipping.
 * state: NINT_OPT_STATE doubles, 8-byte aligned; the caller zeroes it once (or sets [NINT_OPT_APPLIED] on resume):
 *   [0] applied steps   [1] skipped steps   [2] clipped steps (finite norm, coef < 1)   [3] calls
 *   [4] sum of norm over the calls with a finite S   [5] number of those calls   [6] max of norm over them
 *   this call: [7] S   [8] norm   [9] coef   [10] s   [11] step_size   [12] sqrt_bc2   [13] apply (0 / 1)   [14..15] 0
 *   ([10..12] are f32 values held in doubles; [11..12] belong to step applied + 1 whether or not it is applied.)
 * n == 0 is a call with S = 0 (it counts, and applies).  NINT_E_ARG: a NULL p / g / m / v / state / scratch, a negative or
 * NaN max_norm, a scratch smaller than nint_grad_norm_scratch_bytes(); NINT_E_ALIGN: state or scratch not 8-byte aligned --
 * both before any launch. */
#define NINT_OPT_STATE 16
enum { NINT_OPT_APPLIED = 0, NINT_OPT_SKIPPED = 1, NINT_OPT_CLIPPED = 2, NINT_OPT_CALLS = 3, NINT_OPT_SUM_NORM = 4,
       NINT_OPT_FINITE = 5, NINT_OPT_MAX_NORM = 6, NINT_OPT_S = 7, NINT_OPT_NORM = 8, NINT_OPT_COEF = 9, NINT_OPT_SCALE = 10,
       NINT_OPT_STEP_SIZE = 11, NINT_OPT_SQRT_BC2 = 12, NINT_OPT_APPLY = 13 };
int nint_adam_flat_guarded(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2,
                           double eps, float grad_scale, double max_norm, int skip_nonfinite, double* state,
                           double* scratch, size_t scratch_bytes, void* stream);

/* Fine-tuning: torch.optim.AdamW (decoupled weight decay) over GROUPS of the flat buffer, each with its own learning rate
 * and decay, in ONE launch of the Adam body.  groups: a HOST table of ngroups ranges [begin, end) of element indices, sorted
 * and non-empty, that tile ONE contiguous range [groups[0].begin, groups[ngroups-1].end) without a gap (group k+1 begins
 * where group k ends); it travels to the kernel by value.  Elements outside that range are FROZEN: p, g, m and v are
 * neither read nor written there.  Per element of group k, in torch's AdamW single-tensor order:
 *     p = p * (float)(1 - lr_k * weight_decay_k)       one f32 multiply, the multiplier formed in f64 and rounded once
 *     then the element update of nint_adam_flat as it stands, with step_size = (float)(lr_k / bc1)
 * With weight_decay_k == 0 the multiplier is 1.0f and the group's update is nint_adam_flat(p + begin, ..., end - begin, lr_k)
 * bit for bit.  NINT_E_ARG before any launch: a NULL p / g / m / v / groups, ngroups outside [1, NINT_MAX_OPT_GROUPS], an
 * empty or unsorted group, a gap or an overlap between neighbours, an lr or weight_decay that is negative or not finite,
 * step < 1.
 * nint_adam_flat_groups_guarded: nint_adam_flat_guarded's guard in front of it.  The norm partials and the control kernel run
 * over the range only -- S is nint_grad_norm_flat(g + begin_0, end_last - begin_0) bit for bit, an inf outside the range
 * is never seen -- and the control kernel writes each group's scalars into gstate (DEVICE, 2 * ngroups doubles, 8-byte
 * aligned): gstate[2k] = step_size of group k, gstate[2k+1] = its decay multiplier, f32 values held in doubles like
 * state[10..12].  state[0..13] keep their meaning; [11] is group 0's step size.  A skipped step stores nothing to p, m or
 * v anywhere.  Checks: both entries' own, and gstate NULL (NINT_E_ARG) or not 8-byte aligned (NINT_E_ALIGN). */
typedef struct nint_opt_group { uint64_t begin, end; double lr, weight_decay; } nint_opt_group;   /* host table */
#define NINT_MAX_OPT_GROUPS (2 * NINT_MAX_LAYERS + 2)
int nint_adam_flat_groups(float* p, const float* g, float* m, float* v, const nint_opt_group* groups /*host*/, int ngroups,
                          double beta1, double beta2, double eps, int step, float grad_scale, void* stream);
int nint_adam_flat_groups_guarded(float* p, const float* g, float* m, float* v, const nint_opt_group* groups /*host*/,
                                  int ngroups, double beta1, double beta2, double eps, float grad_scale, double max_norm,
                                  int skip_nonfinite, double* state, double* gstate, double* scratch, size_t scratch_bytes,
                                  void* stream);

/* ---- preproc (dataset.py:520-536, 61-98) --------------------------------------------------------- */
/* Fuse on the channel axis, z-score with mean/std (C = sum lev floats, device), cyclic-lon + lat halo pad.
 * mode 0 = the committed reference behaviour (np.fliplr on the channel axis, dataset.py:96),
 * mode 1 = true latitude reflect (dataset.py:51 semantics).
 * srcs: host array of nsrc device pointers; lev: host array of levels per source (u,v,omega at L levels,
 * prec and emission at 1).
 *
 * nint_preproc_fuse_pad      : ONE sample; srcs[i] points at the window's first time step, (T, lev_i, H, W) f32
 *                              -> out (T, C, Hp, Wp) f32   (the Dataset.__getitem__ result, dataset.py:538-539).
 * nint_preproc_fuse_pad_batch: B samples in one launch; srcs[i] is the whole RECORD (n_steps, lev_i, H, W) and
 *                              sample b reads the time steps [t0[b], t0[b]+T) (the sliding window of
 *                              dataset.py:614-616 as a pointer offset) -> out (B, T, C, Hp, Wp) f32.
 * nint_preproc_fuse_pad_slab : the same B windows written STRAIGHT into the model's input halo slab
 *                              (image t*B+b, ET = dtype, channels-last, channel padding zeroed) on the padded
 *                              grid g->H x g->W = Hp x Wp: the f32 NCHW tensor of dataset.py:538 and the
 *                              nint_pack_btchw pass never exist.  Values are the f32 result rounded once to ET.
 * t0: host array of B non-negative window starts.
 *
 * nint_preproc_fuse_pad_static[_batch|_slab]: the same three with `nstatic` after `nsrc`: the LAST nstatic of the
 *                              nsrc sources are time-invariant (the static attributes of dataset.py:100-122,
 *                              concatenated after the dynamic channels before the pad, :531-533 / :622-624).  A static
 *                              source is laid out (lev_i, H, W) f32 -- one "time step" -- and is read at that step for
 *                              every sample and window step: t0 does not apply to it (and srcs[i] of the single-sample
 *                              entry is its base, not a window offset).  It counts as one source of lev_i levels against
 *                              the 16-source limit; mean / std cover all C channels, static ones included.  Static
 *                              channels are ordinary fused channels otherwise, so in mode 0 the halo rows of channel c
 *                              come from channel C-1-c across the whole C (the met channels' halo from the static
 *                              channels and the other way round).  nstatic outside [0, nsrc]: NINT_E_ARG before any
 *                              launch.  The three entries above are these with nstatic = 0. */
#define NINT_PRE_MAX_B 64   /* samples per launch (larger batches are split internally) */
int nint_preproc_fuse_pad(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc,
                          const float* mean, const float* std, float* out, int T, int H, int W,
                          int Hp, int Wp, int mode, void* stream);
int nint_preproc_fuse_pad_batch(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc,
                                const float* mean, const float* std, const int* t0 /*host*/, int B, float* out,
                                int T, int H, int W, int Hp, int Wp, int mode, void* stream);
int nint_preproc_fuse_pad_slab(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc,
                               const float* mean, const float* std, const int* t0 /*host*/, int B, void* xs_slab,
                               int Cxp, int xfold_k /* 0: plain slab; k: horizontally folded for kernel size k */,
                               int T, int H, int W, const nint_geom* g /*host*/, int mode, int dtype, void* stream);
int nint_preproc_fuse_pad_static(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc, int nstatic,
                                 const float* mean, const float* std, float* out, int T, int H, int W,
                                 int Hp, int Wp, int mode, void* stream);
int nint_preproc_fuse_pad_static_batch(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc, int nstatic,
                                       const float* mean, const float* std, const int* t0 /*host*/, int B, float* out,
                                       int T, int H, int W, int Hp, int Wp, int mode, void* stream);
int nint_preproc_fuse_pad_static_slab(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc, int nstatic,
                                      const float* mean, const float* std, const int* t0 /*host*/, int B, void* xs_slab,
                                      int Cxp, int xfold_k, int T, int H, int W, const nint_geom* g /*host*/, int mode,
                                      int dtype, void* stream);

/* The two slab entries for CYCLIC LONGITUDE (nint_seq.lon_cyclic): a horizontally folded slab (xfold_k > 1) is folded over the
 * padded grid taken mod g->W instead of with zeros outside it -- the model's own boundary condition, so the grid must carry
 * no longitude halo (g->W == W; else NINT_E_ARG).  A plain slab (xfold_k = 0) is written as by the entries above: its halo
 * columns are nint_seq_fwd's. */
int nint_preproc_fuse_pad_slab_cyclic(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc,
                                      const float* mean, const float* std, const int* t0 /*host*/, int B, void* xs_slab,
                                      int Cxp, int xfold_k, int T, int H, int W, const nint_geom* g /*host*/, int mode, int dtype,
                                      void* stream);
int nint_preproc_fuse_pad_static_slab_cyclic(const float* const* srcs /*host*/, const int* lev /*host*/, int nsrc, int nstatic,
                                             const float* mean, const float* std, const int* t0 /*host*/, int B, void* xs_slab,
                                             int Cxp, int xfold_k, int T, int H, int W, const nint_geom* g /*host*/, int mode,
                                             int dtype, void* stream);

/* ---- recurrent state hand-off -------------------------------------------------------------- */
/* (h, c) of every layer from one state block to another, in slab form, in ONE launch.  A state block of
 * layer l is B images of the ET halo slab [Hh][Wh][Chp[l]] (h) and B images of the f32 compact slab [H][W][Chp[l]] (c):
 * slot T of nint_seq.h[l] / .c[l] after a forward pass, slot 0 of a has_init_state workspace, or a stand-alone buffer.
 * h_dst[l] / c_dst[l] / h_src[l] / c_src[l]: host arrays of L device pointers to the first image of each block.
 * Destination sample b receives source sample lane[b]; lane[b] = -1 gives it the zero state (this lane starts a new record);
 * lane = NULL is the identity and needs B_dst == B_src.  Halo-slab images are copied whole: the source's halo and slack are
 * zero by the slab invariant, so the destination's are zero afterwards; a reset image is written as zeros, halo included.
 * B_dst above NINT_PRE_MAX_B is split internally.  Before any launch: NINT_E_ARG for a NULL table or pointer, L outside
 * 1..NINT_MAX_LAYERS, a Chp[l] that is no multiple of nint_kc(dtype), a lane value outside [-1, B_src), or source and
 * destination blocks of a layer that overlap; NINT_E_ALIGN for a pointer that is not 16-byte aligned. */
int nint_state_copy(void* const* h_dst /*host*/, float* const* c_dst /*host*/, const void* const* h_src /*host*/,
                    const float* const* c_src /*host*/, const int32_t* Chp /*host, L*/, int L, int B_dst, int B_src,
                    const int32_t* lane /*host, B_dst entries, or NULL*/, const nint_geom* g /*host*/, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NINT_H */
