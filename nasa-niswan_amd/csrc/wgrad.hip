// wgrad.hip -- conv backward-weight for the ConvLSTM gate convolution on gfx950 MFMA.
//
//   dW[o][c][ky][kx] = sum_{n,y,x} dG[n,y,x,o] * cat[n, y+ky-p, x+kx-p, c]      (autograd of model.py:220)
//
// All T time steps are reduced in ONE launch per source (x / h): the BPTT loop only stores
// dG_t, so the reduction dimension is K = T*B*H*W pixels and the grid is (split-K, output block).
// GEMM view: M = 64 gate columns n' (4 MFMA row tiles), N = 16*NTC cat channels x all k*k taps,
// K = pixels.  The MFMA K index runs over pixels, but the slabs are channels-last, so both
// operands are read TRANSPOSED from their LDS images:
//   bf16: ds_read_b64_tr_b16 -- a 16-lane group turns a 4-pixel x 16-channel block into
//         "lane = channel, 4 pixels per lane"; two reads give the 8 K-slots of a 16x16x32 MFMA.
//         A (dG) and B (cat, shifted by the tap) use the SAME pixel->K-slot assignment, which is
//         all a reduction needs.
//   f32 : plain ds_read_b32 (lane = channel) feeding v_mfma_f32_16x16x4_f32.
// Taps are free: the cat image is a halo tile and a tap is a constant LDS address offset.
// The bias gradient db[o] = sum_pixels dG[.,o] rides along: the dG fragments are in registers anyway, so ONE wave of the
// workgroups that own channel block 0 of the x source multiplies them with an all-ones fragment (4 extra MFMAs per
// pixel row on the wave with the fewest columns); the result is one more column of the partial slab, folded by the
// same reduction launch.  No separate pass over dG, no per-step partial rows in the BPTT kernels.
// Each workgroup keeps its 64 x (16*NTC*taps) output block in accumulators for its whole pixel
// range and writes ONE partial slab; a second kernel folds the slabs in fixed order
// (bitwise reproducible, no float atomics) into the OIHW gradient.
#include <type_traits>
#include "nint_common.h"

// The two LDS images of a pixel tile (PR rows x 32 pixels of dG, the cat halo tile around them), shared by both kernel families:
// RA bytes per dG pixel, RB per cat halo pixel (data + padding: conflict-free strides), counted in 16-byte units INCLUDING the
// padding.  A tile is staged by LDS-DMA (global_load_lds_dwordx4: 64 consecutive units = one 1-KiB piece per wave instruction,
// per-lane source address), no VGPR round trip, no ds_write pass; lanes that land on padding re-read the tile's first unit.
// Kernel, launch record (WgRow.lds) and DESIGN.md 4.2 all read the sizes from here.
template <int KS, int PR_, int RA_, int RB_> struct WgImage {
  static constexpr int PR = PR_, RA = RA_, RB = RB_;
  static constexpr int p = KS / 2, HWt = 32 + 2 * p, HHt = PR + 2 * p;
  static constexpr int UA_ROW = RA / 16, NA_U = PR * 32 * UA_ROW;
  static constexpr int UB_PIX = RB / 16, NB_U = HHt * HWt * UB_PIX, NB_U_PAD = (NB_U + 63) / 64 * 64;
  static constexpr int a_bytes = PR * 32 * RA, b_bytes = NB_U_PAD * 16, buf_bytes = a_bytes + b_bytes;
  static constexpr int NI_A = NA_U / 64, NI_B = NB_U_PAD / 64, NI = NI_A + NI_B;      // DMA pieces of a tile
  static constexpr size_t lds = 2 * (size_t)buf_bytes;                                // two buffers: the next tile lands under this one's MFMAs
  static_assert(NA_U % 64 == 0 && a_bytes % 1024 == 0, "whole DMA pieces");
  static_assert(lds <= 160 * 1024, "two tile buffers in a CU's LDS");
};
// the 4-wave kernel's tile: 64 gate columns of dG (+ 32 / 64 bytes of padding), NTCT channel tiles of cat
template <int DT, int KS, int NTCT>
struct WgNarrow : WgImage<KS, DT == NINT_BF16 ? 4 : 2, DT == NINT_BF16 ? 160 : 320, (NTCT == 1 ? 32 : 96) * (DT == NINT_BF16 ? 1 : 2)> {
  static constexpr int block = 256;
  static constexpr int A_UNITS_PIX = 64 * Elem<DT>::ES / 16;         // 16-byte data units per dG pixel (64 gate columns)
  static constexpr int B_UNITS_PIX = 16 * NTCT * Elem<DT>::ES / 16;  // data units per cat halo pixel
  static constexpr int NI_WM = (WgNarrow::NI + 1) / 2;               // most DMA pieces one wave may take
};

// ---- device pieces both kernels are made of
// The transposed-read pair: two ds_read_b64_tr_b16, `half` bytes (16 pixels) apart, give the 8 K-slots of a 16x16x32 MFMA --
// pixels 4*g + q and 16 + 4*g + q of the 32-pixel row segment that `ad` (per-lane base + immediate) points into.
__device__ __forceinline__ u32x4_t wg_read_tr(const char* ad, int half) {
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(ad));
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(ad + half));
  u32x2_t l2 = __builtin_bit_cast(u32x2_t, lo), h2 = __builtin_bit_cast(u32x2_t, hi);
  return (u32x4_t){l2[0], l2[1], h2[0], h2[1]};
}
// One DMA piece: 64 lanes x 16 bytes from the per-lane address `src` to the 1 KiB at `dst` (wave-uniform).
// Issued as inline asm ON PURPOSE: hipcc would count the builtin as an LDS write and wait vmcnt(0) ahead of the next ds_read (it
// cannot tell the two buffers apart), which makes the staging synchronous; an asm DMA is invisible to its bookkeeping, so the
// wait is ours: s_waitcnt vmcnt(0) ahead of the tile's barrier.  M0 = LDS destination base, saved and restored in the SAME
// statement: the compiler keeps values of its own in M0 and sees none of this.
__device__ __forceinline__ void wg_dma_piece(const char* src, char* dst) {
  unsigned keep;
  const unsigned lds_dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)dst);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}
// The tile cursor (tx, ty, img): coordinates of the next tile to load, set here for a split's first tile and then kept
// incrementally (the tiles of a split are consecutive).
__device__ __forceinline__ void wg_cursor_at(int tile, int tiles_x, int tiles_y, int& tx, int& ty, int& img) {
  const int r = tile / tiles_x;
  tx = tile - r * tiles_x;
  img = r / tiles_y;
  ty = r - img * tiles_y;
}
// (Two more pieces exist in both kernels and stay written out, each with a pointer to its twin: the cursor's step and the store
// of a 16 x 16 accumulator tile into a slab column.  As functions, in every form tried, they moved instructions -- the step in
// the one instance that calls its staging lambda out of line, the store in every instance; see profiles/wgrad_refactor_asm.txt.)

// ---------------------------------------------------------------------------------------------- the 64-column kernel
// Four waves; every wave owns all 4 row tiles (64 gate columns) and JW of the workgroup's 4 * JW (tap, channel-tile) columns
// (25 taps: 7 + 7 + 7 + 4); a source with more columns (the 49 taps of a 7x7 kernel) takes TG column groups on extra workgroups.
// KS (kernel size) and NTCT (channel tiles per column block) are template parameters so that every LDS
// fragment address is `per-lane base VGPR + compile-time immediate`: the transposed reads then cost no
// VALU instruction at all (the MFMAs leave only ~8 issue cycles each to the rest of the wave).
// KX = horizontal taps of the source: KS, or 1 for a horizontally folded x source (nint_layer.xfold: its columns are
// (vertical tap, folded channel tile) and every tap reads the centre column of the halo tile).
template <int DT, int JW, int KS, int NTCT, int KX>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgradArgs a) {
  typedef Elem<DT> E;
  typedef WgNarrow<DT, KS, NTCT> G;
  constexpr int PR = G::PR, RA = G::RA, RB = G::RB, HWt = G::HWt, HHt = G::HHt, p = G::p, k = KS;
  constexpr int UA_ROW = G::UA_ROW, UB_PIX = G::UB_PIX, a_bytes = G::a_bytes, buf_bytes = G::buf_bytes;
  constexpr int NI_A = G::NI_A, NI = G::NI, NI_WM = G::NI_WM;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // (integer division runs on the vector ALU: readfirstlane puts the workgroup-uniform results back into scalars)
  int by = blockIdx.y, part = 0;
  if (a.nparts == 2) {                        // per gate block: the x source's channel blocks, then the h source's (TG == 1)
    const int per_nb = a.s[0].CB + a.s[1].CB;
    const int nbq = by / per_nb, r = by - nbq * per_nb;
    part = r >= a.s[0].CB ? 1 : 0;
    by = part ? nbq * a.s[1].CB + (r - a.s[0].CB) : nbq * a.s[0].CB + r;
  }
  part = __builtin_amdgcn_readfirstlane(part);
  by = __builtin_amdgcn_readfirstlane(by);
  // (this source's fields, read once into scalars: the tile loop must not index the argument table)
  struct { const char* dG; const char* src; long src_img_stride; int src_pix_stride; float* partial; int CB, JG, nblk, ntiles, tiles_per_split, want_db; } S;
  {
    const WgSrc& T = a.s[part];
    S.dG = T.dG; S.src = T.src; S.src_img_stride = T.src_img_stride; S.src_pix_stride = T.src_pix_stride; S.partial = T.partial;
    S.CB = T.CB; S.JG = T.JG; S.nblk = T.nblk; S.ntiles = T.ntiles; S.tiles_per_split = T.tiles_per_split; S.want_db = T.want_db;
  }
  const int tg = __builtin_amdgcn_readfirstlane(by % a.TG);   // column group
  const int bc = __builtin_amdgcn_readfirstlane(by / a.TG);   // (gate block, channel block)
  const int nb = bc / S.CB, cb = bc % S.CB;
  const int jb = tg * 4 * JW;                 // first column of this workgroup
  const int t_begin = blockIdx.x * S.tiles_per_split;
  const int t_end = min(S.ntiles, t_begin + S.tiles_per_split);
  const int j0 = wave * JW;                   // first column of this wave

  f32x4_t acc[4][JW];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < JW; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // bias gradient: channel block 0 / LAST column group of the source that carries it, on the last wave -- which has
  // fewer than JW real columns there (wg_narrow_row's static_assert), so its accumulator column JW-1 is free: no extra registers
  int db_here = 0;                            // (an if, not a && chain inside ?: -- that spelling schedules every instance differently)
  if (S.want_db && cb == 0 && tg == a.TG - 1 && wave == 3) db_here = 1;
  const bool do_db = __builtin_amdgcn_readfirstlane(db_here);

  // DMA pieces of a tile are dealt to the waves in CONTIGUOUS ranges sized to even out each wave's work per tile:
  // a wave with fewer real columns (25 taps over 4 waves = 7, 7, 7, 4) has idle issue slots that the staging of the
  // next tile can use, so it takes more pieces: n_w = (L - nv_w * CM) / CD with the common level L such that the n_w
  // sum to NI (CM = matrix-pipe cycles per column and tile, CD ~ issue cost of one piece).  Wave-uniform integer math.
  int p_begin, p_cnt;
  {
    constexpr int CM = (DT == NINT_BF16 ? 16 : 32 * 4) * 4 * PR, CD = 100;
    int nv[4], n16[4], tot = 0, sum_nv = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { nv[w] = min(JW, max(0, a.J - jb - w * JW)); sum_nv += nv[w]; }
    const int L = (NI * CD + CM * sum_nv) / 4;
#pragma unroll
    for (int w = 0; w < 4; ++w) { n16[w] = max(0, (L - nv[w] * CM) * 16 / CD); tot += n16[w]; }
    // scale to NI pieces (rounded prefix sums), cap every wave at NI_WM and hand the excess on (4 * NI_WM >= 2 * NI)
    int cnt[4], prev = 0, acc16 = 0, excess = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      acc16 += n16[w];
      const int e = w == 3 ? NI : (tot > 0 ? min(NI, (acc16 * NI + tot / 2) / tot) : (w + 1) * NI / 4);
      cnt[w] = e - prev;
      prev = e;
      if (cnt[w] > NI_WM) { excess += cnt[w] - NI_WM; cnt[w] = NI_WM; }
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int take = min(NI_WM - cnt[w], excess);
      cnt[w] += take;
      excess -= take;
    }
    const int s1 = cnt[0], s2 = s1 + cnt[1], s3 = s2 + cnt[2];
    // (the divisions above run on the vector ALU: back into scalars, the LDS destination of a DMA piece is an SGPR)
    p_begin = __builtin_amdgcn_readfirstlane(wave == 0 ? 0 : (wave == 1 ? s1 : (wave == 2 ? s2 : s3)));
    p_cnt = __builtin_amdgcn_readfirstlane(wave == 0 ? cnt[0] : (wave == 1 ? cnt[1] : (wave == 2 ? cnt[2] : cnt[3])));
  }
  // Per-lane source offsets of this wave's DMA pieces (piece t = p_begin + i), relative to the wave-uniform tile
  // base: they do not depend on the tile, so the tile loop spends no VALU on staging addresses.
  unsigned doff[NI_WM];
#pragma unroll
  for (int i = 0; i < NI_WM; ++i) {
    const int t = p_begin + i;
    unsigned o = 0;
    if (t < NI_A) {
      const int u = t * 64 + lane;
      const int pix = u / UA_ROW, q = u - pix * UA_ROW;
      if (q < G::A_UNITS_PIX) o = (unsigned)(((pix >> 5) * a.Wh + (pix & 31)) * a.dG_pix_stride + q * 16);
    } else if (t < NI) {
      const int u = (t - NI_A) * 64 + lane;
      const int hp = u / UB_PIX, q = u - hp * UB_PIX;
      const int hy = hp / HWt, hx = hp - hy * HWt;
      if (hp < HHt * HWt && q < G::B_UNITS_PIX) o = (unsigned)((hy * a.Wh + hx) * S.src_pix_stride + q * 16);
    }
    doff[i] = o;
  }
  int ld_tx, ld_ty, ld_img;
  wg_cursor_at(t_begin, a.tiles_x, a.tiles_y, ld_tx, ld_ty, ld_img);
  const char* const ga0 = S.dG + nb * 64 * E::ES;
  const char* const gb0 = S.src + cb * 16 * NTCT * E::ES;

  auto issue_dma = [&](char* buf) {          // stages tile (ld_img, ld_ty, ld_tx) into buf, then steps to the next tile
    const int y0 = ld_ty * PR, x0 = ld_tx * 32;
    const char* ga = ga0 + (long)ld_img * a.dG_img_stride + ((long)(y0 + a.P) * a.Wh + (x0 + a.P)) * a.dG_pix_stride;
    const char* gb = gb0 + (long)ld_img * S.src_img_stride + ((long)(y0 + a.P - p) * a.Wh + (x0 + a.P - p)) * S.src_pix_stride;
#pragma unroll
    for (int i = 0; i < NI_WM; ++i) {
      const int t = p_begin + i;               // wave-uniform
      if (i < p_cnt) {
        wg_dma_piece((t < NI_A ? ga : gb) + doff[i], buf + (t < NI_A ? t * 1024 : a_bytes + (t - NI_A) * 1024));
      }
    }
    const bool wx = ld_tx + 1 == a.tiles_x;      // (the cursor's step; twin: wgrad_wide_kernel's issue_dma)
    const bool wy = wx && (ld_ty + 1 == a.tiles_y);
    ld_tx = wx ? 0 : ld_tx + 1;
    ld_ty = wy ? 0 : (wx ? ld_ty + 1 : ld_ty);
    ld_img += wy ? 1 : 0;
  };

  if (t_begin < t_end) issue_dma(smem);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // lane constants of the transposed reads
  const int g = lane >> 4, i16 = lane & 15;
  // Per-lane base offsets (VGPRs, computed once).  Column jj of this wave is (tap, channel tile)
  // j0+jj; columns past J are clamped duplicates whose accumulators are never flushed, which keeps
  // the K loop branch-free.
  int vB[JW];
  int vA;
  const int nvalid = __builtin_amdgcn_readfirstlane(min(JW, max(0, a.J - jb - j0)));   // real columns of this wave
  constexpr int JT = KS * KX * NTCT;                                              // = a.J (the row's column count)
  constexpr int XO = KX == KS ? 0 : p;                                            // folded: the centre column
  constexpr int NVL = JT % JW == 0 ? JW : JT % JW;                                // columns of the last, partial group
  if constexpr (DT == NINT_BF16) {
    const int q = i16 >> 2, p8 = (i16 & 3) * 8;
    vA = (4 * g + q) * RA + p8;                      // pixel 4g+q of a 16-pixel half segment, 8 bytes of 4 channels
#pragma unroll
    for (int jj = 0; jj < JW; ++jj) {
      const int j = min(jb + j0 + jj, a.J - 1);
      const int tap = j / NTCT, ct = j - tap * NTCT;
      const int tyy = tap / KX, txx = tap - tyy * KX + XO;
      vB[jj] = a_bytes + (tyy * HWt + txx + 4 * g + q) * RB + ct * 32 + p8;
    }
  } else {
    vA = g * RA + i16 * 4;                // MFMA m of a 16-pixel K-step takes pixel 4m+g
#pragma unroll
    for (int jj = 0; jj < JW; ++jj) {
      const int j = min(jb + j0 + jj, a.J - 1);
      const int tap = j / NTCT, ct = j - tap * NTCT;
      const int tyy = tap / KX, txx = tap - tyy * KX + XO;
      vB[jj] = a_bytes + (tyy * HWt + txx + g) * RB + (ct * 16 + i16) * 4;
    }
  }
  // The tile loop exists once per column count a wave can have (JW, the NVL columns left for the last group, or none):
  // inside it the column count is a compile-time constant, so a tile is ONE basic block -- the compiler is free to
  // hoist the transposed reads of pixel row pr+1 above the MFMAs of row pr -- and no MFMA is predicated.  Every variant
  // issues the same DMA pieces and the same barriers.
  auto run_tiles = [&](auto nvc, auto dbc) __attribute__((always_inline)) {
    constexpr int NV = decltype(nvc)::value;
    constexpr bool DB = decltype(dbc)::value;
    for (int tile = t_begin; tile < t_end; ++tile) {
      const int cur = (tile - t_begin) & 1;
      const bool more = tile + 1 < t_end;
      if (more) issue_dma(smem + (cur ^ 1) * buf_bytes);   // the other buffer was last read before the previous barrier
      const char* Ab = smem + cur * buf_bytes + vA;      // one add per base and tile; everything below is base + immediate
      const char* Bb[JW];
#pragma unroll
      for (int jj = 0; jj < JW; ++jj) Bb[jj] = smem + cur * buf_bytes + vB[jj];
      if constexpr ((NV > 0 || DB) && DT == NINT_BF16) {
#pragma unroll
        for (int pr = 0; pr < PR; ++pr) {
          u32x4_t af[4], bf[NV > 0 ? NV : 1];
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = wg_read_tr(Ab + pr * 32 * RA + i * 32, 16 * RA);
#pragma unroll
          for (int jj = 0; jj < NV; ++jj) bf[jj] = wg_read_tr(Bb[jj] + pr * HWt * RB, 16 * RB);
#pragma unroll
          for (int jj = 0; jj < NV; ++jj)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][jj] = mma_step<NINT_BF16>(af[i], bf[jj], acc[i][jj]);
          if constexpr (DB) {                  // D[gate column][.] += sum over the 32 pixels of this row segment
            const u32x4_t ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][JW - 1] = mma_step<NINT_BF16>(af[i], ones, acc[i][JW - 1]);
          }
        }
      } else if constexpr (NV > 0 || DB) {
#pragma unroll
        for (int pr = 0; pr < PR; ++pr) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            // 16 pixels per K-step: MFMA m takes pixel 4*m + g of the segment as its K index g
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              float af[4];
#pragma unroll
              for (int i = 0; i < 4; ++i)
                af[i] = *(const float*)(Ab + (pr * 32 + ks * 16 + 4 * m) * RA + i * 64);
#pragma unroll
              for (int jj = 0; jj < NV; ++jj) {
                const float bf = *(const float*)(Bb[jj] + (pr * HWt + ks * 16 + 4 * m) * RB);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                  acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf, acc[i][jj], 0, 0, 0);
              }
              if constexpr (DB) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][JW - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], 1.0f, acc[i][JW - 1], 0, 0, 0);
              }
            }
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next tile has landed ...
      __syncthreads();                           // ... for every wave, and this one is fully read
    }
  };
  if (do_db) {                                            // (wave 3 of the last group: NVL < JW columns, or none)
    if (NVL < JW && nvalid == NVL) run_tiles(std::integral_constant<int, NVL < JW ? NVL : 0>{}, std::true_type{});
    else run_tiles(std::integral_constant<int, 0>{}, std::true_type{});
  } else {
    if (nvalid == JW) run_tiles(std::integral_constant<int, JW>{}, std::false_type{});
    else if (nvalid == NVL) run_tiles(std::integral_constant<int, NVL>{}, std::false_type{});
    else run_tiles(std::integral_constant<int, 0>{}, std::false_type{});      // a wave without real columns only stages and synchronises
  }

  // ---- flush: partial[split][blockIdx.y][j local][n'loc 64][c 16]
  float* out = S.partial + ((size_t)blockIdx.x * S.nblk + by) * S.JG * 1024;
#pragma unroll
  for (int jj = 0; jj < JW; ++jj) {
    const int j = j0 + jj;
    if (jb + j < a.J) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          out[(size_t)j * 1024 + (i * 16 + 4 * g + r) * 16 + i16] = acc[i][jj][r];      // (twin: wgrad_wide_kernel's flush)
    }
  }
  if (do_db) {                                            // slab column JG-1: all 16 "channel" columns hold the same sum
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(size_t)(S.JG - 1) * 1024 + (i * 16 + 4 * g + r) * 16 + i16] = acc[i][JW - 1][r];
  }
}

// ---------------------------------------------------------------------------------------------- the 128-column kernel
// Wide layers (round 4).  The 4-wave kernel above stages a 64-column dG tile and a 16/32-channel cat tile per 64 x (16*NTC*taps)
// output block: 62 (5x5) to 137 (3x3) staged bytes per MFMA, and with every CU streaming two such workgroups the L2 -> LDS
// staging rate itself (~25 GB/s per CU by LDS-DMA) is what the matrix pipe waits for; its waves also re-read the dG fragments
// four times.  This kernel gives an 8-wave workgroup (one per CU, two waves per SIMD) a 128-gate-column x NCT-channel-tile
// output block: wave (gh, ct, half) owns the 64 gate columns gh of channel tile ct for a contiguous range of taps -- 4 row tiles
// x 9 columns (3x3: 4 channel tiles), 4 x 13 (5x5: 2 channel tiles, taps 13 + 12), 4 x 13 (7x7: 1 channel tile) -- so a dG tile
// serves NCT channel tiles and a cat tile both gate halves: 35 (5x5) / 59 (3x3) staged bytes per MFMA and 0.65 / 0.72 instead
// of 0.79 / 0.9 transposed reads per MFMA.  Tap ranges are compile-time per wave role (switch on `half`), so every fragment
// address is `per-lane base + immediate`, as above.  Partials leave in the layout of the 4-wave kernel with NTC = 1, so the
// fold kernel and the workspace arithmetic are shared.  bf16 storage only (f32 mode is not the throughput mode).
template <int KS, int NCT>
struct WgWide : WgImage<KS, 4, 288, NCT == 4 ? 160 : (NCT == 2 ? 96 : 32)> {   // dG pixel: 256 + 32 bytes; cat: conflict-free strides
  static constexpr int block = 512;
  static constexpr int taps = KS * KS;
  static constexpr int HG = KS == 3 ? 1 : (KS == 5 ? 2 : 4);         // column groups per channel tile
  static constexpr int JW = (taps + HG - 1) / HG;                   // taps per wave: 9, 13, 13
  static constexpr int NVL = taps - (HG - 1) * JW;                  // taps of the last group: 9, 12, 10
  static constexpr int JWA = JW + (NVL == JW ? 1 : 0);              // accumulator columns (the last group keeps one free for db)
  static constexpr int NW = 2 * NCT * HG;                           // waves
  static constexpr int NI_W = (WgWide::NI + NW - 1) / NW;           // DMA pieces per wave and tile
  static_assert(NW == 8, "eight waves: two per SIMD");
};

template <int KS, int NCT>
__global__ __launch_bounds__(512, 2) void wgrad_wide_kernel(WgradArgs a) {
  typedef WgWide<KS, NCT> G;
  constexpr int PR = G::PR, RA = G::RA, RB = G::RB, HWt = G::HWt, HHt = G::HHt, p = G::p, JW = G::JW, JWA = G::JWA, HG = G::HG;
  constexpr int a_bytes = G::a_bytes, buf_bytes = G::buf_bytes, NI_A = G::NI_A, NI = G::NI, NI_W = G::NI_W;
#ifndef NINT_WG_STREAM
#define NINT_WG_STREAM (JW > 9)
#endif
  constexpr bool STREAM = NINT_WG_STREAM;     // 4 x 13 tiles: explicit two-deep fragment stream; 4 x 9: the compiler's schedule
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gh = wave & 1, cgi = wave >> 1, ct = cgi / HG, half = cgi % HG;
  const WgSrc& T = a.s[0];
  const int CBW = T.CB / NCT;                               // channel groups of NCT tiles (T.CB counts 16-channel tiles)
  const int by = blockIdx.y;
  const int nbw = __builtin_amdgcn_readfirstlane(by / CBW), cbw = __builtin_amdgcn_readfirstlane(by % CBW);
  const int t_begin = blockIdx.x * T.tiles_per_split;
  const int t_end = min(T.ntiles, t_begin + T.tiles_per_split);
  const unsigned src_pix_stride = (unsigned)T.src_pix_stride;

  f32x4_t acc[4][JWA];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < JWA; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // bias gradient: channel tile 0 of the source that carries it, on the waves of the last tap group (free accumulator column)
  const bool do_db = __builtin_amdgcn_readfirstlane((T.want_db && cbw == 0 && ct == 0 && half == HG - 1) ? 1 : 0);

  // DMA pieces of a tile: piece t = wave + NW * i (dealt round-robin: every wave has the same matrix work here).  The per-lane
  // source offset of a piece is recomputed when it is issued (a dozen VALU instructions between MFMAs): the 4 x 13 accumulator
  // tile leaves no registers to keep NI_W of them.
  auto piece_off = [&](int t) __attribute__((always_inline)) {
    unsigned o = 0;
    if (t < NI_A) {
      const unsigned u = (unsigned)(t * 64 + lane);
      const unsigned pix = __umulhi(u, (unsigned)(((1ull << 32) + G::UA_ROW - 1) / G::UA_ROW)), q = u - pix * G::UA_ROW;
      o = q < 16 ? ((pix >> 5) * a.Wh + (pix & 31)) * a.dG_pix_stride + q * 16 : 0u;
    } else {
      const unsigned u = (unsigned)((t - NI_A) * 64 + lane);
      const unsigned hp = __umulhi(u, (unsigned)(((1ull << 32) + G::UB_PIX - 1) / G::UB_PIX)), q = u - hp * G::UB_PIX;
      const unsigned hy = __umulhi(hp, (unsigned)(((1ull << 32) + HWt - 1) / HWt)), hx = hp - hy * HWt;
      o = (hp < (unsigned)(HHt * HWt) && q < 2u * NCT) ? (hy * a.Wh + hx) * src_pix_stride + q * 16 : 0u;
    }
    return o;
  };
  int ld_tx, ld_ty, ld_img;
  wg_cursor_at(t_begin, a.tiles_x, a.tiles_y, ld_tx, ld_ty, ld_img);
  const char* const ga0 = T.dG + nbw * 128 * 2;
  const char* const gb0 = T.src + cbw * 16 * NCT * 2;
  const long src_img_stride = T.src_img_stride;
  auto issue_dma = [&](char* buf) {
    const int y0 = ld_ty * PR, x0 = ld_tx * 32;
    const char* ga = ga0 + (long)ld_img * a.dG_img_stride + ((long)(y0 + a.P) * a.Wh + (x0 + a.P)) * a.dG_pix_stride;
    const char* gb = gb0 + (long)ld_img * src_img_stride + ((long)(y0 + a.P - p) * a.Wh + (x0 + a.P - p)) * src_pix_stride;
#pragma unroll
    for (int i = 0; i < NI_W; ++i) {
      const int t = wave + G::NW * i;              // wave-uniform
      if (t < NI) {
        wg_dma_piece((t < NI_A ? ga : gb) + piece_off(t), buf + (t < NI_A ? t * 1024 : a_bytes + (t - NI_A) * 1024));
      }
    }
    const bool wx = ld_tx + 1 == a.tiles_x;      // (the cursor's step; twin: wgrad_kernel's issue_dma)
    const bool wy = wx && (ld_ty + 1 == a.tiles_y);
    ld_tx = wx ? 0 : ld_tx + 1;
    ld_ty = wy ? 0 : (wx ? ld_ty + 1 : ld_ty);
    ld_img += wy ? 1 : 0;
  };
  if (t_begin < t_end) issue_dma(smem);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p8 = (i16 & 3) * 8;
  const int vA = (4 * g + q4) * RA + gh * 128 + p8;                   // row tile i: + i * 32
  const int vB = a_bytes + (4 * g + q4) * RB + ct * 32 + p8;          // tap (ty, tx): + (ty * HWt + tx) * RB

  auto run_tiles = [&](auto tap0c, auto nvc, auto dbc) __attribute__((always_inline)) {
    constexpr int TAP0 = decltype(tap0c)::value, NV = decltype(nvc)::value;
    constexpr bool DB = decltype(dbc)::value;
    for (int tile = t_begin; tile < t_end; ++tile) {
      const int cur = (tile - t_begin) & 1;
      if (tile + 1 < t_end) issue_dma(smem + (cur ^ 1) * buf_bytes);   // the other buffer was last read before the previous barrier
      const char* Ab = smem + cur * buf_bytes + vA;
      const char* Bb = smem + cur * buf_bytes + vB;
#pragma unroll
      for (int pr = 0; pr < PR; ++pr) {
        u32x4_t af[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = wg_read_tr(Ab + pr * 32 * RA + i * 32, 16 * RA);
        auto colptr = [&](int jj) __attribute__((always_inline)) {
          const int tap = TAP0 + jj, tyy = tap / KS, txx = tap - tyy * KS;
          return Bb + (tyy * HWt + txx) * RB + pr * HWt * RB;
        };
        if constexpr (STREAM) {
          // cat fragments STREAMED: two live at a time, the next column's reads issued ahead of this column's MFMAs (the
          // compiler's own schedule hoists a whole row of them: 52 registers the 4 x 13 tile does not have)
          u32x4_t bfq[2];
          if constexpr (NV > 0) bfq[0] = wg_read_tr(colptr(0), 16 * RB);
#pragma unroll
          for (int jj = 0; jj < NV; ++jj) {
            if (jj + 1 < NV) bfq[(jj + 1) & 1] = wg_read_tr(colptr(jj + 1), 16 * RB);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][jj] = mma_step<NINT_BF16>(af[i], bfq[jj & 1], acc[i][jj]);
          }
        } else {
#pragma unroll
          for (int jj = 0; jj < NV; ++jj) {
            const u32x4_t bf = wg_read_tr(colptr(jj), 16 * RB);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][jj] = mma_step<NINT_BF16>(af[i], bf, acc[i][jj]);
          }
        }
        if constexpr (DB) {
          const u32x4_t ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][JWA - 1] = mma_step<NINT_BF16>(af[i], ones, acc[i][JWA - 1]);
        }
        if constexpr (STREAM) {
          __builtin_amdgcn_sched_group_barrier(0x100, NV > 0 ? 10 : 8, 0);
#pragma unroll
          for (int jj = 0; jj < NV; ++jj) {
            if (jj + 1 < NV) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
          }
          if constexpr (DB) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next tile has landed ...
      __syncthreads();                                   // ... for every wave, and this one is fully read
    }
  };
  // wave roles: the tap range is a compile-time constant inside each instance of the tile loop
  auto role = [&](auto hc) __attribute__((always_inline)) {
    constexpr int H_ = decltype(hc)::value;
    constexpr int TAP0 = H_ * JW, NV = H_ == HG - 1 ? G::NVL : JW;
    if (H_ == HG - 1 && do_db) run_tiles(std::integral_constant<int, TAP0>{}, std::integral_constant<int, NV>{}, std::true_type{});
    else run_tiles(std::integral_constant<int, TAP0>{}, std::integral_constant<int, NV>{}, std::false_type{});
  };
  if constexpr (HG == 1) role(std::integral_constant<int, 0>{});
  else if constexpr (HG == 2) { if (half == 0) role(std::integral_constant<int, 0>{}); else role(std::integral_constant<int, 1>{}); }
  else { if (half == 0) role(std::integral_constant<int, 0>{}); else if (half == 1) role(std::integral_constant<int, 1>{});
         else if (half == 2) role(std::integral_constant<int, 2>{}); else role(std::integral_constant<int, 3>{}); }

  // ---- flush in the 4-wave kernel's slab layout with NTC = 1: partial[split][(nb, cb)][tap][n'loc 64][c 16]
  const int nb = 2 * nbw + gh, cb = cbw * NCT + ct;
  float* out = T.partial + ((size_t)blockIdx.x * T.nblk + (size_t)nb * T.CB + cb) * T.JG * 1024;
  const int tap0 = half * JW, nv = half == HG - 1 ? G::NVL : JW;
#pragma unroll
  for (int jj = 0; jj < JW; ++jj) {
    if (jj < nv) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(tap0 + jj) * 1024 + (i * 16 + 4 * g + r) * 16 + i16] = acc[i][jj][r];   // (twin: wgrad_kernel's flush)
    }
  }
  if (do_db) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(T.JG - 1) * 1024 + (i * 16 + 4 * g + r) * 16 + i16] = acc[i][JWA - 1][r];
  }
}

// Fold the split-K slabs of ONE source (x or h part) into dW (OIHW f32).  A workgroup owns 64 consecutive
// elements of the slab layout [block][j][n'loc 64][c 16] (one 256-byte line per split, fully coalesced) and
// spreads the splits over its blockDim/64 waves; the per-wave sums are folded through LDS.  The order is a
// fixed function of the launch shape (bitwise reproducible); only the single write per weight is scattered.
// t.acc (nint_seq.accumulate): that write is dW = dW + sum instead of dW = sum -- the same thread, the same sum.
__global__ void wgrad_reduce_kernel(ReduceTable t) {
  __shared__ f32x4_t red[1024];
  int ei = 0;
  for (int q = 1; q < t.n; ++q) ei = blockIdx.x >= t.e[q].blk_begin ? q : ei;     // entries are in launch order
  const ReduceEntry& E = t.e[ei];
  const int Cx = E.Cx, Ch = E.Ch, k = E.k, CB = E.CB, NTC = E.NTC, J = E.J, splits = E.splits, is_h = E.is_h;
  const int TG = E.TG, JG = E.JG;
  const float* __restrict__ part = E.part;
  float* __restrict__ dW = E.dW;
  const int taps = k * k, Ctot = Cx + Ch;
  const size_t slab = (size_t)E.NB * CB * TG * JG * 1024;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6, G = E.waves;   // waves >= G idle through the barrier
  // a workgroup owns 256 consecutive slab elements, 4 per lane (16-byte loads: 1 KiB per wave and split)
  const size_t i = ((size_t)(blockIdx.x - E.blk_begin) * 64 + lane) * 4;  // slab is a multiple of 1024: no tail
  f32x4_t s = {0.f, 0.f, 0.f, 0.f};
  if (grp < G) {
#pragma unroll 8
    // NON-TEMPORAL: the slabs are read exactly once (in the step: 76 -> 66 us at B = 8, 76 -> 56 us at B = 1, where the fold is 5 % of
    // the step; the same hint on the weight-gradient kernels' slab STORES costs them more than it saves here: profiles/r04_h_fold_nt.txt)
    for (int sp = grp; sp < splits; sp += G) s += __builtin_nontemporal_load((const f32x4_t*)(part + i + (size_t)sp * slab));
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (grp != 0) return;
  for (int q = 1; q < G; ++q) s += red[q * 64 + lane];
  const int c16 = i & 15, nloc = (i >> 4) & 63;       // c16 is a multiple of 4: the lane's elements are channels c16 .. c16+3
  size_t r = i >> 10;
  const int jl = r % JG; r /= JG;
  const int tgi = r % TG; r /= TG;
  const int cb = r % CB;
  const int nb = r / CB;
  const int np = nb * 64 + nloc;                      // gate column n' = (cblock*4+gate)*16+col
  const int ch = (np >> 6) * 16 + (np & 15), gate = (np >> 4) & 3;
  const int JR = JG - (E.db ? 1 : 0);                 // real columns per group
  if (jl >= JR) {                                     // the bias-gradient column (all 16 "channels" hold the same sum)
    if (cb == 0 && tgi == TG - 1 && c16 == 0 && ch < Ch) E.db[gate * Ch + ch] = t.acc ? E.db[gate * Ch + ch] + s[0] : s[0];
    return;
  }
  const int j = tgi * JR + jl;
  if (j >= J || ch >= Ch) return;                     // unused slots of the last column group / padding rows
  const int tap0 = j / NTC;
  const int ct = j - tap0 * NTC;
  const int Csrc = is_h ? Ch : Cx;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int cc = (cb * NTC + ct) * 16 + c16 + e;          // channel inside this source
    int tap = tap0;
    if (!is_h && E.xfold) {                           // folded x source: column (ky, kx*Cx + c) -> W[.][c][ky][kx]
      if (cc >= k * Cx) continue;
      tap = tap0 * k + cc / Cx;
      cc = cc % Cx;
    }
    if (cc >= Csrc) continue;                         // padding columns
    const int ic = is_h ? Cx + cc : cc;
    float* dst = dW + (((size_t)(gate * Ch + ch)) * Ctot + ic) * taps + tap;
    *dst = t.acc ? *dst + s[e] : s[e];                  // (nint_seq.accumulate: one f32 add by the element's only writer)
  }
}

// ------------------------------------------------------------------------------ host side
// THE INSTANCE TABLE: every kernel instance that exists, once.  wg_plan derives a key from its rules and looks it up here -- a
// key without a row is NINT_E_SHAPE at plan time (so nint_wgrad_workspace_bytes is 0 and SeqEngine.untrainable_layers names the
// layer) -- and a launch record is filled from the row; nothing else names an instance.
//   4-wave rows (KS, NTCT, JW, KX), each in both storage types: plain sources; the horizontally folded x source of thin
//   first-layer inputs (KX = 1: vertical taps only); 7x7 (49 taps in two column groups).  The last line's rows -- one channel
//   tile per block, five columns per wave -- want a channel count of 16 mod 32: f32 slabs (padded to 16) reach them, bf16 slabs
//   as SeqEngine pads them (nint_kc = 32) never do (tests/test_wgrad_plan_cpu.py sweeps that through nint_debug_wgrad_plan), so
//   their bf16 halves serve raw nint_layer callers only.
#define WG_NARROW_ROWS(X) \
  X(5, 1, 7, 5) X(3, 2, 5, 3) X(1, 2, 5, 1) \
  X(5, 2, 5, 1) X(3, 2, 5, 1) X(7, 2, 5, 1) \
  X(7, 1, 7, 7) \
  X(3, 1, 5, 3) X(1, 1, 5, 1) X(5, 1, 5, 1) X(3, 1, 5, 1) X(7, 1, 5, 1)
//   8-wave rows (KS, NCT), bf16 storage only (f32 mode is not the throughput mode):
#define WG_WIDE_ROWS(X) X(3, 4) X(5, 2) X(7, 1)

struct WgRow {
  int KS, NTC, JW, KX;       // the key; JW = 0: an 8-wave row (NTC = its channel tiles per workgroup, KX = KS)
  int block;
  const void* kern[2];       // host handles by storage type (NINT_F32, NINT_BF16); nullptr: not instantiated
  size_t lds[2];             // dynamic LDS bytes: the geometry struct's two tile buffers
};
constexpr int wg_jw(int J) { return J <= 20 ? 5 : 7; }                    // columns per wave of the 4-wave kernel
template <int KS, int NTCT, int JW, int KX> static WgRow wg_narrow_row() {
  constexpr int J = KS * KX * NTCT, TG = (J + 4 * JW - 1) / (4 * JW);     // columns; column groups of 4 * JW
  static_assert(JW == wg_jw(J), "a row wg_plan's rules can derive");
  static_assert(TG == 1 || J % JW == 0, "column groups hold whole waves of columns (the tile loop exists for JW, J % JW and 0 columns per wave)");
  static_assert(J - (TG - 1) * 4 * JW <= 3 * JW + (JW - 1), "the db column needs wave 3's last accumulator column free");
  typedef WgNarrow<NINT_F32, KS, NTCT> F;
  typedef WgNarrow<NINT_BF16, KS, NTCT> B;
  return WgRow{KS, NTCT, JW, KX, F::block, {(const void*)wgrad_kernel<NINT_F32, JW, KS, NTCT, KX>, (const void*)wgrad_kernel<NINT_BF16, JW, KS, NTCT, KX>},
               {F::lds, B::lds}};
}
template <int KS, int NCT> static WgRow wg_wide_row() {
  typedef WgWide<KS, NCT> G;
  return WgRow{KS, NCT, 0, KS, G::block, {nullptr, (const void*)wgrad_wide_kernel<KS, NCT>}, {0, G::lds}};
}
static const WgRow wg_rows[] = {
#define X(KS, NTCT, JW, KX) wg_narrow_row<KS, NTCT, JW, KX>(),
  WG_NARROW_ROWS(X)
#undef X
#define X(KS, NCT) wg_wide_row<KS, NCT>(),
  WG_WIDE_ROWS(X)
#undef X
};
static const WgRow* wg_find_row(int dtype, int KS, int NTC, int JW, int KX) {      // NTC = 0: any (an 8-wave row by its KS)
  for (const WgRow& r : wg_rows)
    if (r.KS == KS && (!NTC || r.NTC == NTC) && r.JW == JW && r.KX == KX && r.kern[dtype == NINT_BF16]) return &r;
  return nullptr;
}

struct WgPart {            // one source (x or h) of the reduction
  const WgRow* row;        // its kernel instance
  int NTC, J, KX, CB, TG, JG, splits;     // slab layout: channel tiles per block, columns, horizontal taps, ...
  int nblk;                // blocks of a slab: NB * CB * TG, of JG KiB-columns each
  int cols;                // workgroup columns (grid y) of a launch of its own
  size_t slab() const { return (size_t)nblk * JG * 1024; }     // floats per split
};
struct WgPlan {
  WgPart part[2];
  int NB, tiles_x, tiles_y, ntiles;
  size_t off_h, total_floats;
  bool merged;            // both sources in ONE launch (narrow layers: the launches are bound by re-reading dG, and the x and h
                          // workgroups of a pixel range then share its tiles in L2)
};

// The 128-column kernel holds a SOURCE (x or h) of a layer when it is an unfolded bf16 slab, the gate columns come in pairs of
// 64-column blocks and the source's channels in whole channel groups (3x3: 64 channels, 5x5: 32, 7x7: 16) -- the reference
// stack's second layer (64 -> 32, 3x3) takes it for its x source only.  nint_layer.wide: 1 = never, 2 / 0 = wherever held.
static const WgRow* wg_wide_row_of(const nint_layer* ly, int dtype, int q) {
  if (ly->wide == 1 || (q == 0 && ly->xfold)) return nullptr;
  const WgRow* r = wg_find_row(dtype, ly->k, 0, 0, ly->k);
  if (!r || (4 * ly->Ch16) % 128 || (q == 0 ? ly->Cxp : ly->Chp) % (16 * r->NTC)) return nullptr;
  return r;
}

// THE SPLIT RULE: enough splits of the pixel tiles that `columns` workgroup columns give target_workgroups workgroups, but never
// fewer than NINT_WG_MIN_TILES tiles per split -- the accumulator flush (J KiB-tiles per workgroup) must stay small against the
// K work -- re-derived so that no split is empty.  whole_xcds: rounded down to a multiple of 8 -- workgroup (split, column)
// sits on XCD (split + splits * column) % 8, so all columns of a split, which read the same dG tiles, then share one L2.
#ifndef NINT_WG_MIN_TILES
#define NINT_WG_MIN_TILES 8
#endif
static int wg_splits(int target_workgroups, int columns, int ntiles, bool whole_xcds) {
  int s = nint_cdiv(target_workgroups, columns);
  if (s > ntiles / NINT_WG_MIN_TILES) s = ntiles / NINT_WG_MIN_TILES;
  if (s < 1) s = 1;
  s = nint_cdiv(ntiles, nint_cdiv(ntiles, s));
  if (whole_xcds && s >= 8) s -= s % 8;
  return s;
}

static int wg_plan(const nint_layer* ly, int dtype, int n_cu, int N, const nint_geom* g, WgPlan* pl) {
  pl->NB = 4 * ly->Ch16 / 64;
  const int PR = dtype == NINT_BF16 ? 4 : 2;
  pl->tiles_x = g ? nint_cdiv(g->W, 32) : 1;
  pl->tiles_y = g ? nint_cdiv(g->H, PR) : 1;
  pl->ntiles = g ? N * pl->tiles_x * pl->tiles_y : (1 << 30);
  if (n_cu <= 0) n_cu = 256;
  for (int q = 0; q < 2; ++q) {
    WgPart& w = pl->part[q];
    const int Cp = q == 0 ? ly->Cxp : ly->Chp;
    w.row = wg_wide_row_of(ly, dtype, q);
    if (w.row) {
      // partial slabs in the 4-wave kernel's layout with one channel tile per block (NTC = 1)
      w.KX = ly->k; w.NTC = 1; w.J = ly->k * ly->k; w.TG = 1;
      w.JG = w.J + (q == 0 ? 1 : 0);
      w.CB = Cp / 16;
      w.nblk = pl->NB * w.CB;
      w.cols = (pl->NB / 2) * (w.CB / w.row->NTC);
      w.splits = wg_splits(n_cu, w.cols, pl->ntiles, true);     // one 8-wave workgroup per CU
      continue;
    }
    w.KX = (q == 0 && ly->xfold) ? 1 : ly->k;           // folded x source: vertical taps only
    const int taps = ly->k * w.KX;
    w.NTC = (taps * 2 <= 20 && Cp % 32 == 0) ? 2 : 1;   // channel tiles per column block
    w.J = taps * w.NTC;
    // every wave owns all 4 row tiles (64 gate columns) and a quarter of the (tap, channel-tile) columns
    w.row = wg_find_row(dtype, ly->k, w.NTC, wg_jw(w.J), w.KX);
    if (!w.row) return NINT_E_SHAPE;                    // no such instance: refused here, before any workspace is sized
    const int JW = w.row->JW;
    // more than 4*JW columns (the 49 taps of a 7x7 kernel): column groups on extra workgroups
    w.TG = nint_cdiv(w.J, 4 * JW);
    w.JG = (w.TG == 1 ? w.J : 4 * JW) + (q == 0 ? 1 : 0);     // the x part's slabs carry the bias-gradient column
    const int CW = 16 * w.NTC;
    if (Cp % CW) return NINT_E_SHAPE;
    w.CB = Cp / CW;
    w.cols = w.nblk = pl->NB * w.CB * w.TG;
    // two workgroups per CU in flight.  (NINT_WG_MIN_TILES was 32 until round 3; at B = 1-2 per GPU that left the narrow
    // layers' launches at 92-276 workgroups: 8 measured +2.9 % on the B = 1 step, +0.9 % at B = 2, nothing at B >= 4 where the
    // workgroup cap binds first; 4 and 2 equal 8.)
    w.splits = wg_splits(2 * n_cu, w.cols, pl->ntiles, false);
  }
  // same kernel for both sources and few workgroup columns: one launch, one split count
  WgPart &wx = pl->part[0], &wh = pl->part[1];
  pl->merged = wx.row == wh.row && wx.row->JW && wx.TG == 1 && wh.TG == 1 && wx.cols + wh.cols <= 8;
  // (whole XCDs -- 86 splits for layer 1: 534 us; 80: see DESIGN.md)
  if (pl->merged) wx.splits = wh.splits = wg_splits(2 * n_cu, wx.cols + wh.cols, pl->ntiles, true);
  pl->off_h = wx.splits * wx.slab();
  pl->total_floats = pl->off_h + wh.splits * wh.slab();
  return NINT_OK;
}

extern "C" size_t nint_wgrad_workspace_bytes(const nint_layer* ly, int dtype, int n_cu) {
  if (!ly) return 0;
  WgPlan pl;
  // upper bound independent of N: splits are capped by 2*n_cu / blocks
  if (wg_plan(ly, dtype, n_cu, 1, nullptr, &pl) != NINT_OK) return 0;
  return pl.total_floats * sizeof(float);
}

// Weight / bias gradients of several layers ("jobs") in one go: two MFMA launches per layer (x and h source) into
// consecutive regions of ONE workspace, then ONE launch folds every split-K slab of every layer into its dW and db
// (the x part's slabs carry the bias-gradient column).  Planned here into plans[0..njobs) and *fold -- host arithmetic only --
// and enqueued from those records (below; seq.hip: the last steps of a backward pass).
// h_skip: the first h_skip images have an identically zero h source (h_{-1} = 0 of a sequence that starts from
// the zero state, model.py:259-262): the h part skips them -- 1/T of its work.
int nint_internal_wgrad_plan(const WgJob* jobs, int njobs, const nint_geom* g, int dtype, float* partial, size_t partial_bytes,
                             int n_cu, WgJobPlan* plans, WgFoldPlan* fold) {
  if (!jobs || njobs < 1 || njobs > NINT_MAX_LAYERS || !g || !partial) return NINT_E_ARG;
  if (dtype != NINT_F32 && dtype != NINT_BF16) return NINT_E_ARG;
  const int es = dtype == NINT_BF16 ? 2 : 4;
  ReduceTable& rt = fold->t;
  rt = ReduceTable{};
  size_t off = 0;
  unsigned blk = 0;
  int red_threads = 256;
  for (int q = 0; q < njobs; ++q) {
    const WgJob& jb = jobs[q];
    const nint_layer* ly = jb.ly;
    if (!ly || !jb.dG || !jb.x_slab || !jb.h_slab || !jb.dW || !jb.db || jb.N <= 0) return NINT_E_ARG;
    if (jb.h_skip < 0 || jb.h_skip > jb.N) return NINT_E_ARG;
    WgPlan pl;
    int rc = wg_plan(ly, dtype, n_cu, jb.N, g, &pl);
    if (rc != NINT_OK) return rc;
    if ((off + pl.total_floats) * sizeof(float) > partial_bytes) return NINT_E_ARG;
    float* base = partial + off;
    off += (pl.total_floats + 63) / 64 * 64;
    const int Gc = 4 * ly->Ch16;
    WgradArgs a = {};
    a.dG_pix_stride = Gc * es;
    a.dG_img_stride = (long)g->Hh * g->Wh * a.dG_pix_stride;
    a.k = ly->k; a.p = ly->k / 2;
    a.P = g->P; a.Wh = g->Wh;
    a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y;
    WgJobPlan& jp = plans[q];
    jp.n = 0;
    for (int part = 0; part < 2; ++part) {
      const WgPart& w = pl.part[part];
      WgSrc& S = a.s[pl.merged ? part : 0];
      const int skip = part == 1 ? jb.h_skip : 0;
      S.dG = (const char*)jb.dG + (size_t)skip * a.dG_img_stride;
      const int Cp = part == 0 ? ly->Cxp : ly->Chp;
      S.src_pix_stride = Cp * es;
      S.src_img_stride = (long)g->Hh * g->Wh * S.src_pix_stride;
      S.src = (const char*)(part == 0 ? jb.x_slab : jb.h_slab) + (size_t)skip * S.src_img_stride;
      S.partial = base + (part == 0 ? 0 : pl.off_h);
      S.CB = w.CB; S.JG = w.JG;
      S.nblk = w.nblk;
      S.want_db = part == 0 ? 1 : 0;           // the x part sees every image (the h part may skip the first time step)
      S.ntiles = (jb.N - skip) * pl.tiles_x * pl.tiles_y;  // empty splits flush zeros
      S.tiles_per_split = S.ntiles > 0 ? nint_cdiv(S.ntiles, w.splits) : 1;   // spread what is there evenly over the planned splits
      a.NTC = w.NTC; a.J = w.J; a.TG = w.TG;
      a.taps = ly->k * w.KX;
      if (!pl.merged || part == 1) {           // a launch per source, or both sources in one: filled from the row
        a.nparts = pl.merged ? 2 : 1;
        const int gy = pl.merged ? pl.part[0].cols + w.cols : w.cols;
        jp.launch[jp.n++] = WgLaunch{w.row->kern[dtype], w.splits, gy, w.row->block, w.row->lds[dtype], a};
      }
      ReduceEntry& E = rt.e[rt.n++];
      E.part = S.partial; E.dW = jb.dW; E.db = part == 0 ? jb.db : nullptr;
      E.Cx = ly->Cx; E.Ch = ly->Ch; E.Ch16 = ly->Ch16; E.k = ly->k; E.NB = pl.NB; E.CB = w.CB; E.NTC = w.NTC; E.J = w.J;
      E.splits = w.splits; E.is_h = part; E.xfold = ly->xfold; E.TG = w.TG; E.JG = w.JG;
      E.blk_begin = blk;
      blk += (unsigned)(w.slab() / 256);
      E.waves = 4;                               // 4 waves share the splits of a 256-element line (16-wave workgroups for the
                                                 // many-split entries made every entry's workgroup 1024 threads: 46 -> 40 us)
      if (E.waves * 64 > red_threads) red_threads = E.waves * 64;
    }
  }
  fold->grid = blk; fold->block = red_threads;
  return NINT_OK;
}

int nint_internal_wgrad_enqueue(const WgJobPlan* jp, void* stream) {
  for (int i = 0; i < jp->n; ++i) {
    const WgLaunch& l = jp->launch[i];
    if (l.lds > 64 * 1024)
      NINT_CHECK_HIP(hipFuncSetAttribute(l.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
    void* args[] = {(void*)&l.a};
    (void)hipLaunchKernel(l.kern, dim3(l.gx, l.gy), dim3(l.block), args, l.lds, (hipStream_t)stream);
    NINT_LAUNCH_CHECK();
  }
  return NINT_OK;
}

int nint_internal_wgrad_fold_enqueue(const WgFoldPlan* fp, void* stream) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(fp->grid), dim3(fp->block), 0, (hipStream_t)stream, fp->t);
  NINT_LAUNCH_CHECK();
  return NINT_OK;
}

extern "C" int nint_conv_wgrad(const nint_layer* ly, const nint_geom* g, int dtype, int N, const void* dG,
                               const void* x_slab, const void* h_slab, float* dW, float* db, float* partial,
                               size_t partial_bytes, int n_cu, void* stream) {
  const WgJob jb = {ly, N, dG, x_slab, h_slab, dW, db, 0};
  WgJobPlan jp; WgFoldPlan fold;
  int rc = nint_internal_wgrad_plan(&jb, 1, g, dtype, partial, partial_bytes, n_cu, &jp, &fold);
  if (rc == NINT_OK) rc = nint_internal_wgrad_enqueue(&jp, stream);
  return rc != NINT_OK ? rc : nint_internal_wgrad_fold_enqueue(&fold, stream);
}

// ------------------------------------------------------------------------------ the plan, for tests and tools
extern "C" int nint_debug_wgrad_plan(const nint_layer* ly, const nint_geom* g, int dtype, int N, int h_skip, int n_cu,
                                     nint_wgrad_plan_rec* out) {
  if (!out) return NINT_E_ARG;
  float* const base = (float*)(uintptr_t)4096;              // made up: the planner dereferences no job pointer
  const WgJob jb = {ly, N, base, base, base, base, base, h_skip};
  WgJobPlan jp; WgFoldPlan fold;
  const int rc = nint_internal_wgrad_plan(&jb, 1, g, dtype, base, ly ? nint_wgrad_workspace_bytes(ly, dtype, n_cu) : 0, n_cu, &jp, &fold);
  if (rc != NINT_OK) return rc;
  *out = nint_wgrad_plan_rec{};
  out->n_launch = jp.n; out->n_fold = fold.t.n; out->fold_grid = (int)fold.grid; out->fold_block = fold.block;
  for (int i = 0; i < jp.n; ++i) {
    const WgLaunch& l = jp.launch[i];
    nint_wgrad_launch_rec& r = out->launch[i];
    for (const WgRow& row : wg_rows)               // the instance, from the handle the launch carries
      if (row.kern[dtype] == l.kern) { r.family = row.block / 64; r.KS = row.KS; r.NTC = row.NTC; r.JW = row.JW; r.KX = row.KX; }
    r.nparts = l.a.nparts; r.gx = l.gx; r.gy = l.gy; r.block = l.block; r.lds = (int)l.lds;
    for (int q = 0; q < l.a.nparts; ++q) {
      const WgSrc& S = l.a.s[q];
      r.src[q] = nint_wgrad_src_rec{S.CB, S.JG, l.a.TG, S.nblk, S.ntiles, S.tiles_per_split, S.want_db, jp.n == 1 ? q : i, S.partial - base};
    }
  }
  for (int i = 0; i < fold.t.n; ++i) {
    out->fold[i].blk_begin = (int)fold.t.e[i].blk_begin; out->fold[i].splits = fold.t.e[i].splits; out->fold[i].waves = fold.t.e[i].waves;
  }
  return NINT_OK;
}
