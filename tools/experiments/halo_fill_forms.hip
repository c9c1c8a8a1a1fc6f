// halo_fill_forms.hip -- the conv kernels' halo-tile fill, alone: which FORM of the fill is fastest at the three tile shapes the
// bench step runs?  (csrc/conv_igemm.hip stages its A operand this way at the top of every workgroup.)
//
// A workgroup (4 waves) fills the LDS image of one halo tile from channels-last slabs, waits, passes a barrier and then reads
// the image once with fragment-shaped ds_read_b128 (16 consecutive pixels x 4 lane groups g, as the K loop does), so the fill
// cannot be optimised away and a wrong mapping shows in the checksum.  Forms:
//   a   today's: LDS-DMA pieces of 64 consecutive pixels of one (chunk, g) plane -> 64 cache lines per wave instruction
//   b   LDS-DMA pieces of 16 pixels x 4 quarters (lanes 4j..4j+3 = pixel j) -> 16 lines; the image is pixel-major inside a
//       16-pixel block, [chunk][block][j][slot][16 B], and lane 4j+s fetches quarter q(j, s) such that the fragment read of lane
//       group g at pixel j finds its quarter in slot(j, g) = 2*(g&1) + (((j>>2)&1) ^ (g>>1)): conflict-free for every tap
//       alignment under the 16-lane groups of ds_read_b128 ({0-3,12-15,20-27}, {4-11,16-19,28-31}, and the same + 32)
//   c   global_load_dwordx4 with the lane -> (pixel, quarter) mapping of b, then ds_write_b128 into today's [chunk][g][pixel]
//       planes; the plane stride is padded by PAD bytes (c64 = an odd number of 64-byte units, c32, c0 = today's stride)
// Grid = 256 x (workgroups per CU); every round of every launch takes fresh tiles of a slab set larger than the Infinity Cache.
//   hipcc -O3 --offload-arch=gfx950 -o halo_fill_forms tools/experiments/halo_fill_forms.hip
//   ./halo_fill_forms            timing table (us per fill: median / min / max of the repeats)
//   ./halo_fill_forms pmc        one launch per (shape, form), every tap alignment read: for a SQ_LDS_BANK_CONFLICT run of its own
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

struct FillArgs {
  const char* src0; const char* src1;
  int nchunk0, nchunk1, pix0, pix1;        // 64-byte chunks and bytes per pixel of either source
  long img0, img1;                         // bytes per image
  int Wh, tiles_x, tiles_y, n_tiles;       // slab row pitch in pixels; tiles per image; tiles in the slab set
  int MT, HWt, NHP, NHPp;                  // tile rows, halo width, halo pixels, padded to 16
  unsigned magic_nhpp, magic_hwt, magic_blk;   // ceil(2^32 / d) for d = NHPp, HWt, NHPp / 16
  int plane;                               // bytes of one g plane (forms a, c)
  int rounds, tile_start, sweep_step;
  unsigned* sums;                          // [workgroup][256] checksums
  unsigned long long* stamps;              // [workgroup][2]: fill clocks (shader, 100 MHz) summed over the rounds
};

__device__ __forceinline__ int slot_of(int j, int g) { return 2 * (g & 1) + (((j >> 2) & 1) ^ (g >> 1)); }
__device__ __forceinline__ int quarter_of(int j, int s) { return (s >> 1) | (((s & 1) ^ ((j >> 2) & 1)) << 1); }

template <int FORM, int PPW>     // PPW: pieces per wave, form c holds them all in registers
__global__ __launch_bounds__(256) void fill_kernel(const FillArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = a.nchunk0 + a.nchunk1;
  const int NHP = a.NHP, NHPp = a.NHPp, HWt = a.HWt, plane = a.plane;
  const int nblk = NHPp / 16;
  unsigned sum = 0;
  unsigned long long clk = 0, rt = 0;
  // XCD-contiguous tile order, as the kernels: workgroup b runs on XCD b % 8
  int tile_in_grid;
  {
    const int nb = gridDim.x, b = blockIdx.x, q8 = nb / 8, r8 = nb % 8, x = b % 8, i = b / 8;
    tile_in_grid = x * q8 + (x < r8 ? x : r8) + i;
  }
  for (int r = 0; r < a.rounds; ++r) {
    int tile = (int)(((long)a.tile_start + (long)r * gridDim.x + tile_in_grid) % a.n_tiles);
    const int tx = tile % a.tiles_x; tile /= a.tiles_x;
    const int ty = tile % a.tiles_y;
    const int img = tile / a.tiles_y;
    const long org = (long)(ty * a.MT) * a.Wh + tx * 16;
    const char* base0 = a.src0 + img * a.img0 + org * a.pix0;
    const char* base1 = a.src1 ? a.src1 + img * a.img1 + org * a.pix1 : nullptr;
    auto src_of = [&](int c, int hp, int q) __attribute__((always_inline)) {
      hp = hp < NHP ? hp : 0;                  // pad pixels re-read pixel 0
      const int hy = (int)__umulhi((unsigned)hp, a.magic_hwt);
      const int hx = hp - hy * HWt;
      return (c < a.nchunk0) ? base0 + ((long)hy * a.Wh + hx) * a.pix0 + c * 64 + q * 16
                             : base1 + ((long)hy * a.Wh + hx) * a.pix1 + (c - a.nchunk0) * 64 + q * 16;
    };
    const unsigned long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    if constexpr (FORM == 0) {
      const int a_units = nchunks * 4 * NHPp;
      for (int ub = wave * 64; ub < a_units; ub += 4 * 64) {
        const int u = ub + lane;
        const int cq = (int)__umulhi((unsigned)u, a.magic_nhpp);
        const int hp = u - cq * NHPp;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src_of(cq >> 2, hp, cq & 3),
                                         (__attribute__((address_space(3))) void*)(smem + (size_t)ub * 16), 16, 0, 0);
      }
    } else if constexpr (FORM == 1) {
      const int pieces = nchunks * nblk;
      const int j = lane >> 2, q = quarter_of(j, lane & 3);
      for (int pc = wave; pc < pieces; pc += 4) {
        const int c = (int)__umulhi((unsigned)pc, a.magic_blk);
        const int hp = (pc - c * nblk) * 16 + j;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src_of(c, hp, q),
                                         (__attribute__((address_space(3))) void*)(smem + (size_t)pc * 1024), 16, 0, 0);
      }
    } else {
      const int pieces = nchunks * nblk;
      const int j = lane >> 2, q = lane & 3;
      u32x4_t v[PPW];
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int pc = min(wave + 4 * i, pieces - 1);
        const int c = (int)__umulhi((unsigned)pc, a.magic_blk);
        const int hp = (pc - c * nblk) * 16 + j;
        v[i] = *(const u32x4_t*)src_of(c, hp, q);
      }
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int pc = wave + 4 * i;
        const int c = (int)__umulhi((unsigned)min(pc, pieces - 1), a.magic_blk);
        const int hp = (pc - c * nblk) * 16 + j;
        if (pc < pieces) *(u32x4_t*)(smem + (c * 4 + q) * plane + hp * 16) = v[i];
      }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned long long c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    clk += c1 - c0; rt += r1 - r0;
    // fragment-shaped sweep: lane group g, 16 consecutive pixels from `b`; sweep_step 17 reads the image about once,
    // sweep_step 1 reads every tap alignment
    const int g = lane >> 4, x = lane & 15;
    for (int c = 0; c < nchunks; ++c)
      for (int b = wave * a.sweep_step; b + 16 <= NHPp; b += 4 * a.sweep_step) {
        const int hp = b + x;
        int off;
        if constexpr (FORM == 1) off = c * (NHPp * 64) + (hp >> 4) * 1024 + (hp & 15) * 64 + slot_of(hp & 15, g) * 16;
        else off = (c * 4 + g) * plane + hp * 16;
        const u32x4_t w = *(const u32x4_t*)(smem + off);
        sum += (w[0] ^ (w[1] * 3u)) + (w[2] ^ (w[3] * 5u)) * (unsigned)(1 + c + 4 * g + 16 * hp);   // weighted by the LOGICAL position
      }
    __syncthreads();                           // the next round overwrites the image
  }
  a.sums[(size_t)blockIdx.x * 256 + tid] = sum;
  if (tid == 0) { a.stamps[blockIdx.x * 2] = clk; a.stamps[blockIdx.x * 2 + 1] = rt; }
}

__global__ void init_kernel(unsigned* p, size_t n, unsigned seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = h;
  }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

struct Shape { const char* name; int MT, p, nchunk0, nchunk1, wpc; };
static const Shape SHAPES[3] = {
  {"8-row 12x20, 4 chunks of a 256-B pixel, 2 wg/CU", 8, 2, 4, 0, 2},
  {"8-row 10x18, 3 chunks of 128+64-B pixels, 2 wg/CU", 8, 1, 2, 1, 2},
  {"4-row 6x18, 2 chunks of 64+64-B pixels, 4 wg/CU", 4, 1, 1, 1, 4},
};
struct Form { const char* name; int form, pad; };
static const Form FORMS[5] = {{"a", 0, 0}, {"b", 1, 0}, {"c64", 2, 64}, {"c32", 2, 32}, {"c0", 2, 0}};

static unsigned magic(int d) { return (unsigned)((0x100000000ull + d - 1) / d); }

template <int PPW>
static void launch(int form, int grid, int lds, const FillArgs& a) {
  if (form == 0) hipLaunchKernelGGL((fill_kernel<0, PPW>), dim3(grid), dim3(256), lds, 0, a);
  else if (form == 1) hipLaunchKernelGGL((fill_kernel<1, PPW>), dim3(grid), dim3(256), lds, 0, a);
  else hipLaunchKernelGGL((fill_kernel<2, PPW>), dim3(grid), dim3(256), lds, 0, a);
}

int main(int argc, char** argv) {
  const bool pmc = argc > 1 && !strcmp(argv[1], "pmc");
  const int rounds = pmc ? 2 : 16, repeats = pmc ? 1 : 15, warm = pmc ? 0 : 2;
  const size_t SLAB = (size_t)640 << 20;       // bytes of the slab set: 2.5 x the 256 MiB Infinity Cache
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  printf("halo fill forms: %d rounds per launch, %d repeats; us per fill = median [min .. max] of the repeats\n", rounds, repeats);
  printf("  stamp = issue -> landed -> barrier, mean over the workgroups (100 MHz clock); launch = kernel time / rounds, sweep included\n");
  for (int si = 0; si < 3; ++si) {
    const Shape& s = SHAPES[si];
    FillArgs a; memset(&a, 0, sizeof a);
    a.MT = s.MT; a.HWt = 16 + 2 * s.p; a.NHP = (s.MT + 2 * s.p) * a.HWt; a.NHPp = (a.NHP + 15) / 16 * 16;
    a.nchunk0 = s.nchunk0; a.nchunk1 = s.nchunk1; a.pix0 = 64 * s.nchunk0; a.pix1 = 64 * s.nchunk1;
    a.tiles_x = 10; a.tiles_y = 96 / s.MT;     // the 100 x 154 grid's full tiles
    const int Hh = a.tiles_y * s.MT + 2 * s.p; a.Wh = a.tiles_x * 16 + 2 * s.p;      // every halo tile inside its image
    a.img0 = (long)Hh * a.Wh * a.pix0; a.img1 = (long)Hh * a.Wh * a.pix1;
    const int n_img = (int)(SLAB / (size_t)(a.img0 + a.img1)) ;
    a.n_tiles = n_img * a.tiles_x * a.tiles_y;
    a.magic_nhpp = magic(a.NHPp); a.magic_hwt = magic(a.HWt); a.magic_blk = magic(a.NHPp / 16);
    a.rounds = rounds; a.sweep_step = pmc ? 1 : 17;
    const int grid = 256 * s.wpc, nchunks = s.nchunk0 + s.nchunk1;
    char *d0 = nullptr, *d1 = nullptr;
    CK(hipMalloc(&d0, (size_t)n_img * a.img0));
    init_kernel<<<2048, 256>>>((unsigned*)d0, (size_t)n_img * a.img0 / 4, 1u);
    if (a.nchunk1) { CK(hipMalloc(&d1, (size_t)n_img * a.img1)); init_kernel<<<2048, 256>>>((unsigned*)d1, (size_t)n_img * a.img1 / 4, 2u); }
    a.src0 = d0; a.src1 = d1;
    CK(hipMalloc(&a.sums, (size_t)grid * 256 * 4)); CK(hipMalloc(&a.stamps, (size_t)grid * 16));
    CK(hipDeviceSynchronize());
    printf("\n%s: halo %d px (padded %d), %d images, grid %d\n", s.name, a.NHP, a.NHPp, n_img, grid);
    unsigned long long ref_sum = 0;
    for (int fi = 0; fi < 5; ++fi) {
      const Form& f = FORMS[fi];
      a.plane = a.NHPp * 16 + f.pad;
      const int image = f.form == 1 ? nchunks * a.NHPp * 64 : nchunks * 4 * a.plane;
      // dynamic LDS sized so that exactly wpc workgroups fit a CU's 160 KiB
      const int lds = std::max(image, 160 * 1024 / (s.wpc + 1) + 1024);
      if (lds > 64 * 1024 || lds * s.wpc > 160 * 1024) { printf("form %s: LDS %d does not fit\n", f.name, lds); return 1; }
      const int pieces = nchunks * a.NHPp / 16, ppw = (pieces + 3) / 4;
      std::vector<float> us_launch, us_stamp, mhz;
      std::vector<unsigned> hs((size_t)grid * 256);
      std::vector<unsigned long long> st((size_t)grid * 2);
      unsigned long long first_sum = 0;
      for (int rep = -warm; rep < repeats; ++rep) {
        a.tile_start = (int)(((long)(rep + warm) * rounds * grid) % a.n_tiles);     // the same tiles for every form
        CK(hipEventRecord(e0, 0));
        if (ppw <= 4) launch<4>(f.form, grid, lds, a);
        else if (ppw <= 9) launch<9>(f.form, grid, lds, a);
        else if (ppw <= 15) launch<15>(f.form, grid, lds, a);
        else { printf("pieces per wave %d\n", ppw); return 1; }
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep < 0) continue;
        CK(hipMemcpy(st.data(), a.stamps, st.size() * 8, hipMemcpyDeviceToHost));
        double sc = 0, sr = 0;
        for (int w = 0; w < grid; ++w) { sc += (double)st[2 * w]; sr += (double)st[2 * w + 1]; }
        us_launch.push_back(ms * 1000.f / rounds);
        us_stamp.push_back((float)(sr / grid / rounds / 100.0));
        mhz.push_back((float)(sc / (sr / 100.0)));
        if (rep == 0) {
          CK(hipMemcpy(hs.data(), a.sums, hs.size() * 4, hipMemcpyDeviceToHost));
          for (unsigned v : hs) first_sum += v;
        }
      }
      if (fi == 0) ref_sum = first_sum;
      std::sort(us_launch.begin(), us_launch.end()); std::sort(us_stamp.begin(), us_stamp.end()); std::sort(mhz.begin(), mhz.end());
      const int m = repeats / 2;
      printf("  form %-3s  stamp %6.2f [%6.2f .. %6.2f]   launch %6.2f [%6.2f .. %6.2f]   %4.0f MHz   LDS %5d   checksum %s\n", f.name,
             us_stamp[m], us_stamp.front(), us_stamp.back(), us_launch[m], us_launch.front(), us_launch.back(), mhz[m], lds,
             first_sum == ref_sum ? "= a" : "DIFFERS");
    }
    CK(hipFree(d0)); if (d1) CK(hipFree(d1)); CK(hipFree(a.sums)); CK(hipFree(a.stamps));
  }
  return 0;
}
