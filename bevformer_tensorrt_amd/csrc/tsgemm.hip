// Tall-skinny fp16 GEMM on the matrix cores for the dense layers that wrap the samplers (SURVEY.md 8a-5:
// value_proj / output_proj / FFN of the encoder, the 1x1 convolutions of the channels-last backbone):
//     out[m, n] = act( sum_k x[m, k] * w[n, k] + bias[n] (+ residual[m, n]) ),   M >> N, K
// x [M, K] and w [N, K] row-major fp16 (nn.Linear / 1x1-conv weight layout), fp32 accumulation, ONE rounding
// to fp16.  These layers are memory-bound at batch 1 (the 1024 -> 256 convolution of ResNet stage 3 moves
// 89 MB for 18 GFLOP): what matters is that every CU streams its share of x exactly once, at full rate,
// with the weight slices coming from L2.  The library's tile shapes leave a third of the chip idle on
// M = 34 800 (272 tiles of 128 rows on 256 CUs -> two rounds); here
//   * the rows are split in units of 32 over ONE persistent block per CU (a CU gets 4 or 5 units at
//     M = 34 800; 85 % balance instead of 53 %), processed as tiles of up to 160 rows x 256 columns;
//   * both operands go global -> LDS by DMA (buffer_load ... lds, no VGPRs), 64 k-values per step, two
//     LDS stages, one barrier per step; LDS rows are 128 bytes with the 16-byte chunks XOR-swizzled (applied
//     to the DMA's SOURCE address, the DMA being lane-linear), so the ds_read_b128 fragment reads are
//     conflict-free (the scheme of the DCNv2 kernel, mdconv.hip);
//   * wave w owns columns 32 w .. 32 w + 31 of the tile for ALL its row units (v_mfma_f32_32x32x16_f16, up
//     to 5 accumulator tiles per wave): one weight fragment per k-substep is reused by 5 matrix
//     instructions;
//   * the epilogue goes through LDS in fp32 (two column halves): threads then own 16 contiguous bytes
//     of an output row, so bias / residual / ReLU are evaluated in fp32 on coalesced 16-byte accesses and
//     rounded once -- or, for the encoder's value projection, the row is written straight into the padded
//     head-major planes the SCA sampler reads (msda_pad.h: pixel-pair entries of the big levels, row-major
//     pixels of the staged ones), which removes the separate re-layout pass (70 us per SCA call).
// N > 256: grid.y walks the 256-column chunks.  Domain: K % 64 == 0, N % 256 == 0 (other layers stay on
// hipBLASLt).  K <= 256 runs on the weight-stationary flavour further down (tsgemm_ws_kernel); this kernel stays
// for K > 256 and as its A/B partner (bevops_tsgemm_set_variant).
#include <stdlib.h>

#include <type_traits>

#include "gemm_host.h"
#include "mdconv.h"
#include "msda_pad.h"

namespace bevops {
namespace {

constexpr int kTsBN = 256;      // columns per tile
constexpr int kTsG = 5;         // row units (of 32) per tile
constexpr int kTsThreads = 512;
constexpr int kTsW = kTsBN * 128;          // weight stage image (32 KB)
constexpr int kTsX = kTsG * 32 * 128;      // activation stage image (20 KB)
constexpr int kTsStage = kTsW + kTsX;
constexpr int kTsEpiStride = 128 * 4 + 16; // fp32 staging row (128 columns) + bank pad
constexpr int kTsStages = 3;               // two k-steps of DMA in flight behind the one being multiplied
constexpr int kTsLds = kTsStages * kTsStage;   // 156 KB; the epilogue staging (160 x 528 = 82.5 KB) reuses it
constexpr int kTsS8LnLds = kTsLds + 2 * kTsBN * 2;   // tsgemm_s8_kernel<2>: + the norm's weight and bias, fp16 [256] each

struct TsPacked {   // EPI == 1: destination of the encoder's value projection
  char *gset, *sset;   // (EPI == 2: the LayerNorm's weight and bias, fp16 [N])
  Hm3Tab t;
  int nk, heads;    // rows per camera, heads (N == heads * 32)
  float eps;        // EPI == 2
  long long gstride;   // grouped EPI 0 (tsgemm_ws_grouped_kernel<KS>): elements between the outputs of two column chunks
};

// sum over the 16 lanes of a DPP row (= the 16 threads that share an output row in the epilogue), in every lane
__device__ __forceinline__ float row16_sum(float v) {
  v = quad_sum(v);
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));   // row_half_mirror
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true));   // row_mirror
}

typedef __attribute__((address_space(3))) void lds_void_t;

// Staging accesses of the weight-stationary kernel, written as instructions: the compiler orders every LDS access it
// emits itself behind ALL outstanding LDS-DMA (s_waitcnt vmcnt(0)), which would drain the row prefetch in front of each
// epilogue.  The staging rows never overlap the DMA's row images; the kernel waits for its own writes (lgkmcnt) itself.
__device__ __forceinline__ unsigned lds_addr(const void *p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)p;
}
template <int OFF>
__device__ __forceinline__ void lds_write16(unsigned addr, f32x4 v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
__device__ __forceinline__ void lds_read32(unsigned addr, float (&v)[8]) {   // 32 bytes, waited for
  f32x4 a, b;
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(a), "=&v"(b)
               : "v"(addr)
               : "memory");
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}

// ---- per-thread epilogue arithmetic shared by the weight-stationary kernel below (a thread owns 8 consecutive columns
// of one output row, fp32 values `v` read back from the staging rows)
__device__ __forceinline__ void ts_add_res(float (&v)[8], const uint4 q) {
  v[0] += h2f_lo(q.x); v[1] += h2f_hi(q.x); v[2] += h2f_lo(q.y); v[3] += h2f_hi(q.y);
  v[4] += h2f_lo(q.z); v[5] += h2f_hi(q.z); v[6] += h2f_lo(q.w); v[7] += h2f_hi(q.w);
}
__device__ __forceinline__ uint4 ts_pack8(const float (&v)[8]) {
  uint4 o;
  o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
  return o;
}
__device__ __forceinline__ float ts_sum8(const uint4 o) {
  return (h2f_lo(o.x) + h2f_hi(o.x)) + (h2f_lo(o.y) + h2f_hi(o.y)) + (h2f_lo(o.z) + h2f_hi(o.z)) +
         (h2f_lo(o.w) + h2f_hi(o.w));
}

// EPI 1: row m (tile row r of `rows`, columns col .. col + 7) into the padded planes.  `stage` is the fp32 staging image
// of the tile's current 128-column half (rows of kTsEpiStride bytes): the right neighbour's values come from there.
__device__ __forceinline__ void ts_store_planes(const float (&v)[8], const TsPacked &pk, size_t m, int col, int r, int rows,
                                                int c8, const char *stage) {
  // row m = pixel `s` of camera `cam`; column chunk -> (head, channels 8 q .. 8 q + 7)
  const int cam = (int)(m / (size_t)pk.nk), s = (int)(m - (size_t)cam * pk.nk);
  const int head = col >> 5, q8 = (col & 31) >> 3;
  // the level's constants by compare-and-select over the (scalar) table: indexing the by-value table with a per-lane
  // level would be vector loads from the argument segment, and waiting for those waits for the row prefetch as well
  int l = 0, src0 = pk.t.src0[0], Wl = pk.t.W[0], ent0 = pk.t.ent0[0];
#pragma unroll
  for (int k = 1; k < kHm3MaxLevels; ++k)
    if (k < pk.t.L && s >= pk.t.src0[k]) { l = k; src0 = pk.t.src0[k]; Wl = pk.t.W[k]; ent0 = pk.t.ent0[k]; }
  const int rel = s - src0;
  const int y = rel / Wl, xx = rel - y * Wl;
  const int wp = Wl + 1;
  const int f = ent0 + (y + 1) * wp + xx;        // padded entry of this pixel
  const size_t plane = (size_t)cam * pk.heads + head;
  const unsigned h0 = pack_h2(v[0], v[1]), h1 = pack_h2(v[2], v[3]), h2 = pack_h2(v[4], v[5]), h3 = pack_h2(v[6], v[7]);
  if (l >= pk.t.ls) {   // staged level: row-major 64 B per pixel
    *reinterpret_cast<uint4 *>(pk.sset + (plane * pk.t.s_entries + f) * kLdsPixBytes + q8 * 16) = make_uint4(h0, h1, h2, h3);
    return;
  }
  // big level: entry f = (this pixel, right neighbour), entry f - 1 = (left neighbour, this pixel); this thread writes
  // the halves that hold ITS pixel: the .lo lanes of entry f and the .hi lanes of entry f - 1
  float nb[8];
  const bool has_r = xx + 1 < Wl && r + 1 < rows;
  const bool own_r = xx + 1 < Wl;
  if (has_r) {
    lds_read32(lds_addr(stage + (r + 1) * kTsEpiStride + c8 * 32), nb);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) nb[k] = 0.f;
  }
  char *e = pk.gset + (plane * pk.t.g_entries + f) * kEntBytes + q8 * 32;
  if (has_r || !own_r) {   // the whole entry is known here: (mine, right) or (mine, pad)
    uint4 o0, o1;
    o0.x = pack_h2(v[0], nb[0]); o0.y = pack_h2(v[1], nb[1]); o0.z = pack_h2(v[2], nb[2]); o0.w = pack_h2(v[3], nb[3]);
    o1.x = pack_h2(v[4], nb[4]); o1.y = pack_h2(v[5], nb[5]); o1.z = pack_h2(v[6], nb[6]); o1.w = pack_h2(v[7], nb[7]);
    *reinterpret_cast<uint4 *>(e) = o0;
    *reinterpret_cast<uint4 *>(e + 16) = o1;
  } else {                 // right neighbour lives in the next tile: only my halves (2-byte stores)
    unsigned short *e16 = reinterpret_cast<unsigned short *>(e);
    const unsigned hv[4] = {h0, h1, h2, h3};
#pragma unroll
    for (int k = 0; k < 4; ++k) { e16[4 * k] = (unsigned short)(hv[k] & 0xffffu); e16[4 * k + 2] = (unsigned short)(hv[k] >> 16); }
  }
  if (xx == 0) {           // entry f - 1 is the pad before the row: (0, mine)
    uint4 o0, o1;
    o0.x = h0 << 16; o0.y = h0 & 0xffff0000u; o0.z = h1 << 16; o0.w = h1 & 0xffff0000u;
    o1.x = h2 << 16; o1.y = h2 & 0xffff0000u; o1.z = h3 << 16; o1.w = h3 & 0xffff0000u;
    *reinterpret_cast<uint4 *>(e - kEntBytes) = o0;
    *reinterpret_cast<uint4 *>(e - kEntBytes + 16) = o1;
  } else if (r == 0) {     // left neighbour lives in the previous tile: my halves of entry f - 1
    unsigned short *e16 = reinterpret_cast<unsigned short *>(e - kEntBytes);
    const unsigned hv[4] = {h0, h1, h2, h3};
#pragma unroll
    for (int k = 0; k < 4; ++k) { e16[4 * k + 1] = (unsigned short)(hv[k] & 0xffffu); e16[4 * k + 3] = (unsigned short)(hv[k] >> 16); }
  }
}

// EPI 2: LayerNorm of one row of 256 from its rounded sums (`lo` / `hi8`: this thread's 8 columns of the two 128-column
// halves, `rs`: their fp32 sum), the 16 threads of the row in one DPP row; two passes, one rounding.
// `gb`: the norm's weight and bias for this thread's columns, {weight, bias} of half 0, then of half 1 (ts_ln_params).
__device__ __forceinline__ void ts_ln_params(const TsPacked &pk, int c8, uint4 (&gb)[4]) {
  const __half *gam = reinterpret_cast<const __half *>(pk.gset), *bet = reinterpret_cast<const __half *>(pk.sset);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    gb[2 * h] = *reinterpret_cast<const uint4 *>(gam + h * 128 + c8 * 8);
    gb[2 * h + 1] = *reinterpret_cast<const uint4 *>(bet + h * 128 + c8 * 8);
  }
}
__device__ __forceinline__ void ts_ln_row(const uint4 lo, const uint4 hi8, float rs, float eps, const uint4 (&gb)[4],
                                          __half *out_row, int c8) {
  const float mean = row16_sum(rs) * (1.f / 256.f);
  float f[16];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint4 o = h ? hi8 : lo;
    f[8 * h + 0] = h2f_lo(o.x) - mean; f[8 * h + 1] = h2f_hi(o.x) - mean;
    f[8 * h + 2] = h2f_lo(o.y) - mean; f[8 * h + 3] = h2f_hi(o.y) - mean;
    f[8 * h + 4] = h2f_lo(o.z) - mean; f[8 * h + 5] = h2f_hi(o.z) - mean;
    f[8 * h + 6] = h2f_lo(o.w) - mean; f[8 * h + 7] = h2f_hi(o.w) - mean;
  }
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) sq = fmaf(f[k], f[k], sq);
  const float rstd = rsqrtf(row16_sum(sq) * (1.f / 256.f) + eps);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int col = h * 128 + c8 * 8;
    const uint4 g4 = gb[2 * h], b4 = gb[2 * h + 1];
    const float gg[8] = {h2f_lo(g4.x), h2f_hi(g4.x), h2f_lo(g4.y), h2f_hi(g4.y),
                         h2f_lo(g4.z), h2f_hi(g4.z), h2f_lo(g4.w), h2f_hi(g4.w)};
    const float bb[8] = {h2f_lo(b4.x), h2f_hi(b4.x), h2f_lo(b4.y), h2f_hi(b4.y),
                         h2f_lo(b4.z), h2f_hi(b4.z), h2f_lo(b4.w), h2f_hi(b4.w)};
    float y[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = fmaf(f[8 * h + k] * rstd, gg[k], bb[k]);
    *reinterpret_cast<uint4 *>(out_row + col) = ts_pack8(y);
  }
}

// EPI 0: out = act(acc + bias (+ residual)) -> [M, N] fp16.  EPI 1: acc + bias -> packed planes.
// EPI 2 (round 6, N == 256): out = LayerNorm(fp16(acc + bias + residual)) -- the layer the encoder / decoder blocks put
// behind output_proj and the FFN's second linear (modules/encoder.py:586-636: attention or FFN, then norm).  A thread
// owns the same 8 columns of the same rows in both 128-column halves of the epilogue, so the rounded sums of a row stay
// in registers (5 rows x 2 halves x 16 bytes) and its mean / variance are two 16-lane DPP reductions: the row is
// normalised from exactly the binary16 values the unfused pair (GEMM, then bevops_layer_norm) would have read back,
// two passes (mean, then centred squares), one rounding; no second launch, no 20 MB written and re-read.
template <int EPI>
__global__ __launch_bounds__(kTsThreads) void tsgemm_f16_kernel(const __half *__restrict__ x,
                                                                const __half *__restrict__ w,
                                                                const __half *__restrict__ bias,
                                                                const __half *__restrict__ res,
                                                                __half *__restrict__ out, int M, int N, int K,
                                                                int relu, int units_total, TsPacked pk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.y * kTsBN;
  // this block's row units: a contiguous range, the first (units_total % grid) blocks take one more
  const int nb = gridDim.x, bi = blockIdx.x;
  const int per = units_total / nb, extra = units_total % nb;
  const int u_begin = bi * per + min(bi, extra);
  const int u_end = u_begin + per + (bi < extra ? 1 : 0);
  if (u_begin >= u_end) return;

  const __amdgpu_buffer_rsrc_t rs_x =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__half *>(x), 0, (unsigned)((size_t)M * K * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__half *>(w), 0, (unsigned)((size_t)N * K * 2), 0x00020000);
  // DMA roles.  Weight tile: 32 pieces of 8 rows, 4 per wave; activation tile: up to 20 pieces, piece
  // wave + 8 j.  lane -> (row in piece, 16-byte chunk); the swizzle sits on the source chunk
  const unsigned prow = (unsigned)(lane >> 3), pchunk = (unsigned)(lane & 7);
  unsigned w_off[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned row = (unsigned)((wave * 4 + j) * 8) + prow;
    w_off[j] = (unsigned)(((size_t)(n0 + row) * K) * 2) + ((pchunk ^ swz8(row)) << 4);
  }
  const unsigned hi = (unsigned)(lane >> 5);
  const unsigned fa = (unsigned)(wave * 32 + (lane & 31));   // weight fragment row
  const int nk = K / 64;

  // column constants of this lane: acc[g][4 rq + e] is column wave * 32 + 8 rq + 4 hi + e
  float bcol[16];
#pragma unroll
  for (int rq = 0; rq < 4; ++rq)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      bcol[4 * rq + e] = bias ? __half2float(bias[n0 + wave * 32 + 8 * rq + 4 * (int)hi + e]) : 0.f;

  for (int u0 = u_begin; u0 < u_end; u0 += kTsG) {
    const int G = min(kTsG, u_end - u0);
    const int r0 = u0 * 32;
    const int pieces_x = G * 4;
    unsigned x_off[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned row = (unsigned)((wave + 8 * j) * 8) + prow;
      x_off[j] = (unsigned)(((size_t)(r0 + row) * K) * 2) + ((pchunk ^ swz8(row)) << 4);
    }
    // every resident block walks the same weight matrix: start each one at a different k-slice (and wrap), so
    // that the CUs of an XCD do not pull the same 32 KB from the same L2 channels in the same step (the fp32
    // summation order then depends on the block index only)
    const int k_rot = bi % nk;
    auto dma = [&](int step, int buf) {
      char *wd = smem + buf * kTsStage + wave * 4096;
      int kstep = step + k_rot;
      if (kstep >= nk) kstep -= nk;
      const int soff = kstep * 128;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void_t *)(wd + j * 1024), 16, (int)w_off[j], soff, 0, 0);
      char *xd = smem + buf * kTsStage + kTsW;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (wave + 8 * j < pieces_x)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void_t *)(xd + (wave + 8 * j) * 1024), 16,
                                                   (int)x_off[j], soff, 0, 0);
    };
    f32x16 acc[kTsG];
#pragma unroll
    for (int g = 0; g < kTsG; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;

    // three LDS stages: the DMA of steps s + 1 and s + 2 is in flight while step s is multiplied (x comes
    // from HBM: one step of cover leaves its latency exposed on every step).  A wave waits for ITS pieces
    // of step s (vmcnt counts its own DMA instructions: 4 weight pieces + 0..3 activation pieces per
    // step), the barrier then makes everybody's pieces visible -- and also says that stage (s + 2) % 3,
    // last read in step s - 1, is free again.
    const int my_dma = 4 + (wave < pieces_x ? 1 : 0) + (wave + 8 < pieces_x ? 1 : 0) + (wave + 16 < pieces_x ? 1 : 0);
    auto wait_keep_one_step = [&]() {
      switch (my_dma) {
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
      }
    };
    // the k loop for a compile-time unit count (a run-time `g < G` inside the unrolled multiply loop is a
    // branch per matrix instruction: the fragment reads then wait out their LDS latency one by one)
    auto kloop = [&](auto gc) __attribute__((always_inline)) {
      constexpr int GG = decltype(gc)::value;
      dma(0, 0);
      if (nk > 1) dma(1, 1);
      for (int s = 0; s < nk; ++s) {
        const int buf = s % kTsStages;
        if (s + 1 < nk) wait_keep_one_step();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (s + 2 < nk) dma(s + 2, (s + 2) % kTsStages);
        const char *Wb = smem + buf * kTsStage;
        const char *Xb = Wb + kTsW;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const unsigned c = 2u * ks + hi;
          const f16x8 a = *reinterpret_cast<const f16x8 *>(Wb + fa * 128 + ((c ^ swz8(fa)) << 4));
          f16x8 b[GG];
#pragma unroll
          for (int g = 0; g < GG; ++g) {
            const unsigned xr = (unsigned)(g * 32 + (lane & 31));
            b[g] = *reinterpret_cast<const f16x8 *>(Xb + xr * 128 + ((c ^ swz8(xr)) << 4));
          }
#pragma unroll
          for (int g = 0; g < GG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b[g], acc[g], 0, 0, 0);
        }
      }
    };
    switch (G) {
      case 1: kloop(std::integral_constant<int, 1>{}); break;
      case 2: kloop(std::integral_constant<int, 2>{}); break;
      case 3: kloop(std::integral_constant<int, 3>{}); break;
      case 4: kloop(std::integral_constant<int, 4>{}); break;
      default: kloop(std::integral_constant<int, 5>{}); break;
    }
    __builtin_amdgcn_s_barrier();   // every wave is done with the stages: the epilogue reuses them
    // ---- epilogue through LDS (fp32), two halves of 128 columns: waves 0..3, then waves 4..7
    const int rows = min(G * 32, M - r0);
    uint4 keep[2][kTsG];          // EPI == 2: the rounded sums of this thread's (row, 8 columns), per half and row pass
    float rsum[kTsG];
    if constexpr (EPI == 2) {
#pragma unroll
      for (int i = 0; i < kTsG; ++i) rsum[i] = 0.f;
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if ((wave >> 2) == half) {
        const int cw = (wave & 3) * 32;
#pragma unroll
        for (int g = 0; g < kTsG; ++g) {
          if (g < G) {
            char *rowp = smem + (g * 32 + (lane & 31)) * kTsEpiStride;
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
              float4 v = make_float4(acc[g][4 * rq] + bcol[4 * rq], acc[g][4 * rq + 1] + bcol[4 * rq + 1],
                                     acc[g][4 * rq + 2] + bcol[4 * rq + 2], acc[g][4 * rq + 3] + bcol[4 * rq + 3]);
              *reinterpret_cast<float4 *>(rowp + (cw + 8 * rq + 4 * (int)hi) * 4) = v;
            }
          }
        }
      }
      __builtin_amdgcn_s_barrier();
      // thread -> (row, 8 columns): 16 chunks per row of 128 columns, 32 rows per pass
      auto row_pass = [&](int r, auto itc) __attribute__((always_inline)) {
        constexpr int it = decltype(itc)::value;
        (void)it;
        const int c8 = tid & 15;
        const float4 lo = *reinterpret_cast<const float4 *>(smem + r * kTsEpiStride + c8 * 32);
        const float4 hi4 = *reinterpret_cast<const float4 *>(smem + r * kTsEpiStride + c8 * 32 + 16);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi4.x, hi4.y, hi4.z, hi4.w};
        const int col = n0 + half * 128 + c8 * 8;
        const size_t m = (size_t)(r0 + r);
        if constexpr (EPI == 2) {
          if (res) {
            const uint4 q = *reinterpret_cast<const uint4 *>(res + m * N + col);
            v[0] += h2f_lo(q.x); v[1] += h2f_hi(q.x); v[2] += h2f_lo(q.y); v[3] += h2f_hi(q.y);
            v[4] += h2f_lo(q.z); v[5] += h2f_hi(q.z); v[6] += h2f_lo(q.w); v[7] += h2f_hi(q.w);
          }
          uint4 o;
          o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
          keep[half][it] = o;
          rsum[it] += (h2f_lo(o.x) + h2f_hi(o.x)) + (h2f_lo(o.y) + h2f_hi(o.y)) + (h2f_lo(o.z) + h2f_hi(o.z)) +
                      (h2f_lo(o.w) + h2f_hi(o.w));
        } else if constexpr (EPI == 0) {
          if (res) {
            const uint4 q = *reinterpret_cast<const uint4 *>(res + m * N + col);
            v[0] += h2f_lo(q.x); v[1] += h2f_hi(q.x); v[2] += h2f_lo(q.y); v[3] += h2f_hi(q.y);
            v[4] += h2f_lo(q.z); v[5] += h2f_hi(q.z); v[6] += h2f_lo(q.w); v[7] += h2f_hi(q.w);
          }
          if (relu) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
          }
          uint4 o;
          o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
          *reinterpret_cast<uint4 *>(out + m * N + col) = o;
        } else {
          // row m = pixel `s` of camera `cam`; column chunk -> (head, channels 8 q .. 8 q + 7)
          const int cam = (int)(m / (size_t)pk.nk), s = (int)(m - (size_t)cam * pk.nk);
          const int head = col >> 5, q8 = (col & 31) >> 3;
          int l = 0;
#pragma unroll
          for (int k = 1; k < kHm3MaxLevels; ++k)
            if (k < pk.t.L && s >= pk.t.src0[k]) l = k;
          const int rel = s - pk.t.src0[l];
          const int y = rel / pk.t.W[l], xx = rel - y * pk.t.W[l];
          const int wp = pk.t.W[l] + 1;
          const int f = pk.t.ent0[l] + (y + 1) * wp + xx;        // padded entry of this pixel
          const size_t plane = (size_t)cam * pk.heads + head;
          const unsigned h0 = pack_h2(v[0], v[1]), h1 = pack_h2(v[2], v[3]), h2 = pack_h2(v[4], v[5]), h3 = pack_h2(v[6], v[7]);
          if (l >= pk.t.ls) {   // staged level: row-major 64 B per pixel
            *reinterpret_cast<uint4 *>(pk.sset + (plane * pk.t.s_entries + f) * kLdsPixBytes + q8 * 16) =
                make_uint4(h0, h1, h2, h3);
          } else {
            // big level: entry f = (this pixel, right neighbour), entry f - 1 = (left neighbour, this pixel);
            // this thread writes the halves that hold ITS pixel: the .lo lanes of entry f and the .hi lanes
            // of entry f - 1 (2-byte lanes of 4-byte words: two 16-byte read-modify-free stores are not
            // possible, so the neighbour's values come from LDS)
            float nb[8];
            const bool has_r = xx + 1 < pk.t.W[l] && r + 1 < rows;
            const bool own_r = xx + 1 < pk.t.W[l];
            if (has_r) {
              const float4 a4 = *reinterpret_cast<const float4 *>(smem + (r + 1) * kTsEpiStride + c8 * 32);
              const float4 b4 = *reinterpret_cast<const float4 *>(smem + (r + 1) * kTsEpiStride + c8 * 32 + 16);
              nb[0] = a4.x; nb[1] = a4.y; nb[2] = a4.z; nb[3] = a4.w; nb[4] = b4.x; nb[5] = b4.y; nb[6] = b4.z; nb[7] = b4.w;
            } else {
#pragma unroll
              for (int k = 0; k < 8; ++k) nb[k] = 0.f;
            }
            char *e = pk.gset + (plane * pk.t.g_entries + f) * kEntBytes + q8 * 32;
            if (has_r || !own_r) {   // the whole entry is known here: (mine, right) or (mine, pad)
              uint4 o0, o1;
              o0.x = pack_h2(v[0], nb[0]); o0.y = pack_h2(v[1], nb[1]); o0.z = pack_h2(v[2], nb[2]); o0.w = pack_h2(v[3], nb[3]);
              o1.x = pack_h2(v[4], nb[4]); o1.y = pack_h2(v[5], nb[5]); o1.z = pack_h2(v[6], nb[6]); o1.w = pack_h2(v[7], nb[7]);
              *reinterpret_cast<uint4 *>(e) = o0;
              *reinterpret_cast<uint4 *>(e + 16) = o1;
            } else {                 // right neighbour lives in the next tile: only my halves (2-byte stores)
              unsigned short *e16 = reinterpret_cast<unsigned short *>(e);
              const unsigned hv[4] = {h0, h1, h2, h3};
#pragma unroll
              for (int k = 0; k < 4; ++k) { e16[4 * k] = (unsigned short)(hv[k] & 0xffffu); e16[4 * k + 2] = (unsigned short)(hv[k] >> 16); }
            }
            if (xx == 0) {           // entry f - 1 is the pad before the row: (0, mine)
              uint4 o0, o1;
              o0.x = h0 << 16; o0.y = h0 & 0xffff0000u; o0.z = h1 << 16; o0.w = h1 & 0xffff0000u;
              o1.x = h2 << 16; o1.y = h2 & 0xffff0000u; o1.z = h3 << 16; o1.w = h3 & 0xffff0000u;
              *reinterpret_cast<uint4 *>(e - kEntBytes) = o0;
              *reinterpret_cast<uint4 *>(e - kEntBytes + 16) = o1;
            } else if (r == 0) {     // left neighbour lives in the previous tile: my halves of entry f - 1
              unsigned short *e16 = reinterpret_cast<unsigned short *>(e - kEntBytes);
              const unsigned hv[4] = {h0, h1, h2, h3};
#pragma unroll
              for (int k = 0; k < 4; ++k) { e16[4 * k + 1] = (unsigned short)(hv[k] & 0xffffu); e16[4 * k + 3] = (unsigned short)(hv[k] >> 16); }
            }
          }
        }
      };
      if constexpr (EPI == 2) {   // compile-time pass index: the kept values live in registers
        const int rb = tid >> 4;
        if (rb < rows) row_pass(rb, std::integral_constant<int, 0>{});
        if (rb + 32 < rows) row_pass(rb + 32, std::integral_constant<int, 1>{});
        if (rb + 64 < rows) row_pass(rb + 64, std::integral_constant<int, 2>{});
        if (rb + 96 < rows) row_pass(rb + 96, std::integral_constant<int, 3>{});
        if (rb + 128 < rows) row_pass(rb + 128, std::integral_constant<int, 4>{});
      } else {
        for (int r = tid >> 4; r < rows; r += kTsThreads / 16) row_pass(r, std::integral_constant<int, 0>{});
      }
      __builtin_amdgcn_s_barrier();
    }
    if constexpr (EPI == 2) {
      const int c8 = tid & 15;
      const __half *gam = reinterpret_cast<const __half *>(pk.gset), *bet = reinterpret_cast<const __half *>(pk.sset);
      int it = 0;
#pragma unroll
      for (int r = tid >> 4; r < kTsG * 32; r += kTsThreads / 16, ++it) {
        if (r >= rows) break;
        const float mean = row16_sum(rsum[it]) * (1.f / 256.f);
        float f[16];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint4 o = keep[h][it];
          f[8 * h + 0] = h2f_lo(o.x) - mean; f[8 * h + 1] = h2f_hi(o.x) - mean;
          f[8 * h + 2] = h2f_lo(o.y) - mean; f[8 * h + 3] = h2f_hi(o.y) - mean;
          f[8 * h + 4] = h2f_lo(o.z) - mean; f[8 * h + 5] = h2f_hi(o.z) - mean;
          f[8 * h + 6] = h2f_lo(o.w) - mean; f[8 * h + 7] = h2f_hi(o.w) - mean;
        }
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) sq = fmaf(f[k], f[k], sq);
        const float rstd = rsqrtf(row16_sum(sq) * (1.f / 256.f) + pk.eps);
        const size_t m = (size_t)(r0 + r);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int col = h * 128 + c8 * 8;
          const uint4 g4 = *reinterpret_cast<const uint4 *>(gam + col), b4 = *reinterpret_cast<const uint4 *>(bet + col);
          const float gg[8] = {h2f_lo(g4.x), h2f_hi(g4.x), h2f_lo(g4.y), h2f_hi(g4.y),
                               h2f_lo(g4.z), h2f_hi(g4.z), h2f_lo(g4.w), h2f_hi(g4.w)};
          const float bb[8] = {h2f_lo(b4.x), h2f_hi(b4.x), h2f_lo(b4.y), h2f_hi(b4.y),
                               h2f_lo(b4.z), h2f_hi(b4.z), h2f_lo(b4.w), h2f_hi(b4.w)};
          float y[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) y[k] = fmaf(f[8 * h + k] * rstd, gg[k], bb[k]);
          uint4 o;
          o.x = pack_h2(y[0], y[1]); o.y = pack_h2(y[2], y[3]); o.z = pack_h2(y[4], y[5]); o.w = pack_h2(y[6], y[7]);
          *reinterpret_cast<uint4 *>(out + m * N + col) = o;
        }
      }
    }
  }
}

// EPI 1: the entries of the padded sets that hold no pixel at all -- per plane the leading / trailing entry,
// the pad rows above and below each level, the pad pixel after each row of a staged level, and the pad
// after the LAST row of a big level (the pad after any other row of a big level is the entry
// (0, first pixel of the next row): the GEMM epilogue writes it).  grid (x, planes).
__global__ __launch_bounds__(256) void tsgemm_pad_zero_kernel(TsPacked pk, int planes) {
  const Hm3Tab &t = pk.t;
  const int plane = blockIdx.y;
  if (plane >= planes) return;
  for (int l = 0; l < t.L; ++l) {
    const bool staged = l >= t.ls;
    const int wp = t.W[l] + 1, H = t.H[l];
    const int ebytes = staged ? kLdsPixBytes : kEntBytes;
    const int chunks = ebytes / 16;
    char *base = (staged ? pk.sset + (size_t)plane * t.s_entries * kLdsPixBytes
                         : pk.gset + (size_t)plane * t.g_entries * kEntBytes);
    // pad entries of this level: row 0 (wp entries, but for a big level the LAST one pairs with row 1's
    // first pixel and is written by the epilogue), row H + 1 (wp), and column W of rows 1..H (big level:
    // rows 1..H-1 pair with the next row's first pixel -> epilogue; row H's pad -> zero here)
    const int total = 2 * wp + H;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total * chunks; i += gridDim.x * 256) {
      const int e = i / chunks, c = i - e * chunks;
      int yp, xx;
      if (e < wp) { yp = 0; xx = e; }
      else if (e < 2 * wp) { yp = H + 1; xx = e - wp; }
      else { yp = e - 2 * wp + 1; xx = t.W[l]; }
      if (!staged && xx == t.W[l] && yp < H) continue;   // (0, first pixel of row yp + 1): the epilogue's
      *reinterpret_cast<uint4 *>(base + (size_t)(t.ent0[l] + yp * wp + xx) * ebytes + c * 16) = make_uint4(0, 0, 0, 0);
    }
  }
  // leading entry 0 and the trailing entry of each set
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    const int c = threadIdx.x & 7, which = threadIdx.x >> 3;
    char *g = pk.gset + (size_t)plane * t.g_entries * kEntBytes;
    *reinterpret_cast<uint4 *>(g + (which ? (size_t)(t.g_entries - 1) * kEntBytes : 0) + c * 16) = make_uint4(0, 0, 0, 0);
    if (t.s_entries && c < 4) {
      char *s = pk.sset + (size_t)plane * t.s_entries * kLdsPixBytes;
      *reinterpret_cast<uint4 *>(s + (which ? (size_t)(t.s_entries - 1) * kLdsPixBytes : 0) + c * 16) = make_uint4(0, 0, 0, 0);
    }
  }
}

// ---- the weight-stationary flavour for K <= 256 (K = 64 KS).  In tsgemm_f16_kernel every tile pulls its 256 x K weight
// slice through the CU's load path again (128 KB per 160-row tile at K = 256, next to 80 KB of rows), and load, multiply
// and store of a tile run one after another.  Here
//   * a wave keeps ITS 32 weight rows in registers for the whole launch: K / 8 fragments of 16 bytes per lane (64 VGPRs
//     at K = 256), read once from global memory with the lane -> (row, k-chunk) mapping of the LDS fragment read above;
//     no weight byte passes through LDS;
//   * LDS holds whole-K images of 64 activation rows (KS sub-images of 64 x 128 bytes, the same swizzled row image) in
//     a ring of three, plus the fp32 staging of one 128-column half: the rows of tile t + 2 are requested before tile
//     t is multiplied, and a wave waits for its pieces of tile t + 1 just before the first store of tile t, so row
//     loads are in flight during the multiply AND the stores.  Every wave issues exactly KS DMA instructions per tile
//     (pieces outside the block's rows get an out-of-range offset: the buffer descriptor answers zeros without an
//     access), so the waits are counted: what is left outstanding is the newest request, the previous tile's stores
//     and the residual rows of the next tile (read one tile ahead);
//   * N > 256: one block per (row partition, 256-column chunk), all co-resident; the chunks of a partition sit on the
//     same XCD (block b runs on XCD b % 8) and walk the same rows at the same time, so the re-read comes from L2.
// Summation order: k ascending in every block, the same matrix instruction, operand layout, fp32 epilogue and single
// rounding as above -- an output row depends on its own operands only, not on the block index, M or the CU count.
// GRP (EPI 0, bevops_tsgemm_f16_grouped): column chunk g is a dense [M, 256] matrix of its own at out + g * pk.gstride --
// G layers that read the same rows as ONE launch; only the store address differs from the N = G * 256 launch.
constexpr int kWsG = 2;                          // row units per tile (the staging writes below are written for 2)
constexpr int kWsRows = kWsG * 32;
constexpr int kWsBufs = 3;
constexpr int kWsStep = kWsRows * 128;           // one 64-k sub-image of a tile (8 KB)
constexpr int kWsEpi = kWsRows * kTsEpiStride;   // fp32 staging of a 128-column half (33 KB), at the start of LDS
constexpr int ws_lds(int ks) { return kWsEpi + kWsBufs * ks * kWsStep; }   // 129 KB at K = 256

// KS2 > 0 (EPI 0, bevops_gemm2_f16): the last KS2 of a tile's KS sub-images come from a second activation tensor --
// channels-last pixels of 64 KS2 channels, output row m at pixel (b, s yo, s xo) -- and x holds rows of 64 (KS - KS2)
// values.  A wave still issues exactly KS DMA instructions per tile, in the same order, each through the descriptor of its
// source: the counted waits, the ring and the multiply are the plain kernel's, and so are the bits on the materialised
// [x | rows of x2] (k ascending: source 1, then source 2).
struct TsSrc2 {
  const __half *x2;
  unsigned bytes;                          // size of the second tensor
  int hin, win, hout, wout, stride;
};

template <int EPI, int KS, bool GRP, int KS2 = 0>
__device__ __forceinline__ void tsgemm_ws_body(const __half *__restrict__ x, const __half *__restrict__ w,
                                               const __half *__restrict__ bias, const __half *__restrict__ res,
                                               __half *__restrict__ out, int M, int N, int relu, int units_total, int parts,
                                               int chunks, const TsPacked &pk, const TsSrc2 &src2 = TsSrc2{}) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int K = KS * 64;
  constexpr int KS1 = KS - KS2, K1 = KS1 * 64, K2 = KS2 * 64;   // (KS2 == 0: KS1 == KS, K1 == K)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // block -> (row partition, column chunk); the chunks of a partition on one XCD when the grid allows it
  int part, chunk;
  if (gridDim.x % (8u * (unsigned)chunks) == 0) {
    const int i = (int)(blockIdx.x >> 3);
    chunk = i % chunks;
    part = (i / chunks) * 8 + (int)(blockIdx.x & 7);
  } else {
    chunk = (int)blockIdx.x % chunks;
    part = (int)blockIdx.x / chunks;
  }
  const int n0 = chunk * kTsBN;
  const int per = units_total / parts, extra = units_total % parts;
  const int u_begin = part * per + min(part, extra);
  const int u_end = u_begin + per + (part < extra ? 1 : 0);
  if (u_begin >= u_end) return;
  const int ntiles = (u_end - u_begin + kWsG - 1) / kWsG;

  const __amdgpu_buffer_rsrc_t rs_x =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__half *>(x), 0, (unsigned)((size_t)M * K1 * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x2 =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__half *>(src2.x2), 0, KS2 > 0 ? src2.bytes : 0u, 0x00020000);
  const unsigned hi = (unsigned)(lane >> 5);
  const unsigned fa = (unsigned)(wave * 32 + (lane & 31));   // weight row of this lane's fragments
  // the wave's weight rows: fragment 4 kstep + ks holds k = 64 kstep + 16 ks + 8 hi .. + 7 of row n0 + fa
  f16x8 wr[KS * 4];
  {
    const __half *wrow = w + (size_t)(n0 + (int)fa) * K + hi * 8;
#pragma unroll
    for (int kk = 0; kk < KS * 4; ++kk) wr[kk] = *reinterpret_cast<const f16x8 *>(wrow + kk * 16);
  }
  // column constants of this lane: acc[g][4 rq + e] is column wave * 32 + 8 rq + 4 hi + e
  float bcol[16];
  if (bias) {   // four 8-byte loads in flight together
    uint2 bq[4];
#pragma unroll
    for (int rq = 0; rq < 4; ++rq)
      bq[rq] = *reinterpret_cast<const uint2 *>(bias + n0 + wave * 32 + 8 * rq + 4 * (int)hi);
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      bcol[4 * rq] = h2f_lo(bq[rq].x); bcol[4 * rq + 1] = h2f_hi(bq[rq].x);
      bcol[4 * rq + 2] = h2f_lo(bq[rq].y); bcol[4 * rq + 3] = h2f_hi(bq[rq].y);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) bcol[i] = 0.f;
  }

  // DMA role: piece `wave` of a tile = its rows 8 wave .. 8 wave + 7, lane -> (row in piece, 16-byte chunk), the
  // swizzle on the source chunk; KS instructions per wave and tile, always
  const unsigned trow = (unsigned)(wave * 8 + (lane >> 3));
  const unsigned tchunk = (((unsigned)(lane & 7)) ^ swz8(trow)) << 4;
  auto dma = [&](int t, int buf) {
    const int row = (u_begin + t * kWsG) * 32 + (int)trow;
    const bool valid = t < ntiles && u_begin + t * kWsG + (wave >> 2) < u_end && row < M;
    const unsigned voff = valid ? (unsigned)((size_t)row * K1 * 2) + tchunk : 0xFFFFFF00u;
    char *d = smem + kWsEpi + buf * (KS * kWsStep) + wave * 1024;
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void_t *)(d + ks * kWsStep), 16, (int)voff, ks * 128, 0, 0);
    if constexpr (KS2 > 0) {
      unsigned voff2 = 0xFFFFFF00u;
      if (valid) {
        size_t pix = (size_t)row;            // stride 1: the rows ARE the pixels
        if (src2.stride != 1) {
          const int per = src2.hout * src2.wout;
          const int b = row / per, q = row - b * per;
          const int yo = q / src2.wout, xo = q - yo * src2.wout;
          pix = ((size_t)b * src2.hin + (size_t)(yo * src2.stride)) * src2.win + (size_t)(xo * src2.stride);
        }
        voff2 = (unsigned)(pix * K2 * 2) + tchunk;
      }
#pragma unroll
      for (int ks = 0; ks < KS2; ++ks)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x2, (lds_void_t *)(d + (KS1 + ks) * kWsStep), 16, (int)voff2, ks * 128,
                                                 0, 0);
    }
  };
  // all but the youngest tile's pieces of this wave have landed
  auto wait_keep_one_tile = [&]() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KS) : "memory"); };
  // The same wait inside the loop, where more than the youngest request is younger than the pieces waited for: the
  // stores of the previous tile and the residual loads of the next one.  The counter retires in order: leaving
  // exactly those outstanding waits for the pieces and for nothing issued after them (in particular not for the write
  // acknowledgements of the previous tile).  `younger` is a LOWER bound of their number (waiting for more is safe, for
  // less is not), wave-uniform.
  auto wait_for_next_tile = [&](int younger) {
    switch (younger) {
      case 0: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KS) : "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KS + 2) : "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KS + 4) : "memory"); break;
      case 6: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KS + 6) : "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KS + 8) : "memory"); break;   // 8, the most there is
    }
  };
  const int rb = tid >> 4, c8 = tid & 15;   // epilogue role: rows rb, rb + 32 of the tile, 8 columns of a half
  // residual rows of tile t (rows past the end are clamped, never stored): read one tile AHEAD, so that waiting for
  // them never waits for the stores of the tile before
  uint4 rq[2][kWsG];
  auto load_res = [&](int t, uint4(&q)[2][kWsG]) {
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int i = 0; i < kWsG; ++i) {
        const size_t m = (size_t)min((u_begin + t * kWsG) * 32 + rb + 32 * i, M - 1);
        q[half][i] = *reinterpret_cast<const uint4 *>(res + m * N + n0 + half * 128 + c8 * 8);
      }
  };
  uint4 gb[4];   // EPI 2: the norm's parameters of this thread's columns, read once (a load inside the loop would have to
                 // be waited for, and with it every request issued before it)
  if constexpr (EPI == 2) ts_ln_params(pk, c8, gb);
  if constexpr (EPI != 1) {
    if (res) load_res(0, rq);
  }

  dma(0, 0);
  dma(1, 1);
#pragma unroll
  for (int kk = 0; kk < KS * 4; ++kk) asm volatile("" ::"v"(wr[kk]));   // the weights have arrived HERE, not in the loop
  wait_keep_one_tile();
  __builtin_amdgcn_s_barrier();

  int buf = 0;
  int stores_prev = 0;   // store instructions of this wave in the previous tile, at least
  for (int t = 0; t < ntiles; ++t) {
    const int u0 = u_begin + t * kWsG;
    const int r0 = u0 * 32;
    const int rows = min(min(kWsRows, (u_end - u0) * 32), M - r0);
    uint4 rqn[2][kWsG];
    if constexpr (EPI != 1) {
      if (res) load_res(t + 1, rqn);
    }
    {
      int b2 = buf + 2;
      if (b2 >= kWsBufs) b2 -= kWsBufs;
      dma(t + 2, b2);   // that buffer was multiplied in tile t - 1, before its epilogue's barriers
    }
    f32x16 acc[kWsG];
#pragma unroll
    for (int g = 0; g < kWsG; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
    const char *Xt = smem + kWsEpi + buf * (KS * kWsStep);
#pragma unroll
    for (int kk = 0; kk < KS * 4; ++kk) {
      const unsigned c = 2u * (kk & 3) + hi;
      f16x8 b[kWsG];
#pragma unroll
      for (int g = 0; g < kWsG; ++g) {
        const unsigned xr = (unsigned)(g * 32 + (lane & 31));
        b[g] = *reinterpret_cast<const f16x8 *>(Xt + (kk >> 2) * kWsStep + xr * 128 + ((c ^ swz8(xr)) << 4));
      }
#pragma unroll
      for (int g = 0; g < kWsG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[kk], b[g], acc[g], 0, 0, 0);
    }
    // ---- epilogue through LDS (fp32), two halves of 128 columns: waves 0..3, then waves 4..7
    uint4 keep[2][kWsG];
    float rsum[kWsG];
    if constexpr (EPI == 2) {
#pragma unroll
      for (int i = 0; i < kWsG; ++i) rsum[i] = 0.f;
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if ((wave >> 2) == half) {
        const int cw = (wave & 3) * 32;
#pragma unroll
        for (int g = 0; g < kWsG; ++g) {
          const unsigned rowa = lds_addr(smem + (lane & 31) * kTsEpiStride + (cw + 4 * (int)hi) * 4);
          auto put = [&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value;
            const f32x4 v = {acc[g][4 * q] + bcol[4 * q], acc[g][4 * q + 1] + bcol[4 * q + 1],
                             acc[g][4 * q + 2] + bcol[4 * q + 2], acc[g][4 * q + 3] + bcol[4 * q + 3]};
            if (g == 0) lds_write16<q * 32>(rowa, v);
            else lds_write16<32 * kTsEpiStride + q * 32>(rowa, v);
          };
          put(std::integral_constant<int, 0>{}); put(std::integral_constant<int, 1>{});
          put(std::integral_constant<int, 2>{}); put(std::integral_constant<int, 3>{});
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      // before the first store of this tile: my pieces of tile t + 1 are in LDS (the barrier that ends the half shows
      // them to everybody), the request for tile t + 2 stays in flight behind the stores
      if (half == 0) wait_for_next_tile(stores_prev + ((EPI != 1 && res) ? 4 : 0));
#pragma unroll
      for (int i = 0; i < kWsG; ++i) {
        const int r = rb + 32 * i;
        if (r < rows) {
          float v[8];
          lds_read32(lds_addr(smem + r * kTsEpiStride + c8 * 32), v);
          const int col = n0 + half * 128 + c8 * 8;
          const size_t m = (size_t)(r0 + r);
          if constexpr (EPI == 1) {
            ts_store_planes(v, pk, m, col, r, rows, c8, smem);
          } else {
            if (res) ts_add_res(v, rq[half][i]);
            if constexpr (EPI == 2) {
              const uint4 o = ts_pack8(v);
              keep[half][i] = o;
              rsum[i] += ts_sum8(o);
            } else {
              if (relu) {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
              }
              if constexpr (GRP)
                *reinterpret_cast<uint4 *>(out + (size_t)chunk * (size_t)pk.gstride + m * kTsBN + (col - n0)) = ts_pack8(v);
              else
                *reinterpret_cast<uint4 *>(out + m * N + col) = ts_pack8(v);
            }
          }
        }
      }
      __builtin_amdgcn_s_barrier();
    }
    if constexpr (EPI == 2) {
#pragma unroll
      for (int i = 0; i < kWsG; ++i) {
        const int r = rb + 32 * i;
        if (r < rows) ts_ln_row(keep[0][i], keep[1][i], rsum[i], pk.eps, gb, out + (size_t)(r0 + r) * N, c8);
      }
    }
    if constexpr (EPI != 1) {
      if (res) {
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int i = 0; i < kWsG; ++i) rq[half][i] = rqn[half][i];
      }
    }
    // every (half, row pass) with a live row in this wave stored at least once (EPI 2: two stores per live row)
    stores_prev = __builtin_amdgcn_readfirstlane(2 * ((wave * 4 < rows ? 1 : 0) + (wave * 4 + 32 < rows ? 1 : 0)));
    if (++buf == kWsBufs) buf = 0;
  }
}

template <int EPI, int KS>
__global__ __launch_bounds__(kTsThreads) void tsgemm_ws_kernel(const __half *__restrict__ x, const __half *__restrict__ w,
                                                               const __half *__restrict__ bias,
                                                               const __half *__restrict__ res, __half *__restrict__ out,
                                                               int M, int N, int relu, int units_total, int parts,
                                                               int chunks, TsPacked pk) {
  tsgemm_ws_body<EPI, KS, false>(x, w, bias, res, out, M, N, relu, units_total, parts, chunks, pk);
}

template <int KS>
__global__ __launch_bounds__(kTsThreads) void tsgemm_ws_grouped_kernel(const __half *__restrict__ x, const __half *__restrict__ w,
                                                                       const __half *__restrict__ bias, __half *__restrict__ out,
                                                                       int M, int N, int units_total, int parts, int chunks,
                                                                       TsPacked pk) {
  tsgemm_ws_body<0, KS, true>(x, w, bias, nullptr, out, M, N, 0, units_total, parts, chunks, pk);
}

template <int KS, int KS2>
__global__ __launch_bounds__(kTsThreads) void tsgemm_ws2_kernel(const __half *__restrict__ x, const __half *__restrict__ w,
                                                                const __half *__restrict__ bias, __half *__restrict__ out,
                                                                int M, int N, int relu, int units_total, int parts, int chunks,
                                                                TsSrc2 src2) {
  tsgemm_ws_body<0, KS, false, KS2>(x, w, bias, nullptr, out, M, N, relu, units_total, parts, chunks, TsPacked{}, src2);
}

// ---- the int8 activation chain's flavour (quantization.Int8ChainBackbone: the 1x1 convolutions of ResNet stages 3 / 4):
//     out = requant( act( (sum_k a[m, k] w[n, k]) * s_a * s_w[n] + bias[n] (+ identity[m, n]) ) )
// a [M, K], w [N, K] int8 row-major, int32 sums (exact), fp32 bias, identity rows int8 (with their own scale) or fp16,
// output int8 (requantised with the consumer's scale) or fp16.  The same persistent skeleton as tsgemm_f16_kernel --
// one block per CU, tiles of up to 160 rows x 256 columns, both operands global -> LDS by DMA in three stages, XOR
// swizzled 128-byte rows -- with 128 k-values per step instead of 64 (the LDS images, the DMA roles and the 16-byte
// fragment reads are byte-for-byte the fp16 kernel's: a v_mfma_i32_32x32x32_i8 operand is 16 consecutive bytes of k,
// lanes 32..63 the second 16 of a 32-value sub-step).  Measured (profiles/r04/tsgemm_s8_ab.jsonl): faster than the
// tiled int8 GEMM on the 256-column layers with K = 1 024 (stage-3 conv1: 21.5 vs 24.6 us), slower for N > 256 (every
// 256-column chunk re-reads the activation rows): functions/int8_chain.py picks it for the former only.
// A second flavour (EPI == 2, bevops_tsgemm_s8_ln) puts the LayerNorm that ends every encoder block of the INT8 engine in
// the epilogue: see the comment at the kernel.
typedef int i32x4v __attribute__((ext_vector_type(4)));
typedef int i32x16v __attribute__((ext_vector_type(16)));

struct TsS8Args {
  const int8_t *a, *w;
  const float *bias, *wscale;   // fp32 [N] or null
  const void *res;              // int8 or fp16 [M, N] or null
  void *out;                    // int8 or fp16 [M, N]
  float s_aw, s_res, inv_s_out;
  int M, N, K, relu, units_total, res_i8, out_i8;
};

struct TsS8LnArgs : TsS8Args {   // EPI == 2: the LayerNorm's weight and bias (pk.gset / pk.sset, fp16 [256]) and eps
  TsPacked pk;
};

// EPI 0: the epilogue above.  EPI 2 (N == 256, one column chunk, fp16 out, no ReLU): the block's LayerNorm in the
// epilogue, out = LayerNorm_256(fp16(acc * s_a * s_w + bias (+ identity))) * ln_weight + ln_bias, with the row layout of
// tsgemm_f16_kernel<2>: a thread owns the same 8 columns of the same rows in both 128-column halves, keeps the rounded
// sums of half 0 in registers (5 row passes x 16 bytes, nothing is stored in half 0) and normalises the row in half 1
// (ts_ln_row: fp32 mean and centred squares over the 16 lanes of a DPP row, one rounding) -- from exactly the binary16
// values the pair bevops_tsgemm_s8 (fp16 out) -> bevops_layer_norm would have read back.  The arguments of the two
// flavours are different types, so the EPI 0 instantiation keeps its argument segment and its code.
template <int EPI>
__global__ __launch_bounds__(kTsThreads) void tsgemm_s8_kernel(
    const std::conditional_t<EPI == 2, TsS8LnArgs, TsS8Args> p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = p.M, N = p.N, K = p.K;
  const int n0 = blockIdx.y * kTsBN;
  const int nb = gridDim.x, bi = blockIdx.x;
  const int per = p.units_total / nb, extra = p.units_total % nb;
  const int u_begin = bi * per + min(bi, extra);
  const int u_end = u_begin + per + (bi < extra ? 1 : 0);
  if (u_begin >= u_end) return;
  const __amdgpu_buffer_rsrc_t rs_x =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(p.a), 0, (unsigned)((size_t)M * K), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(p.w), 0, (unsigned)((size_t)N * K), 0x00020000);
  const unsigned prow = (unsigned)(lane >> 3), pchunk = (unsigned)(lane & 7);
  unsigned w_off[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned row = (unsigned)((wave * 4 + j) * 8) + prow;
    w_off[j] = (unsigned)((size_t)(n0 + row) * K) + ((pchunk ^ swz8(row)) << 4);
  }
  const unsigned hi = (unsigned)(lane >> 5);
  const unsigned fa = (unsigned)(wave * 32 + (lane & 31));
  const int nk = K / 128;
  // column constants of this lane: acc[g][4 rq + e] is column wave * 32 + 8 rq + 4 hi + e
  float scol[16], bcol[16];
#pragma unroll
  for (int rq = 0; rq < 4; ++rq)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = n0 + wave * 32 + 8 * rq + 4 * (int)hi + e;
      scol[4 * rq + e] = p.wscale ? p.s_aw * p.wscale[col] : p.s_aw;
      bcol[4 * rq + e] = p.bias ? p.bias[col] : 0.f;
    }
  // EPI 2: the norm's weight and bias (fp16 [256] each) are read from global memory once, before the first tile, into the
  // 1 KB of LDS behind the three stages; a thread fetches its columns' 64 bytes from there in half 1, where the
  // accumulators are dead (held in registers for the whole launch they cost 16 VGPRs at the kernel's peak: it spilled)
  TsPacked ln_lds;
  if constexpr (EPI == 2) {
    ln_lds.gset = smem + kTsLds;
    ln_lds.sset = smem + kTsLds + kTsBN * 2;
    if (tid < 64) {
      const char *src = (tid < 32 ? p.pk.gset : p.pk.sset) + (tid & 31) * 16;
      *reinterpret_cast<uint4 *>(smem + kTsLds + tid * 16) = *reinterpret_cast<const uint4 *>(src);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // written before this wave's first barrier (in the k loop)
    }
  }
  for (int u0 = u_begin; u0 < u_end; u0 += kTsG) {
    const int G = min(kTsG, u_end - u0);
    const int r0 = u0 * 32;
    const int pieces_x = G * 4;
    unsigned x_off[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned row = (unsigned)((wave + 8 * j) * 8) + prow;
      x_off[j] = (unsigned)((size_t)(r0 + row) * K) + ((pchunk ^ swz8(row)) << 4);
    }
    const int k_rot = bi % nk;   // (integer sums: the order of the k-slices does not change the result)
    auto dma = [&](int step, int buf) {
      char *wd = smem + buf * kTsStage + wave * 4096;
      int kstep = step + k_rot;
      if (kstep >= nk) kstep -= nk;
      const int soff = kstep * 128;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void_t *)(wd + j * 1024), 16, (int)w_off[j], soff, 0, 0);
      char *xd = smem + buf * kTsStage + kTsW;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (wave + 8 * j < pieces_x)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void_t *)(xd + (wave + 8 * j) * 1024), 16,
                                                   (int)x_off[j], soff, 0, 0);
    };
    i32x16v acc[kTsG];
#pragma unroll
    for (int g = 0; g < kTsG; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][r] = 0;
    const int my_dma = 4 + (wave < pieces_x ? 1 : 0) + (wave + 8 < pieces_x ? 1 : 0) + (wave + 16 < pieces_x ? 1 : 0);
    auto wait_keep_one_step = [&]() {
      switch (my_dma) {
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
      }
    };
    auto kloop = [&](auto gc) __attribute__((always_inline)) {
      constexpr int GG = decltype(gc)::value;
      dma(0, 0);
      if (nk > 1) dma(1, 1);
      for (int s = 0; s < nk; ++s) {
        const int buf = s % kTsStages;
        if (s + 1 < nk) wait_keep_one_step();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (s + 2 < nk) dma(s + 2, (s + 2) % kTsStages);
        const char *Wb = smem + buf * kTsStage;
        const char *Xb = Wb + kTsW;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const unsigned c = 2u * ks + hi;
          const i32x4v a = *reinterpret_cast<const i32x4v *>(Wb + fa * 128 + ((c ^ swz8(fa)) << 4));
          i32x4v b[GG];
#pragma unroll
          for (int g = 0; g < GG; ++g) {
            const unsigned xr = (unsigned)(g * 32 + (lane & 31));
            b[g] = *reinterpret_cast<const i32x4v *>(Xb + xr * 128 + ((c ^ swz8(xr)) << 4));
          }
#pragma unroll
          for (int g = 0; g < GG; ++g) acc[g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[g], acc[g], 0, 0, 0);
        }
      }
    };
    switch (G) {
      case 1: kloop(std::integral_constant<int, 1>{}); break;
      case 2: kloop(std::integral_constant<int, 2>{}); break;
      case 3: kloop(std::integral_constant<int, 3>{}); break;
      case 4: kloop(std::integral_constant<int, 4>{}); break;
      default: kloop(std::integral_constant<int, 5>{}); break;
    }
    __builtin_amdgcn_s_barrier();
    // ---- epilogue through LDS (fp32: sums already scaled and shifted), two halves of 128 columns
    const int rows = min(G * 32, M - r0);
    uint4 keep[kTsG];   // EPI 2: the rounded sums of half 0 of this thread's (row, 8 columns), per row pass
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if ((wave >> 2) == half) {
        const int cw = (wave & 3) * 32;
#pragma unroll
        for (int g = 0; g < kTsG; ++g) {
          if (g < G) {
            char *rowp = smem + (g * 32 + (lane & 31)) * kTsEpiStride;
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
              float4 v = make_float4((float)acc[g][4 * rq] * scol[4 * rq] + bcol[4 * rq],
                                     (float)acc[g][4 * rq + 1] * scol[4 * rq + 1] + bcol[4 * rq + 1],
                                     (float)acc[g][4 * rq + 2] * scol[4 * rq + 2] + bcol[4 * rq + 2],
                                     (float)acc[g][4 * rq + 3] * scol[4 * rq + 3] + bcol[4 * rq + 3]);
              *reinterpret_cast<float4 *>(rowp + (cw + 8 * rq + 4 * (int)hi) * 4) = v;
            }
          }
        }
      }
      __builtin_amdgcn_s_barrier();
      if constexpr (EPI == 2) {
        // Row pass `it` of this thread is tile row (tid >> 4) + 32 it: a compile-time index with an `r < rows` guard, so
        // keep[] / rsum[] are registers, never a dynamically indexed array in scratch.  The 16 threads of a row are 16
        // consecutive lanes: the guard is uniform over the DPP row ts_ln_row reduces over.
        auto ln_pass = [&](auto itc) __attribute__((always_inline)) {
          constexpr int it = decltype(itc)::value;
          const int r = (tid >> 4) + 32 * it;
          if (r >= rows) return;
          const int c8 = tid & 15;
          const float4 lo = *reinterpret_cast<const float4 *>(smem + r * kTsEpiStride + c8 * 32);
          const float4 hi4 = *reinterpret_cast<const float4 *>(smem + r * kTsEpiStride + c8 * 32 + 16);
          float v[8] = {lo.x, lo.y, lo.z, lo.w, hi4.x, hi4.y, hi4.z, hi4.w};
          const int col = half * 128 + c8 * 8;
          const size_t m = (size_t)(r0 + r);
          if (p.res) {
            if (p.res_i8) {
              const uint2 q = *reinterpret_cast<const uint2 *>(static_cast<const int8_t *>(p.res) + m * kTsBN + col);
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                v[c] += (float)(int)(signed char)((q.x >> (8 * c)) & 0xffu) * p.s_res;
                v[4 + c] += (float)(int)(signed char)((q.y >> (8 * c)) & 0xffu) * p.s_res;
              }
            } else {
              ts_add_res(v, *reinterpret_cast<const uint4 *>(static_cast<const __half *>(p.res) + m * kTsBN + col));
            }
          }
          const uint4 o = ts_pack8(v);   // the ONE rounding of the pre-norm value, as the fp16-output path rounds it
          if (half == 0) {
            keep[it] = o;
          } else {
            uint4 gb[4];
            ts_ln_params(ln_lds, c8, gb);
            ts_ln_row(keep[it], o, ts_sum8(keep[it]) + ts_sum8(o), p.pk.eps, gb, static_cast<__half *>(p.out) + m * kTsBN, c8);
          }
        };
        ln_pass(std::integral_constant<int, 0>{}); ln_pass(std::integral_constant<int, 1>{});
        ln_pass(std::integral_constant<int, 2>{}); ln_pass(std::integral_constant<int, 3>{});
        ln_pass(std::integral_constant<int, 4>{});
        // the staging rows are read: half 1 may overwrite them, the next tile's DMA may overwrite stages 0 and 1
        __builtin_amdgcn_s_barrier();
        continue;
      }
      for (int r = tid >> 4; r < rows; r += kTsThreads / 16) {
        const int c8 = tid & 15;
        const float4 lo = *reinterpret_cast<const float4 *>(smem + r * kTsEpiStride + c8 * 32);
        const float4 hi4 = *reinterpret_cast<const float4 *>(smem + r * kTsEpiStride + c8 * 32 + 16);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi4.x, hi4.y, hi4.z, hi4.w};
        const int col = n0 + half * 128 + c8 * 8;
        const size_t m = (size_t)(r0 + r);
        if (p.res) {
          if (p.res_i8) {
            const uint2 q = *reinterpret_cast<const uint2 *>(static_cast<const int8_t *>(p.res) + m * N + col);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              v[c] += (float)(int)(signed char)((q.x >> (8 * c)) & 0xffu) * p.s_res;
              v[4 + c] += (float)(int)(signed char)((q.y >> (8 * c)) & 0xffu) * p.s_res;
            }
          } else {
            const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const __half *>(p.res) + m * N + col);
            v[0] += h2f_lo(q.x); v[1] += h2f_hi(q.x); v[2] += h2f_lo(q.y); v[3] += h2f_hi(q.y);
            v[4] += h2f_lo(q.z); v[5] += h2f_hi(q.z); v[6] += h2f_lo(q.w); v[7] += h2f_hi(q.w);
          }
        }
        if (p.relu) {
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
        }
        if (p.out_i8) {
          unsigned pk[2] = {0, 0};
#pragma unroll
          for (int c = 0; c < 8; ++c)
            pk[c >> 2] |= ((unsigned)(int)fminf(fmaxf(rintf(v[c] * p.inv_s_out), -127.f), 127.f) & 0xffu) << (8 * (c & 3));
          *reinterpret_cast<uint2 *>(static_cast<int8_t *>(p.out) + m * N + col) = make_uint2(pk[0], pk[1]);
        } else {
          uint4 o;
          o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
          *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + m * N + col) = o;
        }
      }
      __builtin_amdgcn_s_barrier();
    }
  }
}

inline int ts_grid_x(int units, int chunks_n) {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    hipDeviceProp_t p;
    static int cached[16] = {0};
    if (cached[dev & 15] == 0 && hipGetDeviceProperties(&p, dev) == hipSuccess) cached[dev & 15] = p.multiProcessorCount;
    if (cached[dev & 15] > 0) cus = cached[dev & 15];
  }
  (void)chunks_n;
  return units < cus ? units : cus;
}

// bevops_tsgemm_set_variant: 0 = the weight-stationary kernel inside its domain, 1 = tsgemm_f16_kernel everywhere (A/B
// partner); BEVOPS_TSGEMM_WS=0 in the environment at library load is variant 1 for every thread.
thread_local int g_ts_variant = 0;
const bool g_ts_env_old = [] {
  const char *e = getenv("BEVOPS_TSGEMM_WS");
  return e && e[0] == '0' && e[1] == 0;
}();

// the one predicate of the three fp16 entries (they switch together: the planes of bevops_value_proj_packed are tied
// byte for byte to bevops_tsgemm_f16, and so is the LayerNorm epilogue)
inline bool ts_use_ws(int k) { return k <= 256 && g_ts_variant != 1 && !g_ts_env_old; }

template <int EPI, int KS, bool GRP = false>
int ws_launch_ks(const GemmCall &c, const TsPacked &pk) {
  if constexpr (GRP) {
    if (!ensure_dynamic_lds<tsgemm_ws_grouped_kernel<KS>>(ws_lds(KS))) return BEVOPS_FAILURE;
  } else {
    if (!ensure_dynamic_lds<tsgemm_ws_kernel<EPI, KS>>(ws_lds(KS))) return BEVOPS_FAILURE;
  }
  const int units = (int)((c.m + 31) / 32), chunks = c.n / kTsBN;
  const int cus = ts_grid_x(1 << 30, chunks);
  int parts = cus / chunks;
  if (parts < 1) parts = 1;
  // grouped: a multiple of 8 partitions, so that the kernel's block -> (partition, chunk) map can put the chunks of a
  // partition on one XCD for any G (256 CUs / 6 chunks = 42 partitions would scatter them: 40 do not)
  if (GRP && parts >= 8) parts -= parts % 8;
  if (parts > units) parts = units;
  if constexpr (GRP)
    hipLaunchKernelGGL((tsgemm_ws_grouped_kernel<KS>), dim3((unsigned)(parts * chunks)), dim3(kTsThreads), ws_lds(KS), c.st,
                       (const __half *)c.x, (const __half *)c.w, (const __half *)c.bias, (__half *)c.out, (int)c.m, c.n,
                       units, parts, chunks, pk);
  else
    hipLaunchKernelGGL((tsgemm_ws_kernel<EPI, KS>), dim3((unsigned)(parts * chunks)), dim3(kTsThreads), ws_lds(KS), c.st,
                       (const __half *)c.x, (const __half *)c.w, (const __half *)c.bias, (const __half *)c.res,
                       (__half *)c.out, (int)c.m, c.n, c.relu, units, parts, chunks, pk);
  return launch_status();
}

// The launch of the three fp16 entries after their checks: the weight-stationary kernel inside its domain (K <= 256),
// else tsgemm_f16_kernel<EPI>, one persistent block per CU and 256-column chunk.
template <int EPI>
int ts_launch_f16(const GemmCall &c, const TsPacked &pk) {
  if (ts_use_ws(c.k)) {
    if constexpr (EPI == 1) return ws_launch_ks<1, 4>(c, pk);   // the value projection is 256 -> 256: the one KS built for it
    else return gemm_k64<4>(c.k / 64, [&](auto ks) { return ws_launch_ks<EPI, decltype(ks)::value>(c, pk); });
  }
  if (!ensure_dynamic_lds<tsgemm_f16_kernel<EPI>>(kTsLds)) return BEVOPS_FAILURE;
  const int units = (int)((c.m + 31) / 32);
  const dim3 grid((unsigned)ts_grid_x(units, c.n / kTsBN), (unsigned)(c.n / kTsBN));
  hipLaunchKernelGGL(tsgemm_f16_kernel<EPI>, grid, dim3(kTsThreads), kTsLds, c.st, (const __half *)c.x, (const __half *)c.w,
                     (const __half *)c.bias, (const __half *)c.res, (__half *)c.out, (int)c.m, c.n, c.k, c.relu, units, pk);
  return launch_status();
}

// what the three fp16 entries ask of the shared operands, after their null / sign checks (`w_limit`: the weight's byte
// range too; the one-chunk entries never asked)
int ts_f16_check(const GemmCall &c, bool w_limit) {
  if (c.m > 0x7fffffff || gemm_over_limit(c.m, c.k, 2) || (w_limit && gemm_over_limit(c.n, c.k, 2))) return BEVOPS_NOT_SUPPORTED;
  if (misaligned(c.x, 15u) || misaligned(c.w, 15u) || misaligned(c.out, 15u) || (c.bias && misaligned(c.bias, 15u)) ||
      (c.res && misaligned(c.res, 15u)))
    return BEVOPS_BAD_PARAM;
  return BEVOPS_SUCCESS;
}

// The checks bevops_tsgemm_s8 and _s8_ln share (`one_chunk`: N == 256 instead of N % 256 == 0, and the weight's byte
// range is not asked), after the entry's null / sign checks.
int ts_s8_check(const GemmCallS8 &c, bool one_chunk) {
  const bool res8 = c.res && c.res_dtype == BEVOPS_I8, out8 = c.out_dtype == BEVOPS_I8;
  if (!(c.scale_a > 0.f) || (!c.w_scales && !(c.scale_w > 0.f))) return BEVOPS_BAD_PARAM;
  if (c.k % 128 != 0 || (one_chunk ? c.n != kTsBN : c.n % kTsBN != 0)) return BEVOPS_NOT_SUPPORTED;
  if (!out8 && c.out_dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  if (c.res && !res8 && c.res_dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  if (out8 && !(c.scale_out > 0.f)) return BEVOPS_BAD_PARAM;
  if (res8 && !(c.scale_res > 0.f)) return BEVOPS_BAD_PARAM;
  if (c.m > 0x7fffffff || gemm_over_limit(c.m, c.k, 1) || (!one_chunk && gemm_over_limit(c.n, c.k, 1))) return BEVOPS_NOT_SUPPORTED;
  if (misaligned(c.x, 15u) || misaligned(c.w, 15u) || misaligned(c.out, out8 ? 7u : 15u) ||
      (c.res && misaligned(c.res, res8 ? 7u : 15u)) || (c.bias && misaligned(c.bias, 3u)) ||
      (c.w_scales && misaligned(c.w_scales, 3u)))
    return BEVOPS_BAD_PARAM;
  return BEVOPS_SUCCESS;
}

void ts_s8_fill(TsS8Args &p, const GemmCallS8 &c) {
  p.a = static_cast<const int8_t *>(c.x); p.w = static_cast<const int8_t *>(c.w);
  p.bias = static_cast<const float *>(c.bias); p.wscale = c.w_scales; p.res = c.res; p.out = c.out;
  p.s_aw = c.w_scales ? c.scale_a : c.scale_a * c.scale_w;
  p.s_res = c.scale_res;
  p.inv_s_out = c.out_dtype == BEVOPS_I8 ? 1.0f / c.scale_out : 0.f;
  p.M = (int)c.m; p.N = c.n; p.K = c.k; p.relu = c.relu; p.units_total = (int)((c.m + 31) / 32);
  p.res_i8 = c.res && c.res_dtype == BEVOPS_I8 ? 1 : 0;
  p.out_i8 = c.out_dtype == BEVOPS_I8 ? 1 : 0;
}

TsPacked ts_ln_params(const void *ln_weight, const void *ln_bias, float eps) {
  TsPacked pk{};
  pk.gset = const_cast<char *>(static_cast<const char *>(ln_weight));
  pk.sset = const_cast<char *>(static_cast<const char *>(ln_bias));
  pk.eps = eps;
  return pk;
}

// the partition of ws_launch_ks (not grouped) for a two-source call
template <int KS, int KS2>
int ws2_launch_ks(const Gemm2Call &g) {
  if (!ensure_dynamic_lds<tsgemm_ws2_kernel<KS, KS2>>(ws_lds(KS))) return BEVOPS_FAILURE;
  const int units = (int)((g.m + 31) / 32), chunks = g.n / kTsBN;
  int parts = ts_grid_x(1 << 30, chunks) / chunks;
  if (parts < 1) parts = 1;
  if (parts > units) parts = units;
  const TsSrc2 src2{(const __half *)g.a2, (unsigned)((unsigned long long)g.B * g.H * g.W * g.k2 * 2), g.H, g.W, g.ho, g.wo,
                    g.stride};
  hipLaunchKernelGGL((tsgemm_ws2_kernel<KS, KS2>), dim3((unsigned)(parts * chunks)), dim3(kTsThreads), ws_lds(KS), g.st,
                     (const __half *)g.a1, (const __half *)g.w, (const __half *)g.bias, (__half *)g.out, (int)g.m, g.n, g.relu,
                     units, parts, chunks, src2);
  return launch_status();
}

}  // namespace

// (gemm_host.h) K1 + K2 <= 256 and whole 256-column chunks, under the variant that runs the weight-stationary kernel
bool tsgemm_ws2_in_domain(const Gemm2Call &g) { return g.n % kTsBN == 0 && g.k1 + g.k2 <= 256 && ts_use_ws(g.k1 + g.k2); }

int tsgemm_ws2_launch(const Gemm2Call &g) {
  return gemm_k64<4>((g.k1 + g.k2) / 64, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    return gemm_k64<KS - 1>(g.k2 / 64, [&](auto ks2) { return ws2_launch_ks<KS, decltype(ks2)::value>(g); });
  });
}

}  // namespace bevops

using namespace bevops;

extern "C" int bevops_tsgemm_set_variant(int variant) {
  const int prev = g_ts_variant;
  g_ts_variant = variant;
  return prev;
}

// rows per tile of the kernel bevops_tsgemm_f16 runs for this k under the current variant (tests size their ragged
// cases with it); 0 outside the domain
extern "C" int bevops_tsgemm_tile_rows(int k) {
  if (k <= 0 || k % 64 != 0) return 0;
  return ts_use_ws(k) ? kWsRows : kTsG * 32;
}

extern "C" int bevops_tsgemm_f16(const void *x, const void *weight, const void *bias, const void *residual,
                                 void *out, long long m, int n, int k, int relu, void *stream) {
  const GemmCall c{x, weight, bias, residual, out, m, n, k, relu, static_cast<hipStream_t>(stream)};
  if (!x || !weight || !out || m <= 0 || n <= 0 || k <= 0) return BEVOPS_BAD_PARAM;
  if (k % 64 != 0 || n % kTsBN != 0) return BEVOPS_NOT_SUPPORTED;
  const int rc = ts_f16_check(c, true);
  return rc != BEVOPS_SUCCESS ? rc : ts_launch_f16<0>(c, TsPacked{});
}

// G dense layers of 256 columns over the SAME rows as one launch: out + g * group_stride (elements) receives the dense
// [M, 256] matrix x @ weight[g * 256 .. g * 256 + 255].T + bias[g * 256 ..], exactly the bytes of G calls of
// bevops_tsgemm_f16 with n = 256 (same kernel, same per-row arithmetic; a row is read from HBM once, by the chunks of its
// partition on one XCD).  K % 64 == 0, K <= 256 (the weight-stationary kernel's domain); no residual, no activation.
extern "C" int bevops_tsgemm_f16_grouped(const void *x, const void *weight, const void *bias, void *out,
                                         long long group_stride, long long m, int groups, int k, void *stream) {
  if (!x || !weight || !out || m <= 0 || groups <= 0 || k <= 0) return BEVOPS_BAD_PARAM;
  if (k % 64 != 0 || k > 256 || groups > 64) return BEVOPS_NOT_SUPPORTED;
  const GemmCall c{x, weight, bias, nullptr, out, m, groups * kTsBN, k, 0, static_cast<hipStream_t>(stream)};
  const int rc = ts_f16_check(c, false);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (group_stride < m * kTsBN || group_stride % 8 != 0) return BEVOPS_BAD_PARAM;   // the G outputs would overlap / lose alignment
  if (!ts_use_ws(k)) {   // the A/B variant: the G launches themselves
    for (int g = 0; g < groups; ++g) {
      const int rc_g = bevops_tsgemm_f16(x, static_cast<const __half *>(weight) + (size_t)g * kTsBN * k,
                                         bias ? static_cast<const __half *>(bias) + (size_t)g * kTsBN : nullptr, nullptr,
                                         static_cast<__half *>(out) + (size_t)g * (size_t)group_stride, m, kTsBN, k, 0, stream);
      if (rc_g != BEVOPS_SUCCESS) return rc_g;
    }
    return BEVOPS_SUCCESS;
  }
  TsPacked pk{};
  pk.gstride = group_stride;
  return gemm_k64<4>(k / 64, [&](auto ks) { return ws_launch_ks<0, decltype(ks)::value, true>(c, pk); });
}

// out = LayerNorm_256(fp16(x @ weight.T + bias + residual)) * ln_weight + ln_bias in ONE launch (EPI 2 above).
// N must be 256 (the embedding width of the encoder / decoder blocks), K % 64 == 0; fp16 operands, fp32 statistics.
extern "C" int bevops_tsgemm_f16_ln(const void *x, const void *weight, const void *bias, const void *residual,
                                    const void *ln_weight, const void *ln_bias, float eps, void *out, long long m, int n,
                                    int k, void *stream) {
  const GemmCall c{x, weight, bias, residual, out, m, n, k, 0, static_cast<hipStream_t>(stream)};
  if (!x || !weight || !out || !ln_weight || !ln_bias || m <= 0 || n <= 0 || k <= 0 || !(eps >= 0.f)) return BEVOPS_BAD_PARAM;
  if (k % 64 != 0 || n != kTsBN) return BEVOPS_NOT_SUPPORTED;
  const int rc = ts_f16_check(c, false);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(ln_weight, 15u) || misaligned(ln_bias, 15u)) return BEVOPS_BAD_PARAM;
  return ts_launch_f16<2>(c, ts_ln_params(ln_weight, ln_bias, eps));
}

// int8 chain flavour of the persistent tall-skinny GEMM (see tsgemm_s8_kernel).  a_q [M, K] / w_q [N, K] int8;
// w_scales fp32 [N] or NULL (then scale_w); bias fp32 [N] or NULL; residual [M, N] int8 (res_dtype BEVOPS_I8, real =
// q * scale_res) or fp16 or NULL; out [M, N] int8 (requantised with scale_out) or fp16.  Domain: K % 128 == 0,
// N % 256 == 0, 16-byte aligned operands (8-byte for the int8 identity / output rows).
extern "C" int bevops_tsgemm_s8(const void *a_q, float scale_a, const void *w_q, const float *w_scales, float scale_w,
                                const float *bias, const void *residual, int res_dtype, float scale_res, int out_dtype,
                                void *out, float scale_out, long long m, int n, int k, int relu, void *stream) {
  const GemmCallS8 c{{a_q, w_q, bias, residual, out, m, n, k, relu, static_cast<hipStream_t>(stream)},
                     w_scales, scale_a, scale_w, scale_res, scale_out, res_dtype, out_dtype};
  if (!a_q || !w_q || !out || m <= 0 || n <= 0 || k <= 0) return BEVOPS_BAD_PARAM;
  const int rc = ts_s8_check(c, false);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (!ensure_dynamic_lds<tsgemm_s8_kernel<0>>(kTsLds)) return BEVOPS_FAILURE;
  TsS8Args p;
  ts_s8_fill(p, c);
  const dim3 grid((unsigned)ts_grid_x(p.units_total, n / kTsBN), (unsigned)(n / kTsBN));
  hipLaunchKernelGGL(tsgemm_s8_kernel<0>, grid, dim3(kTsThreads), kTsLds, c.st, p);
  return launch_status();
}

// The int8 GEMM with the block's LayerNorm in its epilogue (tsgemm_s8_kernel<2>): arguments as bevops_tsgemm_s8 with an
// fp16 output and no ReLU, plus the norm's fp16 [256] weight / bias and eps.  N must be 256, K % 128 == 0; no workspace.
extern "C" int bevops_tsgemm_s8_ln(const void *a_q, float scale_a, const void *w_q, const float *w_scales, float scale_w,
                                   const float *bias, const void *residual, int res_dtype, float scale_res,
                                   const void *ln_weight, const void *ln_bias, float eps, void *out, long long m, int n,
                                   int k, void *stream) {
  const GemmCallS8 c{{a_q, w_q, bias, residual, out, m, n, k, 0, static_cast<hipStream_t>(stream)},
                     w_scales, scale_a, scale_w, scale_res, 1.f, res_dtype, BEVOPS_F16};
  if (!a_q || !w_q || !out || !ln_weight || !ln_bias || m <= 0 || n <= 0 || k <= 0 || !(eps >= 0.f)) return BEVOPS_BAD_PARAM;
  const int rc = ts_s8_check(c, true);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(ln_weight, 15u) || misaligned(ln_bias, 15u)) return BEVOPS_BAD_PARAM;
  if (!ensure_dynamic_lds<tsgemm_s8_kernel<2>>(kTsS8LnLds)) return BEVOPS_FAILURE;
  TsS8LnArgs p{};
  ts_s8_fill(p, c);
  p.pk = ts_ln_params(ln_weight, ln_bias, eps);
  hipLaunchKernelGGL(tsgemm_s8_kernel<2>, dim3((unsigned)ts_grid_x(p.units_total, 1)), dim3(kTsThreads), kTsS8LnLds, c.st, p);
  return launch_status();
}

// The encoder's value projection (spatial_cross_attention.py:754: value = self.value_proj(value)) written
// straight into the padded head-major planes of the SCA sampler: packed = [big set][staged set][visibility
// bytes], the layout bevops_msda_forward_prepacked consumes for the 4-level x 8-point shape.
extern "C" size_t bevops_value_proj_packed_size(const int32_t *spatial_shapes_host, int num_cams, int nk, int heads,
                                                int channels, int num_levels, int num_query, int num_point) {
  if (!spatial_shapes_host || num_cams <= 0 || nk <= 0) return 0;
  // 0 exactly where bevops_value_proj_packed answers NOT_SUPPORTED: whole 256-column tiles, the two-level staging
  if (heads <= 0 || channels != 32 || (heads * channels) % kTsBN != 0) return 0;
  const MsdaDims d{num_cams, nk, heads, channels, num_levels, num_query, num_point, 4, 1};
  Hm3Tab tab;
  size_t g_room = 0, s_bytes = 0;
  if (!msda_hm5_layout(d, spatial_shapes_host, &tab, &g_room, &s_bytes)) return 0;
  if (gemm_over_limit((unsigned long long)num_cams * nk, heads * channels, 2)) return 0;
  return msda_hm5_workspace_bytes(d, spatial_shapes_host);
}

extern "C" int bevops_value_proj_packed(const void *x, const void *weight, const void *bias,
                                        const int32_t *spatial_shapes_host, void *packed, size_t packed_bytes,
                                        int num_cams, int nk, int heads, int channels, int num_levels,
                                        int num_query, int num_point, void *stream) {
  if (!x || !weight || !spatial_shapes_host || !packed) return BEVOPS_BAD_PARAM;
  if (num_cams <= 0 || nk <= 0 || heads <= 0 || channels != 32 || (heads * channels) % kTsBN != 0) return BEVOPS_NOT_SUPPORTED;
  long total = 0;
  for (int l = 0; l < num_levels; ++l) total += (long)spatial_shapes_host[2 * l] * spatial_shapes_host[2 * l + 1];
  if (total != nk) return BEVOPS_BAD_PARAM;
  TsPacked pk{};
  size_t g_room = 0, s_bytes = 0;
  const MsdaDims d{num_cams, nk, heads, channels, num_levels, num_query, num_point, 4, 1};
  if (!msda_hm5_layout(d, spatial_shapes_host, &pk.t, &g_room, &s_bytes))
    return BEVOPS_NOT_SUPPORTED;
  if (packed_bytes < g_room + s_bytes || misaligned(packed, 127u)) return BEVOPS_BAD_PARAM;
  const int n = heads * channels;   // embed -> embed: K == N
  const GemmCall c{x, weight, bias, nullptr, nullptr, (long long)num_cams * nk, n, n, 0, static_cast<hipStream_t>(stream)};
  const int rc = ts_f16_check(c, false);
  if (rc != BEVOPS_SUCCESS) return rc;
  pk.gset = static_cast<char *>(packed);
  pk.sset = pk.gset + g_room;
  pk.nk = nk;
  pk.heads = heads;
  hipLaunchKernelGGL(tsgemm_pad_zero_kernel, dim3(4, (unsigned)(num_cams * heads)), dim3(256), 0, c.st, pk, num_cams * heads);
  return ts_launch_f16<1>(c, pk);
}

// The same planes from an already projected value tensor [num_cams, nk, heads, 32] (the re-layout pass of the
// drop-in call as an entry of its own): what bevops_value_proj_packed must reproduce byte for byte when
// `value` is its own GEMM's output.
extern "C" int bevops_value_pack_planes(const void *value, const int32_t *spatial_shapes_host, void *packed,
                                        size_t packed_bytes, int num_cams, int nk, int heads, int channels,
                                        int num_levels, int num_query, int num_point, void *stream) {
  if (!value || !spatial_shapes_host || !packed) return BEVOPS_BAD_PARAM;
  TsPacked pk{};
  size_t g_room = 0, s_bytes = 0;
  const MsdaDims d{num_cams, nk, heads, channels, num_levels, num_query, num_point, 4, 1};
  if (!msda_hm5_layout(d, spatial_shapes_host, &pk.t, &g_room, &s_bytes))
    return BEVOPS_NOT_SUPPORTED;
  if (packed_bytes < g_room + s_bytes || misaligned(packed, 127u)) return BEVOPS_BAD_PARAM;
  msda_hm3_repack_launch(value, static_cast<char *>(packed), static_cast<char *>(packed) + g_room, pk.t, num_cams, nk,
                         heads, static_cast<hipStream_t>(stream));
  return launch_status();
}
