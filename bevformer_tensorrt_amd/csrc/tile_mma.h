// The 128-row tiled matrix-core skeleton of the dense / convolution family (tile_gemm.hip, conv_slice.hip,
// conv_slice_s8.hip, deconv.hip, deconv_s8.hip): what every user of it restated before.  design/dense.md, "The 128-row
// tile skeleton and who uses it".
//
// MI355X mapping.  128 x 128 output tiles (128 x 64 for Cout <= 64: NI == 1), 256 threads = 4 waves of 64 x 64 (64 x 32):
// 2 x NI MFMA blocks of 32 x 32 per wave.  64 BYTES of k per step and row in every flavour (32 fp16 values for
// v_mfma_f32_32x32x16_f16, 64 int8 values for v_mfma_i32_32x32x32_i8: the LDS images, the 16-byte fragment reads and the
// staging stores are the same code).  Operands are register-staged through range-checked 16-byte buffer loads (rows past
// M / N and taps outside the image are given the beyond-the-buffer address kGemmOob and read as zero, no branches): a
// thread moves one 16-byte chunk of two activation rows and of two weight rows (one at NI == 1) per step, in TWO register
// sets, so that the loads of two steps are in flight per block, and writes a set into the OTHER of two LDS images while
// the current one is multiplied: one barrier per step.  40 960 bytes of LDS and __launch_bounds__(256, 3): four blocks per
// CU at <= 128 VGPRs, three at <= 168; their prologues, k-loops and epilogues interleave, which covers the HBM latency.
// Tiles are numbered so that the column tiles of one row tile run back to back on one XCD (block b runs on XCD b % 8):
// the activation rows come from HBM once and from that XCD's L2 afterwards.
// Epilogue: the raw sums go through LDS per wave (32 rows x 32 NI columns at a time) so that a thread owns CW consecutive
// channels of one output row and handles them with 16-byte accesses.
//
// A kernel supplies its geometry as ONE callable -- fill a staging set with the next step's four loads and advance the
// own (k, tap, channel) position -- and its arithmetic as ONE callable on (row, CW raw sums).
#pragma once
#include "gemm_host.h"

namespace bevops {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr int kTM = 128;                       // rows per tile
constexpr int kTMJ = 2;                        // 32-row MFMA blocks per wave
constexpr int kTLd = 64 + 16;                  // LDS row: the step's 64 bytes + 16 (conflict-free 16-byte fragment reads)
constexpr int kEpiStride = 64 * 4 + 16;        // staging row: 64 x 4 bytes + pad
constexpr int kLds = 2 * (kTM + 128) * kTLd;   // two images of [A rows | W rows]; the epilogue's 4 x 32 staging rows fit
static_assert(kLds >= 4 * 32 * kEpiStride, "epilogue staging must fit in the operand images");

enum { kActNone = 0, kActRelu = 1, kActSilu = 2 };

// a range-checked 16-byte load: the check is on voff alone (the scalar offset takes no part in it)
__device__ __forceinline__ uint4 bload(const __amdgpu_buffer_rsrc_t &rs, unsigned voff, int soff = 0) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, soff, 0));
}

// one matrix-core instruction on 16-byte fragments: a = 32 weight rows, b = 32 activation rows
__device__ __forceinline__ f32x16_t mma(i32x4_t a, i32x4_t b, f32x16_t acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}
__device__ __forceinline__ i32x16_t mma(i32x4_t a, i32x4_t b, i32x16_t acc) {
  return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
}

__device__ __forceinline__ int sum_bits(float v) { return __float_as_int(v); }
__device__ __forceinline__ int sum_bits(int v) { return v; }

// v * sigmoid(v) = v * rcp(1 + exp(-v)): hardware exponential and reciprocal (1 ulp).  exp(-v) overflows to +inf for
// v < -88.7, where the result is -0; for v > 88 it is v (design/yolox.md derives the bound the tests assert)
__device__ __forceinline__ float silu_f32(float v) { return v * __builtin_amdgcn_rcpf(1.f + __expf(-v)); }

__device__ __forceinline__ int s8_at(const unsigned *w, int c) {   // signed byte c of a little-endian word array
  return (int)(w[c >> 2] << (24 - 8 * (c & 3))) >> 24;
}

// q = clamp(rne(v * inv), -127, 127) into the bytes of CW / 4 words: one rounding for the product, v_rndne_f32, max, min
// (a NaN leaves as -127: max(NaN, -127) = -127)
template <int CW>
__device__ __forceinline__ void requant_s8_pack(const float (&v)[CW], float inv, unsigned (&pk)[CW / 4]) {
#pragma unroll
  for (int q = 0; q < CW / 4; ++q) pk[q] = 0u;
#pragma unroll
  for (int c = 0; c < CW; ++c)
    pk[c >> 2] |= ((unsigned)(int)fminf(fmaxf(rintf(v[c] * inv), -127.f), 127.f) & 0xffu) << (8 * (c & 3));
}

// Where a block and a thread stand.  The 8 XCDs take contiguous runs of the [row][column tile] sequence, `cols` column
// tiles per row.  The deconvolution's [row tile][parity][column tile] order is the same numbering read with
// row = 4 * row tile + parity (a shift and a mask in the kernel, no second division).
struct TilePos {
  int tid, lane, wave, wm, wn;                 // wave (wm, wn) owns rows wm * 64 .. + 63, columns wn * 32 NI .. of the tile
  int r0, r1, lchunk;                          // staging: rows r0 and r0 + 64, byte lchunk of the step's 64 (and of an LDS row)
  int row_tile, col;
  bool valid;                                  // false: a block of the grid's padding -- return at once
  __device__ __forceinline__ TilePos(int tiles_total, int cols) {
    tid = threadIdx.x;
    lane = tid & 63; wave = tid >> 6;
    wm = wave >> 1; wn = wave & 1;
    const int per_xcd = (tiles_total + 7) >> 3;
    const int logical = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    valid = logical < tiles_total;
    row_tile = logical / cols; col = logical % cols;
    r0 = tid >> 2; r1 = r0 + 64;
    lchunk = (tid & 3) * 16;
  }
  // first of the CW consecutive channels this thread owns in the epilogue, n0 the tile's first column
  template <int NI, int CW>
  __device__ __forceinline__ int epi_col(int n0) const { return n0 + wn * 32 * NI + (lane & (32 * NI / CW - 1)) * CW; }
};

// one step's loads of a staging thread: 16 bytes of activation rows r0, r1 and of weight rows r0, r1 (b1: NI == 2 only)
struct TileStage { uint4 a0, a1, b0, b1; };

// The k-loop, a statement macro: declares Acc acc[NI][kTMJ] = sum over nk steps, on the kernel's `char smem[kLds]` and its
// TilePos t.  load(TileStage &) requests the NEXT step's chunks and advances the caller's position; it is called for
// nk + 3 (+ 1 for an odd nk) steps: loads past the last step are issued too -- the callable gives them beyond-the-buffer
// addresses, they read as zero -- and so are the LDS writes of a step that does not exist, into the image nobody reads:
// no branches, exact wait counts.  An odd step count runs one step on zeros.  One step: image (kt + 1) & 1 was last read
// in step kt - 1, which every wave left through the barrier; the set written to it is free again and takes step kt + 3.
// MFMA operand A = the weight rows (output channels n), B = the activation rows (m): a lane's 4 consecutive accumulator
// rows are then 4 consecutive channels of one output row.  The two register sets are named, never indexed at run time.
// A macro and not a function template: through a template (measured, design/dense.md) the compiler rotates the loop's
// schedule -- the fp16 deconvolutions lose 4 % -- and packs conv_slice_s8's 128-column kernels into 128 VGPRs, a fourth
// block per CU; expanded in the kernel's body the code is the one the five files stated before.
#define BEVOPS_TILE_K_LOOP(smem, t, Acc, NI, nk_, acc, load)                                                           \
  Acc acc[NI][kTMJ];                                                                                                    \
  {                                                                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < NI; ++i_)                                                                   \
      _Pragma("unroll") for (int j_ = 0; j_ < kTMJ; ++j_)                                                               \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) acc[i_][j_][r_] = 0;                                          \
    TileStage s0_, s1_;                                                                                                 \
    auto lstore_ = [&](int buf, const TileStage &s) {                                                                   \
      char *As = smem + buf * (kTM + 128) * kTLd, *Ws = As + kTM * kTLd;                                                \
      *reinterpret_cast<uint4 *>(As + t.r0 * kTLd + t.lchunk) = s.a0;                                                   \
      *reinterpret_cast<uint4 *>(As + t.r1 * kTLd + t.lchunk) = s.a1;                                                   \
      *reinterpret_cast<uint4 *>(Ws + t.r0 * kTLd + t.lchunk) = s.b0;                                                   \
      if constexpr (NI == 2) *reinterpret_cast<uint4 *>(Ws + t.r1 * kTLd + t.lchunk) = s.b1;                            \
    };                                                                                                                  \
    auto compute_ = [&](int kt) {                                                                                       \
      const char *As = smem + (kt & 1) * (kTM + 128) * kTLd, *Ws = As + kTM * kTLd;                                     \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                                \
        const int kk = ks * 32 + (t.lane >> 5) * 16;                                                                    \
        i32x4_t a[NI], b[kTMJ];                                                                                         \
        _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                                  \
          a[i] = *reinterpret_cast<const i32x4_t *>(Ws + (t.wn * 32 * NI + i * 32 + (t.lane & 31)) * kTLd + kk);        \
        _Pragma("unroll") for (int j = 0; j < kTMJ; ++j)                                                                \
          b[j] = *reinterpret_cast<const i32x4_t *>(As + (t.wm * 32 * kTMJ + j * 32 + (t.lane & 31)) * kTLd + kk);      \
        _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                                  \
          _Pragma("unroll") for (int j = 0; j < kTMJ; ++j) acc[i][j] = mma(a[i], b[j], acc[i][j]);                      \
      }                                                                                                                 \
    };                                                                                                                  \
    load(s0_);                                                                                                          \
    lstore_(0, s0_);                                                                                                    \
    load(s1_);                                                                                                          \
    load(s0_);                                                                                                          \
    __syncthreads();                                                                                                    \
    auto step_ = [&](int kt, TileStage &next) {                                                                         \
      lstore_((kt + 1) & 1, next);                                                                                      \
      load(next);                                                                                                       \
      compute_(kt);                                                                                                     \
      __syncthreads();                                                                                                  \
    };                                                                                                                  \
    for (int kt = 0, nk = (nk_); kt < nk; kt += 2) {                                                                    \
      step_(kt, s1_);                                                                                                   \
      step_(kt + 1, s0_);                                                                                               \
    }                                                                                                                   \
  }

__device__ __forceinline__ f32x4 acc_quad(const f32x16_t &a, int g) { return f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]}; }
__device__ __forceinline__ i32x4_t acc_quad(const i32x16_t &a, int g) { return i32x4_t{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]}; }

// The epilogue transpose.  acc[i][j][4 g + c] is n = n0 + wn*32*NI + i*32 + 8 g + 4 (lane >> 5) + c,
// m = m0 + wm*64 + j*32 + (lane & 31); through the wave's 32 staging rows (the barrier that ended the last step freed both
// LDS images) a thread gets the CW sums of channels epi_col<NI, CW>(n0) .. of row m, as CW / 4 vectors of four, and
// fn(m, sums) is called where m < M and col_ok.  The LDS reads stand in front of that test, not under it.
template <int NI, int CW, class Acc, class Fn>
__device__ __forceinline__ void tile_epilogue(char *smem, const TilePos &t, const Acc (&acc)[NI][kTMJ], int m0, int M,
                                              bool col_ok, Fn fn) {
  constexpr int kCH = 32 * NI / CW;            // chunks per row of the wave's 32 NI columns
  constexpr int kRows = 64 / kCH;              // staged rows per read-back pass
  constexpr int kIT = 32 / kRows;              // passes over the wave's 32 staged rows
  using Quad = decltype(acc_quad(acc[0][0], 0));
  const int lane = t.lane, cc = lane & (kCH - 1);
  char *stage = smem + t.wave * 32 * kEpiStride;
#pragma unroll
  for (int j = 0; j < kTMJ; ++j) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<Quad *>(stage + (lane & 31) * kEpiStride + (i * 32 + 8 * g + 4 * (lane >> 5)) * 4) = acc_quad(acc[i][j], g);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < kIT; ++it) {
      const int row = it * kRows + lane / kCH;
      const int m = m0 + t.wm * 32 * kTMJ + j * 32 + row;
      Quad s[CW / 4];
#pragma unroll
      for (int q = 0; q < CW / 4; ++q) s[q] = *reinterpret_cast<const Quad *>(stage + row * kEpiStride + cc * CW * 4 + q * 16);
      if (m < M && col_ok) fn(m, s);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// The grid of a launch: 128-column tiles, 64-column ones for cout <= 64 (no matrix work on columns that do not exist);
// `per_row_tile` launches of the column tiles per 128 rows (4: the deconvolution's parities).  The grid is padded to a
// multiple of the 8 XCDs.  false: more tiles than a grid numbers.
inline bool tile_grid(unsigned long long rows, int cout, int per_row_tile, int *tiles_n, int *tiles_total, dim3 *grid) {
  const int tn = cout <= 64 ? 64 : 128;
  *tiles_n = (cout + tn - 1) / tn;
  const long long tiles = (long long)per_row_tile * *tiles_n * (long long)((rows + kTM - 1) / kTM);
  if (tiles > 0x3fffffffLL) return false;
  *tiles_total = (int)tiles;
  *grid = dim3((unsigned)((tiles + 7) / 8 * 8));
  return true;
}

}  // namespace bevops
