// Dense layers with FEW rows (the decoder's 900 object queries, SURVEY.md 8a-5: decoder.py:381-471 and the branches of
// bevformer_head.py:247-282; not reference plugins -- TensorRT owns these layers there):
//     out[m, n] = act( sum_k x[m, k] w[n, k] + bias[n] (+ residual[m, n]) ),   fp16 in / out, fp32 sums.
// At M = 900 the tiled GEMMs (tile_gemm.hip, tsgemm.hip) run 16-32 blocks that each walk a chain of 8-16 dependent
// k-steps (load -> LDS -> barrier -> MFMA, ~1.5 us per step): 15-16 us for 0.1-0.2 GFLOP, sixty times per frame.
// Such a layer has no bandwidth or matrix-core problem, only that chain.  Here there is NO k-loop pipeline at all:
//   * block tile 32 rows x 64 columns (M = 900, N = 256: 116 blocks), 256 threads = 4 waves, each wave owns a QUARTER of
//     K (split-K inside the block);
//   * a wave loads its operands straight from global memory in matrix-instruction fragment layout -- lane (l & 31) is
//     the row, (l >> 5) the 8-value half of a 16-value k-step: one 16-byte buffer load per lane, fragment and step --
//     and issues ALL of them before the first v_mfma_f32_32x32x16_f16: one memory round trip per launch;
//   * the four waves' fp32 partial tiles meet in LDS (32 KB), every thread then owns 8 consecutive columns of one row:
//     bias, identity, ReLU in fp32, one rounding, one 16-byte store.
// Rows / columns past M / N read as zero through the buffer descriptors' range check and are not stored.
// Domain: K % 64 == 0 (four k-quarters of whole 16-value steps), K <= 1024 (operand registers), 16-byte aligned rows.
#include "gemm_host.h"

namespace bevops {
namespace {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int kSgM = 32, kSgN = 64, kSgStride = kSgN + 4;   // partial rows padded by 4 floats (bank spread)

struct SmallArgs {
  const __half *x, *w, *bias, *res;
  __half *out;
  int M, N, K, relu;
};

// DST (bevops_small_gemm_f16_dst): the output columns go to up to kGemmMaxDst destinations, each a column range of the
// launch written as a pitched matrix of its own with an identity of its own -- layers that read the same rows as ONE
// launch.  A range begins on a multiple of 64, so a block's 64 columns have one destination, found by compare-and-select
// over the by-value table with the block's n0 (scalar); columns of the block past the range's end are not stored.
// Everything in front of the identity add is the code of the plain launch.

// STEPS = k-steps (of 16 values) per wave = K / 64
template <int STEPS, bool DST>
__device__ __forceinline__ void small_gemm_body(const SmallArgs &p, const GemmDstTab &d) {
  __shared__ __attribute__((aligned(16))) float part[4][kSgM][kSgStride];   // 34.8 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_n = (p.N + kSgN - 1) / kSgN;
  const int m0 = ((int)blockIdx.x / tiles_n) * kSgM, n0 = ((int)blockIdx.x % tiles_n) * kSgN;
  const int K = p.K;
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__half *>(p.x), 0, (unsigned)((size_t)p.M * K * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__half *>(p.w), 0, (unsigned)((size_t)p.N * K * 2), 0x00020000);
  const int r = lane & 31, half = lane >> 5;
  const int kq = wave * (K / 4) + half * 8;          // first k of this lane's fragments in the wave's quarter
  const unsigned xo = m0 + r < p.M ? (unsigned)(((size_t)(m0 + r) * K + kq) * 2) : kGemmOob;
  const unsigned wo0 = n0 + r < p.N ? (unsigned)(((size_t)(n0 + r) * K + kq) * 2) : kGemmOob;
  const unsigned wo1 = n0 + 32 + r < p.N ? (unsigned)(((size_t)(n0 + 32 + r) * K + kq) * 2) : kGemmOob;
  // every operand fragment of the wave's quarter, requested before any is used
  u32x4 fx[STEPS], fw0[STEPS], fw1[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    fx[s] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)xo, s * 32, 0);
    fw0[s] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)wo0, s * 32, 0);
    fw1[s] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)wo1, s * 32, 0);
  }
  // the identity rows of the epilogue do not depend on the sums either
  const int er = tid >> 3, ec = (tid & 7) * 8;       // epilogue role: row er, columns ec .. ec + 7 of the tile
  const int em = m0 + er, en = n0 + ec;
  const bool vec = (p.N & 7) == 0;
  // DST: this block's destination (block-uniform); d_out stays null for a block outside every range
  __half *d_out = nullptr;
  const __half *d_res = nullptr;
  int d_c0 = 0, d_c1 = 0, d_op = 0, d_rp = 0;
  if constexpr (DST) {
#pragma unroll
    for (int e = 0; e < kGemmMaxDst; ++e) {
      const bool hit = e < d.count && n0 >= d.e[e].col_begin && n0 < d.e[e].col_end;
      d_out = hit ? d.e[e].out : d_out;
      d_res = hit ? d.e[e].res : d_res;
      d_c0 = hit ? d.e[e].col_begin : d_c0;
      d_c1 = hit ? d.e[e].col_end : d_c1;
      d_op = hit ? d.e[e].out_pitch : d_op;
      d_rp = hit ? d.e[e].res_pitch : d_rp;
    }
  }
  const bool dst_ok = !DST || (d_out != nullptr && en < d_c1);   // (range ends are multiples of 8: a chunk is all in or all out)
  const __half *res = DST ? d_res : p.res;
  uint4 rres = make_uint4(0u, 0u, 0u, 0u);
  if (res && vec && em < p.M && en < p.N && dst_ok)
    rres = *reinterpret_cast<const uint4 *>(DST ? res + (size_t)em * d_rp + (en - d_c0) : res + (size_t)em * p.N + en);
  f32x16_t acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  // operand A = weight rows (output columns), B = activation rows: a lane's 4 consecutive accumulator values are 4
  // consecutive n of one output row m (the fragment convention of tile_gemm.hip)
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const f16x8_t b = __builtin_bit_cast(f16x8_t, fx[s]);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, fw0[s]), b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, fw1[s]), b, acc1, 0, 0, 0);
  }
  // acc{cb}[4 g + c]: m = r, n = cb * 32 + 8 g + 4 half + c
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *reinterpret_cast<f32x4 *>(&part[wave][r][8 * g + 4 * half]) =
        f32x4{acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]};
    *reinterpret_cast<f32x4 *>(&part[wave][r][32 + 8 * g + 4 * half]) =
        f32x4{acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]};
  }
  __syncthreads();
  if (em >= p.M || en >= p.N || !dst_ok) return;
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = 0.f;
#pragma unroll
  for (int w4 = 0; w4 < 4; ++w4) {      // fixed order: the result does not depend on which wave finished first
    const f32x4 lo = *reinterpret_cast<const f32x4 *>(&part[w4][er][ec]);
    const f32x4 hi = *reinterpret_cast<const f32x4 *>(&part[w4][er][ec + 4]);
#pragma unroll
    for (int c = 0; c < 4; ++c) { v[c] += lo[c]; v[4 + c] += hi[c]; }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (p.bias && en + c < p.N) v[c] += __half2float(p.bias[en + c]);
  if (res) {
    if (vec) {
      v[0] += h2f_lo(rres.x); v[1] += h2f_hi(rres.x); v[2] += h2f_lo(rres.y); v[3] += h2f_hi(rres.y);
      v[4] += h2f_lo(rres.z); v[5] += h2f_hi(rres.z); v[6] += h2f_lo(rres.w); v[7] += h2f_hi(rres.w);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (en + c < p.N) v[c] += __half2float(res[(size_t)em * p.N + en + c]);   // (never with DST: N % 8 == 0 there)
    }
  }
  if (p.relu) {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = fmaxf(v[c], 0.f);
  }
  __half *o = DST ? d_out + (size_t)em * d_op + (en - d_c0) : p.out + (size_t)em * p.N + en;
  if (vec) {
    uint4 q;
    q.x = pack_h2(v[0], v[1]); q.y = pack_h2(v[2], v[3]); q.z = pack_h2(v[4], v[5]); q.w = pack_h2(v[6], v[7]);
    *reinterpret_cast<uint4 *>(o) = q;
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (en + c < p.N) o[c] = __float2half_rn(v[c]);
  }
}

template <int STEPS>
__global__ __launch_bounds__(256) void small_gemm_f16_kernel(SmallArgs p) {
  small_gemm_body<STEPS, false>(p, GemmDstTab{});
}

template <int STEPS>
__global__ __launch_bounds__(256) void small_gemm_dst_kernel(SmallArgs p, GemmDstTab d) {
  small_gemm_body<STEPS, true>(p, d);
}

// the launch of both entries, after their checks
template <bool DST>
int small_launch(const GemmCall &c, const GemmDstTab &tab) {
  if (c.m == 0) return BEVOPS_SUCCESS;
  SmallArgs p{static_cast<const __half *>(c.x), static_cast<const __half *>(c.w), static_cast<const __half *>(c.bias),
              static_cast<const __half *>(c.res), static_cast<__half *>(c.out), (int)c.m, c.n, c.k, c.relu};
  const long long blocks = ((c.m + kSgM - 1) / kSgM) * ((c.n + kSgN - 1) / kSgN);
  if (blocks > 0x7fffffffLL) return BEVOPS_NOT_SUPPORTED;
  const dim3 grid((unsigned)blocks), blk(256);
  const int rc = gemm_k64<16>(c.k / 64, [&](auto steps) {
    constexpr int S = decltype(steps)::value;
    if constexpr (DST) hipLaunchKernelGGL(small_gemm_dst_kernel<S>, grid, blk, 0, c.st, p, tab);
    else hipLaunchKernelGGL(small_gemm_f16_kernel<S>, grid, blk, 0, c.st, p);
    return BEVOPS_SUCCESS;
  });
  return rc != BEVOPS_SUCCESS ? rc : launch_status();
}

// what both entries ask of the shared operands: K in whole k-quarters of 16-value steps that fit the operand registers
inline bool small_domain(const GemmCall &c) {
  return c.k % 64 == 0 && c.k <= 1024 && c.m <= 65536 && !misaligned(c.x, 15u) && !misaligned(c.w, 15u);
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_small_gemm_f16(const void *x, const void *weight, const void *bias, const void *residual,
                                     void *out, long long M, int N, int K, int relu, void *stream) {
  const GemmCall c{x, weight, bias, residual, out, M, N, K, relu, static_cast<hipStream_t>(stream)};
  if (!x || !weight || !out || M < 0 || N <= 0 || K <= 0) return BEVOPS_BAD_PARAM;
  if (!small_domain(c) || misaligned(out, 15u) || (residual && misaligned(residual, 15u)) || (bias && misaligned(bias, 1u)))
    return BEVOPS_NOT_SUPPORTED;
  if (gemm_over_limit(M, K, 2) || gemm_over_limit(N, K, 2)) return BEVOPS_NOT_SUPPORTED;
  return small_launch<false>(c, GemmDstTab{});
}

// bevops_small_gemm_f16 with a destination table (the decoder's sampling_offsets | attention_weights over the same 900
// queries: N = 64 + 32, the two cached query_pos terms as identities): range [col_begin, col_end) of x @ weight.T + bias
// goes to the pitched matrix of its destination, plus that destination's identity rows.  Exactly the bytes of the separate
// launches on weight[col_begin:col_end]; columns outside every range and the bytes between pitched rows are never written.
extern "C" int bevops_small_gemm_f16_dst(const void *x, const void *weight, const void *bias, const bevops_gemm_dst *dst,
                                         int num_dst, long long M, int N, int K, int relu, void *stream) {
  const GemmCall c{x, weight, bias, nullptr, nullptr, M, N, K, relu, static_cast<hipStream_t>(stream)};
  if (!x || !weight || !dst || M < 0 || N <= 0 || K <= 0 || num_dst <= 0) return BEVOPS_BAD_PARAM;
  if (num_dst > kGemmMaxDst || N % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  if (!small_domain(c) || (bias && misaligned(bias, 15u))) return BEVOPS_NOT_SUPPORTED;
  if (gemm_over_limit(M, K, 2) || gemm_over_limit(N, K, 2)) return BEVOPS_NOT_SUPPORTED;
  GemmDstTab tab;
  const int rc = gemm_dst_table(tab, dst, num_dst, M, N, 8, false);
  return rc != BEVOPS_SUCCESS ? rc : small_launch<true>(c, tab);
}
