// The front of a plain LSS view transformer in ONE launch (bevops_lss_depth_head_f16; LSSViewTransformer.depth_net, the
// softmax over the depth bins and the two slice / permute copies of bevformer_tensorrt_amd/bevdet.py; design/depth_head.md):
//     v[m, j]        = b[j] + sum_k x[m, k] W[j, k]                 fp32 sum on the matrix cores, fp32 bias
//     feat[i, p, c]  = fp16(v[m, c])                      c < C     ONE rounding; pixel-major [n, hw, C]
//     depth[i, d, p] = fp16(exp(v_d - max_d v) / sum_d exp(v_d - max_d v))      plane-major [n, D, hw]; fp32, ONE rounding
// with m = i hw + p.  Neither v nor the logits reach memory.
//
// MI355X mapping.  Rows are scarce (4 224 at batch 1) and columns plenty (C + D up to 256), so a block owns only 32 rows
// -- ONE N-tile of v_mfma_f32_32x32x16_f16 -- and its four waves split the 32-column tiles: wave w takes tiles w and
// w + 4.  132 blocks at batch 1 instead of the 33 of a 128-row tile.  The weight rows are operand A, the pixel rows
// operand B, so a lane's accumulator holds 16 columns of ONE pixel m = lane & 31 (columns 32 t + 8 g + 4 (lane >> 5) + c)
// and its partner lane ^ 32 the other 16.
// No LDS for the operands.  Every weight byte is used by exactly one wave of a block, so staging it would only add a
// round trip: pack_depth_head stores W in fragment order [tile][k-step][lane][8] and an A fragment is one contiguous
// 1 KB wave load.  The block's 32 x Cin input rows (2 - 32 KB) are read by each wave as B fragments, 16 bytes a lane,
// from L1 / L2.  Both are prefetched in registers: two named sets of KC k-steps, the next set in flight while the
// current one is multiplied.
// Softmax on the accumulators: a lane's running maximum over its own depth columns, one half-swap, 512 bytes of LDS
// across the four waves; the same for the sum.  Columns that round C + D up to the tile take part in neither.
// Stores straight from registers.  Depth is a transpose: for one register the 32 lanes of a half hold 32 consecutive
// pixels of ONE plane, so a store instruction writes two 64-byte segments.  Features: the two halves swap 8 bytes so
// that a lane writes 8 consecutive channels as one 16-byte vector.  C % 8 == 0 keeps every group of 8 columns on one
// side of the feature / depth boundary.  A block's rows may straddle an image: every lane addresses from its own m.
#include <cmath>

#include "tile_mma.h"

namespace bevops {
namespace {

constexpr int kDhRows = 32;                    // rows per block

struct DhArgs {
  const __half *x;
  const i32x4_t *w;                            // [nt][nks][64] fragments of 16 bytes
  const float *bias;                           // [32 nt]
  __half *depth, *feat;
  long long rows;
  int hw, x_pitch, nks, C, D, nt;
};

template <int NTW, int KC>
struct DhSet {
  i32x4_t a[NTW][KC], b[KC];
};

// NTW: column tiles per wave (1 when C + D <= 128); KC: k-steps of 16 per register set
template <int NTW, int KC>
__global__ __launch_bounds__(256) void depth_head_kernel(DhArgs p) {
  __shared__ float red[2][4][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hb = lane >> 5;
  const int nks = p.nks, C = p.C, D = p.D, nt = p.nt;
  const long long m = (long long)blockIdx.x * kDhRows + l31;
  const bool row_ok = m < p.rows;
  // (a lane past the last row multiplies the last row again and stores nothing)
  const __half *xr = p.x + (row_ok ? m : p.rows - 1) * p.x_pitch + hb * 8;

  f32x16_t acc[NTW];
#pragma unroll
  for (int i = 0; i < NTW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  auto load = [&](DhSet<NTW, KC> &s, int ch) {
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const int ks = ch * KC + j;
      s.b[j] = i32x4_t{0, 0, 0, 0};
      if (ks < nks) s.b[j] = *reinterpret_cast<const i32x4_t *>(xr + ks * 16);
#pragma unroll
      for (int i = 0; i < NTW; ++i) {
        const int t = wave + 4 * i;
        s.a[i][j] = i32x4_t{0, 0, 0, 0};
        if (ks < nks && t < nt) s.a[i][j] = p.w[((size_t)t * nks + ks) * 64 + lane];
      }
    }
  };
  auto compute = [&](const DhSet<NTW, KC> &s, int ch) {
#pragma unroll
    for (int j = 0; j < KC; ++j)
      if (ch * KC + j < nks) {
#pragma unroll
        for (int i = 0; i < NTW; ++i)
          if (wave + 4 * i < nt) acc[i] = mma(s.a[i][j], s.b[j], acc[i]);
      }
  };
  DhSet<NTW, KC> s0, s1;
  const int nch = (nks + KC - 1) / KC;
  load(s0, 0);
  load(s1, 1);                                 // (a chunk past the last one loads nothing)
  for (int ch = 0; ch < nch; ch += 2) {
    compute(s0, ch);
    load(s0, ch + 2);
    compute(s1, ch + 1);
    load(s1, ch + 3);
  }

  // ---- bias in fp32; the lane's maximum over its own depth columns (d = column - C < D: no padded column)
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int t = wave + 4 * i;
    if (t < nt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = 32 * t + 8 * g + 4 * hb;
        const f32x4 bq = *reinterpret_cast<const f32x4 *>(p.bias + cb);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          acc[i][4 * g + c] += bq[c];
          if (cb >= C && cb + c - C < D) mx = fmaxf(mx, acc[i][4 * g + c]);
        }
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if (hb == 0) red[0][wave][l31] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][0][l31], red[0][1][l31]), fmaxf(red[0][2][l31], red[0][3][l31]));

  // ---- exponentials and their sum in fp32 (a row of NaN logits has mx = -inf: its exponentials are NaN)
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int t = wave + 4 * i;
    if (t < nt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = 32 * t + 8 * g + 4 * hb;
        if (cb >= C) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (cb + c - C < D) {
              const float e = expf(acc[i][4 * g + c] - mx);
              acc[i][4 * g + c] = e;
              sum += e;
            }
        }
      }
    }
  }
  sum += __shfl_xor(sum, 32, 64);
  if (hb == 0) red[1][wave][l31] = sum;
  __syncthreads();
  sum = (red[1][0][l31] + red[1][1][l31]) + (red[1][2][l31] + red[1][3][l31]);
  const float inv = 1.f / sum;

  // ---- stores: a plane's 32 consecutive pixels per lane half; 8 feature channels per lane after the half-swap
  const long long img = m / p.hw, px = m - img * p.hw;
  __half *dp = p.depth + img * D * (long long)p.hw + px;
  __half *fp = p.feat + m * C;
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int t = wave + 4 * i;
    if (t < nt) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int g0 = 2 * q, g1 = g0 + 1, c0 = 32 * t + 8 * g0, c1 = c0 + 8;
        if (c0 < C) {                          // (uniform in the wave: the shuffles below run in every lane)
          const unsigned lo0 = pack_h2(acc[i][4 * g0], acc[i][4 * g0 + 1]), hi0 = pack_h2(acc[i][4 * g0 + 2], acc[i][4 * g0 + 3]);
          const unsigned lo1 = pack_h2(acc[i][4 * g1], acc[i][4 * g1 + 1]), hi1 = pack_h2(acc[i][4 * g1 + 2], acc[i][4 * g1 + 3]);
          // half 0 writes group g0 and needs the partner's quad of it, half 1 writes g1
          const unsigned rlo = (unsigned)__shfl_xor((int)(hb ? lo0 : lo1), 32, 64);
          const unsigned rhi = (unsigned)__shfl_xor((int)(hb ? hi0 : hi1), 32, 64);
          if (row_ok && hb == 0) *reinterpret_cast<uint4 *>(fp + c0) = make_uint4(lo0, hi0, rlo, rhi);
          if (row_ok && hb == 1 && c1 < C) *reinterpret_cast<uint4 *>(fp + c1) = make_uint4(rlo, rhi, lo1, hi1);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = 32 * t + 8 * g + 4 * hb;
        if (cb >= C && row_ok) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int d = cb + c - C;
            if (d < D) dp[(long long)d * p.hw] = __float2half(acc[i][4 * g + c] * inv);
          }
        }
      }
    }
  }
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_lss_depth_head_f16(const void *x, int x_pitch, const void *w_packed, const void *bias_packed,
                                         void *depth, void *feat, int n, int hw, int Cin, int C, int D, void *stream) {
  if (!x || !w_packed || !bias_packed || !depth || !feat) return BEVOPS_BAD_PARAM;
  if (n < 0 || hw < 0 || Cin <= 0 || C <= 0 || D <= 0) return BEVOPS_BAD_PARAM;
  if (x_pitch < Cin || x_pitch % 8 != 0) return BEVOPS_BAD_PARAM;
  if (misaligned(x, 15u) || misaligned(w_packed, 15u) || misaligned(bias_packed, 15u) || misaligned(feat, 15u) ||
      misaligned(depth, 1u))
    return BEVOPS_BAD_PARAM;
  if (Cin % 32 != 0 || Cin > 512 || C % 8 != 0 || C > 128 || C + D > 256) return BEVOPS_NOT_SUPPORTED;
  const long long rows = (long long)n * hw;
  if (rows > 0x7fffffffLL) return BEVOPS_NOT_SUPPORTED;
  if (rows == 0) return BEVOPS_SUCCESS;
  DhArgs p;
  p.x = static_cast<const __half *>(x); p.w = static_cast<const i32x4_t *>(w_packed);
  p.bias = static_cast<const float *>(bias_packed);
  p.depth = static_cast<__half *>(depth); p.feat = static_cast<__half *>(feat);
  p.rows = rows; p.hw = hw; p.x_pitch = x_pitch; p.nks = Cin / 16; p.C = C; p.D = D; p.nt = (C + D + 31) / 32;
  const dim3 grid((unsigned)((rows + kDhRows - 1) / kDhRows));
  if (p.nt <= 4)
    hipLaunchKernelGGL((depth_head_kernel<1, 8>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  else
    hipLaunchKernelGGL((depth_head_kernel<2, 4>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}
