// A whole depthwise-separable layer in ONE launch on CHANNEL SLICES of channels-last fp16 tensors
// (bevops_dwsep_conv_f16; mmcv's DepthwiseSeparableConvModule with the BatchNorms folded, the 3 x 3 layers of a YOLOX
// built with use_depthwise: bevformer_tensorrt_amd/yolox.py, design/yolox_depthwise.md):
//     t[b, yo, xo, c]    = fp16( act_dw( bias_dw[c] + sum_{ky,kx} x[b, s yo + ky - 1, s xo + kx - 1, c] w_dw[ky, kx, c] ) )
//     out[b, yo, xo, co] = fp16( act_pw( bias_pw[co] + sum_c t[b, yo, xo, c] w_pw[co, c] ) + residual[b, yo, xo, co] )
// s in {1, 2}, pad 1, act in {none, ReLU, SiLU}, the identity BEHIND the activation; the addressing contract is
// bevops_conv_slice_f16's (base pointer of the slice, pitch in elements, 16-byte vectors inside their own slice).
//
// t never exists in memory.  The launch is a pointwise GEMM on the 128-row tile skeleton of csrc/tile_mma.h
// (M = B Hout Wout pixels, N = Cout, K = Cin, 32 k-values per step) whose activation operand is not loaded but
// PRODUCED: the skeleton asks a thread, per step, for one 16-byte chunk (8 channels) of tile rows r0 and r0 + 64; here
// the thread computes these 2 x 8 values of t from 2 x 9 input vectors, 9 depthwise weight vectors and one bias vector
// and hands them over as that chunk.  The skeleton writes the chunk into the LDS image that the MFMAs of the current
// step do not read (two images, one barrier per step) and brings the pointwise weight rows as conv_slice.hip's: so the
// depthwise tile of chunk k + 1 is produced while chunk k is multiplied, LDS holds two 128 x 32 depthwise tiles
// whatever Cin is, and Cin has no ceiling but the 32-bit offset rule.
//
// The depthwise stage, per channel, in fp32 and in THIS order:
//     a = bias_dw[c] (0 without one);  for ky = 0, 1, 2: for kx = 0, 1, 2:  a = fma(x[tap], w_dw[ky, kx, c], a)
// one fused multiply-add per tap INSIDE the image; a tap outside it is skipped (a select on the row's tap mask, so a
// non-finite weight of a tap that does not exist never reaches the sum) and its load is given the beyond-the-buffer
// offset: its position is never turned into an address.  Then act_dw in fp32 (tile_mma.h's silu_f32) and ONE rounding to
// fp16 (v_cvt_pk_f16_f32, RNE).  These bits are the B operand of v_mfma_f32_32x32x16_f16, so the launch computes what
// two launches with an fp16 tensor between them compute.
//
// Column tiles (Cout > 128) RECOMPUTE the depthwise tile: tiles of one row tile run back to back on one XCD, the
// second reads x from that XCD's L2.  design/yolox_depthwise.md weighs this against one block sweeping the columns.
// Epilogue: conv_slice.hip's (bias, activation and identity in fp32, ONE rounding, one 16-byte store per thread).
#include "tile_mma.h"

namespace bevops {
namespace {

struct DwsepArgs {
  const void *x, *w_dw, *bias_dw, *w_pw, *bias_pw, *res;
  void *out;
  int M, N, K, act_dw, act_pw, tiles_n, tiles_total;
  unsigned x_bytes, w_bytes;                   // extents of the input slice and the pointwise weight
  int x_pitch, res_pitch, out_pitch;           // elements between two pixels
  int hin, win, hout, wout, stride;
};

__device__ __forceinline__ void unpack8(const uint4 &q, float (&v)[8]) {
  v[0] = h2f_lo(q.x); v[1] = h2f_hi(q.x); v[2] = h2f_lo(q.y); v[3] = h2f_hi(q.y);
  v[4] = h2f_lo(q.z); v[5] = h2f_hi(q.z); v[6] = h2f_lo(q.w); v[7] = h2f_hi(q.w);
}

__device__ __forceinline__ void act8(float (&v)[8], int act) {
  if (act == kActRelu) {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = fmaxf(v[c], 0.f);
  } else if (act == kActSilu) {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = silu_f32(v[c]);
  }
}

__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
  uint4 o;
  o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
  return o;
}

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64)
template <int NI>
__global__ __launch_bounds__(256, 2) void dwsep_conv_kernel(DwsepArgs p) {
  constexpr int kStepK = 32;                   // channels per chunk: the skeleton's 64 bytes of k per row
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  const int M = p.M, N = p.N, K = p.K;
  const TilePos t(p.tiles_total, p.tiles_n);
  if (!t.valid) return;
  const int m0 = t.row_tile * kTM, n0 = t.col * 64 * NI;
  const int r0 = t.r0, r1 = t.r1;
  const int kce = t.lchunk / 2;                // this thread's first channel inside a chunk
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.x), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w_pw), 0, p.w_bytes, 0x00020000);
  // tile row m is output pixel (b, yo, xo): the byte offset of its centre tap (s yo, s xo) at this thread's channels and
  // one bit per tap (ky, kx) that lies inside the image; a row past M has no bit set
  const int per = p.hout * p.wout;
  unsigned x_off0, x_off1, tapmask0, tapmask1;
  auto place = [&](int m, unsigned &off, unsigned &mk) {
    off = kGemmOob; mk = 0;
    if (m >= M) return;
    const int b = m / per, pix = m - b * per;
    const int yo = pix / p.wout, xo = pix - yo * p.wout;
    const int y = yo * p.stride, x = xo * p.stride;
    off = (unsigned)((((size_t)b * p.hin + y) * p.win + x) * p.x_pitch + kce) * 2u;
    for (int tap = 0; tap < 9; ++tap) {
      const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
      mk |= (yy >= 0 && yy < p.hin && xx >= 0 && xx < p.win) ? (1u << tap) : 0u;
    }
  };
  place(m0 + r0, x_off0, tapmask0);
  place(m0 + r1, x_off1, tapmask1);
  const __half *w_dw = static_cast<const __half *>(p.w_dw) + kce;
  const __half *b_dw = p.bias_dw ? static_cast<const __half *>(p.bias_dw) + kce : nullptr;
  const int act_dw = p.act_dw;
  int g_k = 0;                                 // first channel of the NEXT chunk
  const unsigned w_off0 = n0 + r0 < N ? (unsigned)(((size_t)(n0 + r0) * K + kce) * 2) : kGemmOob;
  const unsigned w_off1 = (NI == 2 && n0 + r1 < N) ? (unsigned)(((size_t)(n0 + r1) * K + kce) * 2) : kGemmOob;
  auto load = [&](TileStage &s) {
    const bool kok = g_k < K;                  // block-uniform: the skeleton asks for chunks past the last one too
    s.a0 = make_uint4(0u, 0u, 0u, 0u);
    s.a1 = make_uint4(0u, 0u, 0u, 0u);
    if (kok) {                                 // the depthwise producer: 8 channels of rows r0 and r1
      float a0[8], a1[8], xv[8], wv[8];
      if (b_dw) {
        unpack8(*reinterpret_cast<const uint4 *>(b_dw + g_k), a0);
#pragma unroll
        for (int c = 0; c < 8; ++c) a1[c] = a0[c];
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) a0[c] = a1[c] = 0.f;
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {      // ky-major, kx-minor
        // (modulo 2^32: the sum with the centre's offset is exact for a tap inside the image, the only one that uses it)
        const unsigned delta = (unsigned)((tap / 3 - 1) * p.win + (tap % 3 - 1)) * ((unsigned)p.x_pitch * 2u);
        const bool in0 = (tapmask0 >> tap) & 1u, in1 = (tapmask1 >> tap) & 1u;
        const uint4 q0 = bload(rs_x, in0 ? x_off0 + delta : kGemmOob, g_k * 2);
        const uint4 q1 = bload(rs_x, in1 ? x_off1 + delta : kGemmOob, g_k * 2);
        unpack8(*reinterpret_cast<const uint4 *>(w_dw + (size_t)tap * K + g_k), wv);
        unpack8(q0, xv);
#pragma unroll
        for (int c = 0; c < 8; ++c) a0[c] = in0 ? __builtin_fmaf(xv[c], wv[c], a0[c]) : a0[c];
        unpack8(q1, xv);
#pragma unroll
        for (int c = 0; c < 8; ++c) a1[c] = in1 ? __builtin_fmaf(xv[c], wv[c], a1[c]) : a1[c];
      }
      act8(a0, act_dw);
      act8(a1, act_dw);
      s.a0 = pack8(a0);                        // the ONE rounding of t
      s.a1 = pack8(a1);
    }
    s.b0 = bload(rs_w, kok ? w_off0 : kGemmOob, g_k * 2);
    if constexpr (NI == 2) s.b1 = bload(rs_w, kok ? w_off1 : kGemmOob, g_k * 2);
    g_k += kStepK;
  };
  BEVOPS_TILE_K_LOOP(smem, t, f32x16_t, NI, K / kStepK, acc, load)
  const int ncol = t.epi_col<NI, 8>(n0);
  const bool col_ok = ncol < N;                // N % 8 == 0: the chunk is all in or all out
  const __half *res = static_cast<const __half *>(p.res);
  const int act_pw = p.act_pw;
  float bs[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    bs[c] = (p.bias_pw && col_ok) ? __half2float(static_cast<const __half *>(p.bias_pw)[ncol + c]) : 0.f;
  tile_epilogue<NI, 8>(smem, t, acc, m0, M, col_ok, [&](int m, const f32x4 (&s)[2]) {
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (res) q = *reinterpret_cast<const uint4 *>(res + (size_t)m * p.res_pitch + ncol);
    float v[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = s[0][c] + bs[c];
      v[4 + c] = s[1][c] + bs[4 + c];
    }
    act8(v, act_pw);
    if (res) {                                 // the identity AFTER the activation
      float r[8];
      unpack8(q, r);
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] += r[c];
    }
    *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + (size_t)m * p.out_pitch + ncol) = pack8(v);
  });
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_dwsep_conv_f16(const void *x, int x_pitch, const void *w_dw_taps, const void *bias_dw,
                                     const void *w_pw, const void *bias_pw, const void *residual, int res_pitch, void *out,
                                     int out_pitch, int B, int H, int W, int Cin, int Cout, int stride, int act_dw, int act_pw,
                                     void *stream) {
  if (!x || !w_dw_taps || !w_pw || !out || B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || stride <= 0)
    return BEVOPS_BAD_PARAM;
  if (x_pitch < Cin || out_pitch < Cout || (residual && res_pitch < Cout)) return BEVOPS_BAD_PARAM;
  if (x_pitch % 8 != 0 || out_pitch % 8 != 0 || (residual && res_pitch % 8 != 0)) return BEVOPS_BAD_PARAM;
  // bias_dw is read as 16-byte vectors beside the depthwise weight's; bias_pw element by element
  if (misaligned(x, 15u) || misaligned(w_dw_taps, 15u) || misaligned(w_pw, 15u) || misaligned(out, 15u) ||
      (residual && misaligned(residual, 15u)) || (bias_dw && misaligned(bias_dw, 15u)) || (bias_pw && misaligned(bias_pw, 1u)))
    return BEVOPS_BAD_PARAM;
  if (Cin % 32 != 0 || Cout % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  if (stride > 2 || act_dw < kActNone || act_dw > kActSilu || act_pw < kActNone || act_pw > kActSilu) return BEVOPS_NOT_SUPPORTED;
  // x and the pointwise weight are addressed through 32-bit buffer offsets (identity and output through 64-bit pointers)
  const unsigned long long rows_in = (unsigned long long)B * H * W;
  if (gemm_over_limit(rows_in, x_pitch, 2) || gemm_over_limit((unsigned long long)Cout, Cin, 2)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  DwsepArgs p;
  p.x = x; p.w_dw = w_dw_taps; p.bias_dw = bias_dw; p.w_pw = w_pw; p.bias_pw = bias_pw; p.res = residual; p.out = out;
  p.hin = H; p.win = W; p.stride = stride;
  p.hout = (H - 1) / stride + 1;
  p.wout = (W - 1) / stride + 1;
  const unsigned long long rows = (unsigned long long)B * p.hout * p.wout;
  p.M = (int)rows; p.N = Cout; p.K = Cin; p.act_dw = act_dw; p.act_pw = act_pw;
  p.x_pitch = x_pitch; p.res_pitch = residual ? res_pitch : 0; p.out_pitch = out_pitch;
  p.x_bytes = (unsigned)(((rows_in - 1) * x_pitch + Cin) * 2);      // the last pixel's slice ends here
  p.w_bytes = (unsigned)((size_t)Cout * Cin * 2);
  dim3 grid;
  if (!tile_grid(rows, Cout, 1, &p.tiles_n, &p.tiles_total, &grid)) return BEVOPS_NOT_SUPPORTED;
  if (Cout <= 64) hipLaunchKernelGGL(dwsep_conv_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(dwsep_conv_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}
