// A whole depthwise-separable layer in ONE launch on CHANNEL SLICES of channels-last INT8 tensors
// (bevops_dwsep_conv_s8): the int8 sibling of bevops_dwsep_conv_f16 (csrc/dwsep_conv.hip) for the INT8 build of a YOLOX
// with use_depthwise (quantization.build_int8_yolox(depthwise="int8"), design/yolox_depthwise_int8.md).  What TensorRT's
// INT8 build of a DepthwiseSeparableConvModule computes -- both convolutions quantised, an int8 tensor t between them --
// with t living only in LDS:
//     sum_dw[b, yo, xo, c] = sum_{ky,kx} x_q[b, s yo + ky - 1, s xo + kx - 1, c] w_dw_q[ky, kx, c]            (int32, exact)
//     t[b, yo, xo, c]      = int8( act_dw( sum_dw scale_x w_dw_scales[c] + bias_dw[c] ) / scale_t )
//     sum[b, yo, xo, co]   = sum_c t[b, yo, xo, c] w_pw_q[co, c]                                            (int32, exact)
//     out                  = act_pw( sum scale_t w_pw_scales[co] + bias_pw[co] ) + res_q scale_res, int8 / scale_out or fp16
// s in {1, 2}, pad 1, acts in {none, ReLU, SiLU}, the identity BEHIND the second activation; the addressing contract is
// bevops_conv_slice_s8's (base pointer of the slice, pitch in elements = bytes, 16-byte vectors inside their own slice).
//
// OPERATION ORDER (every step one fp32 operation, written as explicit fma / separate operations, so that the bits do not
// depend on the compiler's contraction choice; include/bevops.h repeats it):
//   inv_t = 1.f / scale_t, inv_out = 1.f / scale_out, s_tw = scale_t * scale_w_pw       on the host, one rounding each
//   stage 1, per channel c:
//     sc = scale_x * w_dw_scales[c]                  one rounding
//     v  = fma((float)sum_dw, sc, bias_dw[c])        sum_dw exact, |sum_dw| <= 9 * 127 * 127: (float) is exact
//     v  = act_dw(v)                                 0 none, 1 max(v, 0), 2 silu_f32 of tile_mma.h
//     t  = clamp(rne(v * inv_t), -127, 127)          requant_s8_pack's steps
//   stage 2, per output channel co: bevops_conv_slice_s8's epilogue with scale_a := scale_t
//     sc = s_tw * w_pw_scales[co] (s_tw without them);  v = fma((float)sum, sc, bias_pw[co]);  v = act_pw(v);
//     v  = fma((float)res_q, scale_res, v)           with an identity only, BEHIND the activation
//     int8: q = clamp(rne(v * inv_out), -127, 127)   fp16: one rounding of v
// Non-finite values as conv_slice_s8.hip: a NaN v leaves as -127 (max(NaN, -127) = -127), +inf as 127, -inf as -127; with
// ReLU a NaN becomes 0 first.  A NaN in stage 1 therefore is t = -127 of its own channel: it reaches the sums through
// column c of w_pw alone.  As fp16 output non-finite values of stage 2 go through as they are.
//
// MAPPING.  The launch is the pointwise int8 GEMM on the 128-row tile skeleton of csrc/tile_mma.h (M = B Hout Wout,
// N = Cout, K = Cin, 64 k-bytes per step, v_mfma_i32_32x32x32_i8) whose activation operand is not loaded but PRODUCED:
// per step the skeleton asks a thread for one 16-byte chunk -- 16 channels -- of tile rows r0 and r0 + 64; the thread issues
// 2 x 9 range-checked 16-byte buffer loads of x (centre offset + a block-uniform tap displacement + its channel; a tap
// outside the image gets the beyond-the-buffer offset and reads zero: with integer weights that zero IS the border),
// 9 depthwise weight vectors, forms the 2 x 16 int32 sums (bytes unpacked by sign-extending bit-field extraction, one
// integer multiply-add per tap and channel), applies stage 1 and hands the packed bytes over.  The skeleton writes them
// into the LDS image the MFMAs of the current step do not read, so chunk k + 1 is produced while chunk k is multiplied;
// LDS is the skeleton's 40 960 bytes whatever Cin is.  No workspace, no atomics.
// Cin % 32 == 0, not 64: the last step can be half empty (Cin 32, 96, 160).  A chunk whose first channel is >= Cin -- and
// every chunk the skeleton requests past the last step -- is zeros with nothing loaded, and its pointwise weight chunk gets
// the beyond-the-buffer offset (its in-range address would be the NEXT weight row).  The test is per chunk (per thread).
// Column tiles (Cout > 128) RECOMPUTE the depthwise tile, as the fp16 kernel does (design/yolox_depthwise.md).
#include "tile_mma.h"

namespace bevops {
namespace {

struct DwsepS8Args {
  const void *x, *w_dw, *w_pw, *res;
  const float *ws_dw, *bias_dw, *ws_pw, *bias_pw;
  void *out;
  int M, N, K, act_dw, act_pw, tiles_n, tiles_total;
  unsigned x_bytes, w_bytes;                   // extents of the input slice and the pointwise weight
  int x_pitch, res_pitch, out_pitch;           // elements (= bytes for the int8 operands) between two pixels
  int hin, win, hout, wout, stride;
  float scale_x, inv_t, s_tw, s_res, inv_out;
};

template <int CW>
__device__ __forceinline__ void act_n(float (&v)[CW], int act) {
  if (act == kActRelu) {
#pragma unroll
    for (int c = 0; c < CW; ++c) v[c] = fmaxf(v[c], 0.f);
  } else if (act == kActSilu) {
#pragma unroll
    for (int c = 0; c < CW; ++c) v[c] = silu_f32(v[c]);
  }
}

// sum[c] += x[c] * w[c] over the 16 signed bytes of two vectors (sign-extending extraction, one integer multiply-add each)
__device__ __forceinline__ void mad16(const uint4 &xq, const int (&w)[16], int (&sum)[16]) {
  const unsigned xw[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
  for (int c = 0; c < 16; ++c) sum[c] += s8_at(xw, c) * w[c];
}

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64); OUT8: int8 output
template <int NI, bool OUT8>
__global__ __launch_bounds__(256, 2) void dwsep_conv_s8_kernel(DwsepS8Args p) {
  constexpr int kStepK = 64;                   // channels (bytes of k) per step
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  const int M = p.M, N = p.N, K = p.K;
  const TilePos t(p.tiles_total, p.tiles_n);
  if (!t.valid) return;
  const int m0 = t.row_tile * kTM, n0 = t.col * 64 * NI;
  const int r0 = t.r0, r1 = t.r1;
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.x), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w_pw), 0, p.w_bytes, 0x00020000);
  // tile row m is output pixel (b, yo, xo): the byte offset of its centre tap (s yo, s xo) and one bit per tap (ky, kx)
  // that lies inside the image; a row past M has no bit set
  const int per = p.hout * p.wout;
  unsigned x_off0, x_off1, tapmask0, tapmask1;
  auto place = [&](int m, unsigned &off, unsigned &mk) {
    off = kGemmOob; mk = 0;
    if (m >= M) return;
    const int b = m / per, pix = m - b * per;
    const int yo = pix / p.wout, xo = pix - yo * p.wout;
    const int y = yo * p.stride, x = xo * p.stride;
    off = (unsigned)((((size_t)b * p.hin + y) * p.win + x) * p.x_pitch);
    for (int tap = 0; tap < 9; ++tap) {
      const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
      mk |= (yy >= 0 && yy < p.hin && xx >= 0 && xx < p.win) ? (1u << tap) : 0u;
    }
  };
  place(m0 + r0, x_off0, tapmask0);
  place(m0 + r1, x_off1, tapmask1);
  const signed char *w_dw = static_cast<const signed char *>(p.w_dw);
  const int act_dw = p.act_dw;
  int g_k = t.lchunk;                          // first channel of this thread's chunk in the NEXT step
  const bool w_ok0 = n0 + r0 < N, w_ok1 = NI == 2 && n0 + r1 < N;
  const unsigned w_row0 = (unsigned)((size_t)(n0 + r0) * K), w_row1 = (unsigned)((size_t)(n0 + r1) * K);
  auto load = [&](TileStage &s) {
    const bool kok = g_k < K;                  // K % 16 == 0: the chunk is all in or all out; past the last step: out
    s.a0 = make_uint4(0u, 0u, 0u, 0u);
    s.a1 = make_uint4(0u, 0u, 0u, 0u);
    if (kok) {                                 // the depthwise producer: 16 channels of rows r0 and r1
      int s0[16], s1[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) s0[c] = s1[c] = 0;
#pragma unroll 1
      for (int ky = 0; ky < 3; ++ky) {         // both tap loops stay ROLLED: unrolled, the scheduler hoists every tap's loads
        // and unpacked bytes (fully: 256 VGPRs and 320 - 520 bytes of scratch; per tap row: 44 bytes at NI == 2); rolled,
        // 156 - 194 VGPRs and none.  The other blocks of the CU cover a tap's latency (design/yolox_depthwise_int8.md)
        const unsigned m0k = tapmask0 >> (3 * ky), m1k = tapmask1 >> (3 * ky);
        // (modulo 2^32: the sum with the centre's offset is exact for a tap inside the image, the only one that uses it)
        const unsigned drow = (unsigned)((ky - 1) * p.win) * (unsigned)p.x_pitch + (unsigned)g_k;
        const signed char *wk = w_dw + (size_t)(3 * ky) * K + g_k;
#pragma unroll 1
        for (int kx = 0; kx < 3; ++kx) {
          const unsigned delta = drow + (unsigned)(kx - 1) * (unsigned)p.x_pitch;
          const uint4 q0 = bload(rs_x, (m0k >> kx) & 1u ? x_off0 + delta : kGemmOob);
          const uint4 q1 = bload(rs_x, (m1k >> kx) & 1u ? x_off1 + delta : kGemmOob);
          const uint4 wq = *reinterpret_cast<const uint4 *>(wk + (size_t)kx * K);
          const unsigned ww[4] = {wq.x, wq.y, wq.z, wq.w};
          int w[16];
#pragma unroll
          for (int c = 0; c < 16; ++c) w[c] = s8_at(ww, c);
          mad16(q0, w, s0);
          mad16(q1, w, s1);
        }
      }
      const float4 *ws4 = reinterpret_cast<const float4 *>(p.ws_dw + g_k);
      const float4 *bs4 = p.bias_dw ? reinterpret_cast<const float4 *>(p.bias_dw + g_k) : nullptr;
      auto stage1 = [&](const int (&sum)[16]) {  // t: the bytes the matrix cores multiply
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {          // (scales and biases per row and quarter: 8 live registers, not 32)
          const float4 a = ws4[q];
          const float4 b = bs4 ? bs4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
          v[4 * q] = __builtin_fmaf((float)sum[4 * q], p.scale_x * a.x, b.x);
          v[4 * q + 1] = __builtin_fmaf((float)sum[4 * q + 1], p.scale_x * a.y, b.y);
          v[4 * q + 2] = __builtin_fmaf((float)sum[4 * q + 2], p.scale_x * a.z, b.z);
          v[4 * q + 3] = __builtin_fmaf((float)sum[4 * q + 3], p.scale_x * a.w, b.w);
        }
        act_n(v, act_dw);
        unsigned pk[4];
        requant_s8_pack(v, p.inv_t, pk);
        return make_uint4(pk[0], pk[1], pk[2], pk[3]);
      };
      s.a0 = stage1(s0);
      s.a1 = stage1(s1);
    }
    s.b0 = bload(rs_w, (kok && w_ok0) ? w_row0 + (unsigned)g_k : kGemmOob);
    if constexpr (NI == 2) s.b1 = bload(rs_w, (kok && w_ok1) ? w_row1 + (unsigned)g_k : kGemmOob);
    g_k += kStepK;
  };
  BEVOPS_TILE_K_LOOP(smem, t, i32x16_t, NI, (K + kStepK - 1) / kStepK, acc, load)
  // ---- stage 2: conv_slice_s8.hip's epilogue (identity behind the activation), a thread owns kCW consecutive channels
  constexpr int kCW = OUT8 ? 16 : 8;
  const int ncol = t.epi_col<NI, kCW>(n0);
  const bool col_ok = ncol < N;                // N % kCW == 0: the chunk is all in or all out
  const signed char *res = static_cast<const signed char *>(p.res);
  const int act_pw = p.act_pw;
  float sc[kCW], bs[kCW];
#pragma unroll
  for (int c = 0; c < kCW; ++c) {
    sc[c] = (p.ws_pw && col_ok) ? p.s_tw * p.ws_pw[ncol + c] : p.s_tw;
    bs[c] = (p.bias_pw && col_ok) ? p.bias_pw[ncol + c] : 0.f;
  }
  tile_epilogue<NI, kCW>(smem, t, acc, m0, M, col_ok, [&](int m, const i32x4_t (&s)[kCW / 4]) {
    unsigned rq[kCW / 4] = {};
    if (res) {
      if constexpr (OUT8) {
        const uint4 q = *reinterpret_cast<const uint4 *>(res + (size_t)m * p.res_pitch + ncol);
        rq[0] = q.x; rq[1] = q.y; rq[2] = q.z; rq[3] = q.w;
      } else {
        const uint2 q = *reinterpret_cast<const uint2 *>(res + (size_t)m * p.res_pitch + ncol);
        rq[0] = q.x; rq[1] = q.y;
      }
    }
    float v[kCW];
#pragma unroll
    for (int c = 0; c < kCW; ++c) v[c] = __builtin_fmaf((float)s[c >> 2][c & 3], sc[c], bs[c]);
    act_n(v, act_pw);
    if (res) {                                 // the identity AFTER the activation
#pragma unroll
      for (int c = 0; c < kCW; ++c) v[c] = __builtin_fmaf((float)s8_at(rq, c), p.s_res, v[c]);
    }
    if constexpr (OUT8) {
      unsigned pk[4];
      requant_s8_pack(v, p.inv_out, pk);
      *reinterpret_cast<uint4 *>(static_cast<signed char *>(p.out) + (size_t)m * p.out_pitch + ncol) =
          make_uint4(pk[0], pk[1], pk[2], pk[3]);
    } else {
      uint4 o;
      o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
      *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + (size_t)m * p.out_pitch + ncol) = o;
    }
  });
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_dwsep_conv_s8(const void *x_q, int x_pitch, float scale_x, const void *w_dw_q_taps,
                                    const float *w_dw_scales, const float *bias_dw, float scale_t, const void *w_pw_q,
                                    const float *w_pw_scales, float scale_w_pw, const float *bias_pw,
                                    const void *residual_q, int res_pitch, float scale_res, int out_dtype, void *out,
                                    int out_pitch, float scale_out, int B, int H, int W, int Cin, int Cout, int stride,
                                    int act_dw, int act_pw, void *stream) {
  if (!x_q || !w_dw_q_taps || !w_dw_scales || !w_pw_q || !out || B < 0 || H <= 0 || W <= 0 || Cin <= 0 ||
      Cout <= 0)
    return BEVOPS_BAD_PARAM;
  if (stride <= 0) return BEVOPS_BAD_PARAM;
  if (out_dtype != BEVOPS_I8 && out_dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  const bool out8 = out_dtype == BEVOPS_I8;
  if (x_pitch < Cin || out_pitch < Cout || (residual_q && res_pitch < Cout)) return BEVOPS_BAD_PARAM;
  if (x_pitch % 16 != 0 || out_pitch % (out8 ? 16 : 8) != 0 || (residual_q && res_pitch % 16 != 0)) return BEVOPS_BAD_PARAM;
  // w_dw_scales and bias_dw are read as 16-byte vectors beside the depthwise weight's; the pointwise ones element by element
  if (misaligned(x_q, 15u) || misaligned(w_dw_q_taps, 15u) || misaligned(w_pw_q, 15u) || misaligned(out, 15u) ||
      (residual_q && misaligned(residual_q, 15u)) || misaligned(w_dw_scales, 15u) || (bias_dw && misaligned(bias_dw, 15u)) ||
      (w_pw_scales && misaligned(w_pw_scales, 3u)) || (bias_pw && misaligned(bias_pw, 3u)))
    return BEVOPS_BAD_PARAM;
  if (bad_scale(scale_x) || bad_scale(scale_t) || bad_scale(scale_w_pw) || (residual_q && bad_scale(scale_res)) || (out8 && bad_scale(scale_out)))
    return BEVOPS_BAD_PARAM;
  if ((stride != 1 && stride != 2) || act_dw < kActNone || act_dw > kActSilu || act_pw < kActNone || act_pw > kActSilu)
    return BEVOPS_NOT_SUPPORTED;
  if (Cin % 32 != 0 || Cout % (out8 ? 16 : 8) != 0) return BEVOPS_NOT_SUPPORTED;
  // x and the pointwise weight are addressed through 32-bit buffer offsets (identity and output through 64-bit pointers)
  const unsigned long long rows_in = (unsigned long long)B * H * W;
  if (gemm_over_limit(rows_in, x_pitch, 1) || gemm_over_limit((unsigned long long)Cout, Cin, 1)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  DwsepS8Args p;
  p.x = x_q; p.w_dw = w_dw_q_taps; p.w_pw = w_pw_q; p.res = residual_q; p.out = out;
  p.ws_dw = w_dw_scales; p.bias_dw = bias_dw; p.ws_pw = w_pw_scales; p.bias_pw = bias_pw;
  p.hin = H; p.win = W; p.stride = stride;
  p.hout = (H - 1) / stride + 1;
  p.wout = (W - 1) / stride + 1;
  const unsigned long long rows = (unsigned long long)B * p.hout * p.wout;
  p.M = (int)rows; p.N = Cout; p.K = Cin; p.act_dw = act_dw; p.act_pw = act_pw;
  p.x_pitch = x_pitch; p.res_pitch = residual_q ? res_pitch : 0; p.out_pitch = out_pitch;
  p.x_bytes = (unsigned)((rows_in - 1) * x_pitch + Cin);            // the last pixel's slice ends here
  p.w_bytes = (unsigned)((size_t)Cout * Cin);
  p.scale_x = scale_x;
  p.inv_t = 1.f / scale_t;
  p.s_tw = scale_t * scale_w_pw;
  p.s_res = residual_q ? scale_res : 0.f;
  p.inv_out = out8 ? 1.f / scale_out : 1.f;
  dim3 grid;
  if (!tile_grid(rows, Cout, 1, &p.tiles_n, &p.tiles_total, &grid)) return BEVOPS_NOT_SUPPORTED;
  const bool narrow = Cout <= 64;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (out8) {
    if (narrow) hipLaunchKernelGGL((dwsep_conv_s8_kernel<1, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dwsep_conv_s8_kernel<2, true>), grid, dim3(256), 0, st, p);
  } else {
    if (narrow) hipLaunchKernelGGL((dwsep_conv_s8_kernel<1, false>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dwsep_conv_s8_kernel<2, false>), grid, dim3(256), 0, st, p);
  }
  return launch_status();
}
