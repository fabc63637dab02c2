// Implicit-GEMM convolution on CHANNEL SLICES of channels-last INT8 tensors (bevops_conv_slice_s8): the int8 sibling of
// bevops_conv_slice_f16 (csrc/conv_slice.hip) for the INT8 build of YOLOX (quantization.build_int8_yolox).
// Operands: x int8 (real = q scale_a), weights int8 taps-major [Cout][k][k][Cin] (real = q scale_w w_scales[co]), bias
// fp32, identity int8 with its own scale, output int8 requantised with the consumer's scale or fp16.  k in {1, 3},
// stride in {1, 2}, x / residual / out point at the first channel of a slice: element (b, y, x, c) at
// base + ((b H + y) W + x) pitch + c, pitches in elements.
//
// EPILOGUE OPERATION ORDER (every step one fp32 operation, written as explicit fma / separate operations, so that the
// result does not depend on the compiler's contraction choice; include/bevops.h repeats it):
//   s_aw  = scale_a * scale_w                        on the host, one fp32 rounding
//   inv   = 1.f / scale_out                          on the host, one fp32 rounding
//   sc    = s_aw * w_scales[co]                      one rounding (sc = s_aw without w_scales)
//   v     = fma((float)sum, sc, bias[co])            sum: the exact int32 sum; (float): round to nearest even, exact
//                                                    for |sum| <= 2^24; ONE rounding for multiply and add
//   v     = act(v)                                   0 none, 1 max(v, 0), 2 v * rcp(1 + exp(-v)) (silu_f32 of
//                                                    tile_mma.h: hardware exponential and reciprocal)
//   v     = fma((float)res_q, scale_res, v)          with an identity only: BEHIND the activation, ONE rounding
//                                                    (bevops_conv_slice_s8_ex with res_first = 1: this step moves IN
//                                                    FRONT of the activation -- mmdet's BasicBlock, relu(conv2 + identity))
//   int8:   q = clamp(rne(v * inv), -127, 127)       one rounding for the product, v_rndne_f32, max, min
//   fp16:   one rounding of v to binary16
// bevops_conv_slice_s8_ex2 adds two block-uniform runtime values to the same four kernels (the ASPP block of the INT8
// build of BEVDepth's DepthNet; the siblings of conv_slice.hip's _ex):
//   dilation d: tap (ky, kx) reads input pixel (y + (ky - pad) d, x + (kx - pad) d): the validity bit in place() and the
//     per-thread delta in gload scale with d (the host passes d x_pitch); nothing else of the k-chunk scheme changes.
//   a PER-IMAGE bias, fp16 [B][image_bias_pitch], in place of bias: the thread that owns the 16 (8) channels of output
//     row m loads them from image m / (Hout Wout) -- per ROW, a 128-row tile can hold pixels of several images -- and
//     v = fma((float)sum, sc, (float)image_bias[b][co]); everything behind it is unchanged.
// bevops_conv_slice_s8_ex forwards with (1, no image bias) and keeps its bits.
// Non-finite values: a NaN v leaves as -127 (max(NaN, -127) = -127), +inf as 127, -inf as -127 (as SiLU: NaN ->
// -127); as fp16 they go through as they are.  With ReLU a NaN becomes 0 before the requantisation.
//
// On the 128-row tile skeleton of csrc/tile_mma.h, on the int8 matrix cores: 64 k-values per step.  Its own: the k-chunk
// scheme below, and a thread of the epilogue owns 16 (int8 out) or 8 (fp16 out) consecutive channels of one pixel.
//
// K-CHUNK SCHEME.  Cin % 32 == 0, not 64: a 64-byte step can straddle a tap (Cin 32, 96, 160) and the last step can
// be half empty (K = 9 * 96 = 13.5 steps).  A thread moves ONE 16-byte chunk per row and step; chunk j of step t holds
// k = 64 t + 16 j .. + 15.  16 divides Cin, so a chunk never straddles a tap, and the thread derives its own
// (tap, channel) = (k / Cin, k % Cin) -- kept incrementally: channel += 64 per step, at most two wraps since
// Cin >= 32.  The tap's address delta and its validity bit (bit `tap` of the row's 9-bit mask) are therefore per
// thread, not block-uniform.  k >= K means tap >= k^2, whose mask bits are clear: the activation chunk reads zero.
// The weight's range check is on the whole buffer, so a chunk behind a row's end would read the next row: its offset is
// replaced by the beyond-the-buffer address when k >= K.  Both operands of a chunk past K are zero.
// All of an address goes into the buffer load's VGPR offset (the scalar offset takes no part in the range check).
#include "tile_mma.h"

namespace bevops {
namespace {

struct ConvSliceS8Args {
  const void *x, *w, *res;
  const float *bias, *wscale;
  const __half *ibias;                         // per-image bias [B][ibias_pitch] (fp16), or nullptr
  void *out;
  int M, N, K, act, res_first, tiles_n, tiles_total;
  unsigned x_bytes, w_bytes;                   // extents of the input slice and the weight (the loads' range check)
  int x_pitch, res_pitch, out_pitch;           // elements (= bytes for the int8 operands) between two pixels
  int cin, hin, win, hout, wout, stride, ks;
  int dil, dpitch, ibias_pitch;                // dilation, dilation * x_pitch; halves between two images' bias rows
  float s_aw, s_res, inv_s_out;
};

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64); OUT8: int8 output
template <int NI, bool OUT8>
__global__ __launch_bounds__(256, 3) void conv_slice_s8_kernel(ConvSliceS8Args p) {
  constexpr int kStepK = 64;                   // k-values (bytes) per step
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  const int M = p.M, N = p.N, K = p.K;
  const TilePos t(p.tiles_total, p.tiles_n);
  if (!t.valid) return;
  const int m0 = t.row_tile * kTM, n0 = t.col * 64 * NI;
  const int r0 = t.r0, r1 = t.r1, lchunk = t.lchunk;   // lchunk: this thread's chunk, byte position in a step too
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.x), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w), 0, p.w_bytes, 0x00020000);
  // output row m is pixel (b, yo, xo); its k-values are [tap][Cin] with tap (ky, kx) read from input pixel
  // (s yo + (ky - pad) dil, s xo + (kx - pad) dil) of the same image, zero outside it (dil > 1: ksize 3, stride 1)
  const int cin = p.cin, ksz = p.ks, taps = ksz * ksz, pad = ksz >> 1, dil = p.dil;
  const int per = p.hout * p.wout;
  unsigned a_off0, a_off1, tapmask0, tapmask1;
  auto place = [&](int m, unsigned &off, unsigned &mk) {
    off = kGemmOob; mk = 0;
    if (m >= M) return;
    const int b = m / per, pix = m - b * per;
    const int yo = pix / p.wout, xo = pix - yo * p.wout;
    const int y = yo * p.stride, x = xo * p.stride;           // centre tap in the input image
    off = (unsigned)((((size_t)b * p.hin + y) * p.win + x) * p.x_pitch);
    for (int tap = 0; tap < taps; ++tap) {
      const int yy = y + (tap / ksz - pad) * dil, xx = x + (tap % ksz - pad) * dil;
      mk |= (yy >= 0 && yy < p.hin && xx >= 0 && xx < p.win) ? (1u << tap) : 0u;
    }
  };
  place(m0 + r0, a_off0, tapmask0);
  place(m0 + r1, a_off1, tapmask1);
  // the position of this thread's chunk in the NEXT load: global k, and (tap = (ty, tx), channel) = (k / Cin, k % Cin)
  int g_k = lchunk, g_c = lchunk, g_tap = 0, g_ty = 0, g_tx = 0;
  const bool w_ok0 = n0 + r0 < N, w_ok1 = NI == 2 && n0 + r1 < N;
  const unsigned w_row0 = (unsigned)((size_t)(n0 + r0) * K), w_row1 = (unsigned)((size_t)(n0 + r1) * K);
  auto wrap = [&]() {                          // one tap further when the channel left the tap
    if (g_c >= cin) {
      g_c -= cin; ++g_tap;
      if (++g_tx == ksz) { g_tx = 0; ++g_ty; }
    }
  };
  auto load = [&](TileStage &s) {
    wrap(); wrap();                            // 64 k-values further: at most two taps, Cin >= 32
    // (chunks past K: g_tap >= taps, whose mask bits are clear; g_tap stays below 32 -- at most five steps past K)
    // (in unsigned arithmetic: for a valid tap |.| <= dil (W + 1) x_pitch, which the entry keeps inside 31 bits, and the
    // sum with a_off is the tap's offset modulo 2^32; chunks past K and invalid taps compute a value too, of any size,
    // and drop it)
    const unsigned delta = ((unsigned)(g_ty - pad) * (unsigned)p.win + (unsigned)(g_tx - pad)) * (unsigned)p.dpitch +
                           (unsigned)g_c;
    s.a0 = bload(rs_a, (tapmask0 >> g_tap) & 1u ? a_off0 + delta : kGemmOob);
    s.a1 = bload(rs_a, (tapmask1 >> g_tap) & 1u ? a_off1 + delta : kGemmOob);
    const bool kok = g_k < K;                  // K % 16 == 0: the chunk is all in or all out
    s.b0 = bload(rs_w, (kok && w_ok0) ? w_row0 + (unsigned)g_k : kGemmOob);
    if constexpr (NI == 2) s.b1 = bload(rs_w, (kok && w_ok1) ? w_row1 + (unsigned)g_k : kGemmOob);
    g_k += kStepK; g_c += kStepK;
  };
  BEVOPS_TILE_K_LOOP(smem, t, i32x16_t, NI, (K + kStepK - 1) / kStepK, acc, load)
  // ---- epilogue, the transpose of tile_mma.h's tile_epilogue STATED HERE: through the template the int8 epilogue compiles
  // to 50 - 120 more instructions and the short 1 x 1 layers lose 0.2 us (design/dense.md).
  // acc[i][j][4 g + c]: n = n0 + wn*32*NI + i*32 + 8 g + 4 (lane >> 5) + c, m = m0 + wm*64 + j*32 + (lane & 31)
  // (the barrier that ended the last step also freed both LDS images)
  const int lane = t.lane, wave = t.wave, wm = t.wm, wn = t.wn;
  constexpr int kCW = OUT8 ? 16 : 8;           // consecutive channels a thread owns: one 16-byte store
  constexpr int kCH = 32 * NI / kCW;           // chunks per row of the wave's 32 NI columns
  constexpr int kRows = 64 / kCH;              // staged rows per read-back pass
  constexpr int kIT = 32 / kRows;              // passes over the wave's 32 staged rows
  const int cc = lane & (kCH - 1);
  const int ncol = n0 + wn * 32 * NI + cc * kCW;
  const bool col_ok = ncol < N;                // N % kCW == 0: the chunk is all in or all out
  char *stage = smem + wave * 32 * kEpiStride;
  const signed char *res = static_cast<const signed char *>(p.res);
  const int act = p.act;
  const bool res_front = res && p.res_first, res_behind = res && !p.res_first;   // block-uniform
  const __half *ibias = p.ibias;               // block-uniform
  float sc[kCW], bs[kCW];
#pragma unroll
  for (int c = 0; c < kCW; ++c) {
    sc[c] = (p.wscale && col_ok) ? p.s_aw * p.wscale[ncol + c] : p.s_aw;
    bs[c] = (p.bias && col_ok) ? p.bias[ncol + c] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < kTMJ; ++j) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<i32x4_t *>(stage + (lane & 31) * kEpiStride + (i * 32 + 8 * g + 4 * (lane >> 5)) * 4) =
            i32x4_t{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < kIT; ++it) {
      const int row = it * kRows + lane / kCH;
      const int m = m0 + wm * 32 * kTMJ + j * 32 + row;
      i32x4_t s[kCW / 4];
#pragma unroll
      for (int q = 0; q < kCW / 4; ++q)
        s[q] = *reinterpret_cast<const i32x4_t *>(stage + row * kEpiStride + cc * kCW * 4 + q * 16);
      if (m >= M || !col_ok) continue;
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
      if (ibias) {                             // a per-image bias: the tile's rows may belong to several images
        const uint4 *bp = reinterpret_cast<const uint4 *>(ibias + (size_t)(m / per) * p.ibias_pitch + ncol);
#pragma unroll
        for (int q = 0; q < kCW / 8; ++q) {
          const uint4 h = bp[q];
          const unsigned hw[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const int cq = 8 * q + c;
            v[cq] = __builtin_fmaf((float)s[cq >> 2][cq & 3], sc[cq], (c & 1) ? h2f_hi(hw[c >> 1]) : h2f_lo(hw[c >> 1]));
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < kCW; ++c) v[c] = __builtin_fmaf((float)s[c >> 2][c & 3], sc[c], bs[c]);
      }
      if (res_front) {                         // the identity IN FRONT of the activation (res_first)
#pragma unroll
        for (int c = 0; c < kCW; ++c) v[c] = __builtin_fmaf((float)s8_at(rq, c), p.s_res, v[c]);
      }
      if (act == kActRelu) {
#pragma unroll
        for (int c = 0; c < kCW; ++c) v[c] = fmaxf(v[c], 0.f);
      } else if (act == kActSilu) {
#pragma unroll
        for (int c = 0; c < kCW; ++c) v[c] = silu_f32(v[c]);
      }
      if (res_behind) {                        // the identity AFTER the activation
#pragma unroll
        for (int c = 0; c < kCW; ++c) v[c] = __builtin_fmaf((float)s8_at(rq, c), p.s_res, v[c]);
      }
      if constexpr (OUT8) {
        unsigned pk[4];
        requant_s8_pack(v, p.inv_s_out, pk);
        *reinterpret_cast<uint4 *>(static_cast<signed char *>(p.out) + (size_t)m * p.out_pitch + ncol) =
            make_uint4(pk[0], pk[1], pk[2], pk[3]);
      } else {
        uint4 o;
        o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
        *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + (size_t)m * p.out_pitch + ncol) = o;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_conv_slice_s8_ex2(const void *x_q, int x_pitch, float scale_a, const void *w_q_taps,
                                        const float *w_scales, float scale_w, const float *bias, const void *residual_q,
                                        int res_pitch, float scale_res, int out_dtype, void *out, int out_pitch,
                                        float scale_out, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                                        int act, int res_first, int dilation, const void *image_bias_f16,
                                        int image_bias_pitch, void *stream) {
  if (!x_q || !w_q_taps || !out || B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return BEVOPS_BAD_PARAM;
  if (ksize <= 0 || stride <= 0) return BEVOPS_BAD_PARAM;
  if (out_dtype != BEVOPS_I8 && out_dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  const bool out8 = out_dtype == BEVOPS_I8;
  if (x_pitch < Cin || out_pitch < Cout || (residual_q && res_pitch < Cout)) return BEVOPS_BAD_PARAM;
  // int8 slices: 16-byte vectors, so a pitch that is no multiple of 16 elements leaves every other pixel unaligned
  if (x_pitch % 16 != 0 || out_pitch % (out8 ? 16 : 8) != 0 || (residual_q && res_pitch % 16 != 0)) return BEVOPS_BAD_PARAM;
  if (misaligned(x_q, 15u) || misaligned(w_q_taps, 15u) || misaligned(out, 15u) ||
      (residual_q && misaligned(residual_q, 15u)) || (bias && misaligned(bias, 3u)) || (w_scales && misaligned(w_scales, 3u)))
    return BEVOPS_BAD_PARAM;
  if (bad_scale(scale_a) || bad_scale(scale_w) || (residual_q && bad_scale(scale_res)) || (out8 && bad_scale(scale_out)))
    return BEVOPS_BAD_PARAM;
  if (dilation < 1) return BEVOPS_BAD_PARAM;
  // a per-image bias: in place of bias; rows of image_bias_pitch halves, each read as 16-byte vectors
  if (image_bias_f16 && (bias || image_bias_pitch < Cout || image_bias_pitch % 8 != 0 || misaligned(image_bias_f16, 15u)))
    return BEVOPS_BAD_PARAM;
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || act < kActNone || act > kActSilu) return BEVOPS_NOT_SUPPORTED;
  if (Cin % 32 != 0 || Cout % (out8 ? 16 : 8) != 0) return BEVOPS_NOT_SUPPORTED;
  // the identity in front of the activation: of an identity, and not of SiLU (no layer of the models has it)
  if (res_first && (!residual_q || act == kActSilu)) return BEVOPS_NOT_SUPPORTED;
  // x and the weight are addressed through 32-bit buffer offsets (identity and output through 64-bit pointers)
  const unsigned long long rows_in = (unsigned long long)B * H * W;
  if (gemm_over_limit(rows_in, x_pitch, 1) || gemm_over_limit((unsigned long long)Cout, ksize * ksize * Cin, 1))
    return BEVOPS_NOT_SUPPORTED;
  if (dilation > 1 && (ksize != 3 || stride != 1)) return BEVOPS_NOT_SUPPORTED;
  // the displacement of a tap, computed for taps outside the image too, is a signed 32-bit byte count
  if (dilation > 1 && (unsigned long long)dilation * ((unsigned long long)W + 1) * (unsigned long long)x_pitch > 0x7fffffffull)
    return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  const int pad = ksize / 2;                   // at stride 1 a dilated 3 x 3 with pad = dilation keeps the size too
  ConvSliceS8Args p;
  p.x = x_q; p.w = w_q_taps; p.res = residual_q; p.bias = bias; p.wscale = w_scales; p.out = out;
  p.hin = H; p.win = W; p.cin = Cin; p.stride = stride; p.ks = ksize;
  p.dil = dilation; p.dpitch = dilation * x_pitch;
  p.ibias = static_cast<const __half *>(image_bias_f16); p.ibias_pitch = image_bias_f16 ? image_bias_pitch : 0;
  p.hout = (H + 2 * pad - ksize) / stride + 1;
  p.wout = (W + 2 * pad - ksize) / stride + 1;
  const unsigned long long rows = (unsigned long long)B * p.hout * p.wout;
  p.M = (int)rows; p.N = Cout; p.K = ksize * ksize * Cin; p.act = act; p.res_first = res_first ? 1 : 0;
  p.x_pitch = x_pitch; p.res_pitch = residual_q ? res_pitch : 0; p.out_pitch = out_pitch;
  p.x_bytes = (unsigned)((rows_in - 1) * x_pitch + Cin);            // the last pixel's slice ends here
  p.w_bytes = (unsigned)((size_t)Cout * p.K);
  p.s_aw = scale_a * scale_w;
  p.s_res = residual_q ? scale_res : 0.f;
  p.inv_s_out = out8 ? 1.f / scale_out : 1.f;
  dim3 grid;
  if (!tile_grid(rows, Cout, 1, &p.tiles_n, &p.tiles_total, &grid)) return BEVOPS_NOT_SUPPORTED;
  const bool narrow = Cout <= 64;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (out8) {
    if (narrow) hipLaunchKernelGGL((conv_slice_s8_kernel<1, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((conv_slice_s8_kernel<2, true>), grid, dim3(256), 0, st, p);
  } else {
    if (narrow) hipLaunchKernelGGL((conv_slice_s8_kernel<1, false>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((conv_slice_s8_kernel<2, false>), grid, dim3(256), 0, st, p);
  }
  return launch_status();
}

extern "C" int bevops_conv_slice_s8_ex(const void *x_q, int x_pitch, float scale_a, const void *w_q_taps,
                                       const float *w_scales, float scale_w, const float *bias, const void *residual_q,
                                       int res_pitch, float scale_res, int out_dtype, void *out, int out_pitch,
                                       float scale_out, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                                       int act, int res_first, void *stream) {
  return bevops_conv_slice_s8_ex2(x_q, x_pitch, scale_a, w_q_taps, w_scales, scale_w, bias, residual_q, res_pitch, scale_res,
                                  out_dtype, out, out_pitch, scale_out, B, H, W, Cin, Cout, ksize, stride, act, res_first, 1,
                                  nullptr, 0, stream);
}

extern "C" int bevops_conv_slice_s8(const void *x_q, int x_pitch, float scale_a, const void *w_q_taps,
                                    const float *w_scales, float scale_w, const float *bias, const void *residual_q,
                                    int res_pitch, float scale_res, int out_dtype, void *out, int out_pitch,
                                    float scale_out, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int act,
                                    void *stream) {
  return bevops_conv_slice_s8_ex(x_q, x_pitch, scale_a, w_q_taps, w_scales, scale_w, bias, residual_q, res_pitch, scale_res,
                                 out_dtype, out, out_pitch, scale_out, B, H, W, Cin, Cout, ksize, stride, act, 0, stream);
}
