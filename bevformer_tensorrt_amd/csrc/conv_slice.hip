// Implicit-GEMM convolution on CHANNEL SLICES of channels-last fp16 tensors, the activation in the epilogue
// (bevops_conv_slice_f16; the convolutions of YOLOX's CSPDarknet / PAFPN / head, bevformer_tensorrt_amd/yolox.py):
//     out[b, yo, xo, co] = act( bias[co] + sum_{ky,kx,ci} x[b, s yo + ky - k/2, s xo + kx - k/2, ci] w[co, ky, kx, ci] )
//                          + residual[b, yo, xo, co]
// with k in {1, 3}, s in {1, 2}, act in {none, ReLU, SiLU}; the identity is added AFTER the activation (mmdet's
// DarknetBottleneck), which no other entry of this library does.  x, residual and out each point at the first channel
// of a slice of a wider channels-last tensor: element (b, y, x, c) lives at base + ((b H + y) W + x) pitch + c.  A layer
// can therefore read one operand of a concatenation and write its own share of the next one: CSPLayer, SPPBottleneck
// and the PAFPN need no torch.cat.  x and out may be disjoint channel slices of ONE buffer: every load is 16 bytes
// inside the input slice, every store 16 bytes inside the output slice.
//
// On the 128-row tile skeleton of csrc/tile_mma.h, 32 fp16 k-values per step.  Its own: pitched rows; Cin % 32 == 0, so a
// step never straddles a tap and a tap is a block-uniform address delta plus a per-row validity bit.  The k-order and the
// MFMA sequence are bevops_conv_tile_f16's, so with pitch == channels, no identity and act in {0, 1} the two entries give
// equal bits (tests/test_conv_slice_gpu.py).
// Epilogue, a thread on 8 consecutive channels of one output pixel: bias, activation and identity in fp32, ONE rounding to
// fp16, one 16-byte store.  SiLU is tile_mma.h's silu_f32: -0 for v < -88.7, v for v > 88; NaN and inf go through.
//
// bevops_conv_slice_f16_ex (the ASPP block of BEVDepth's DepthNet, design/bevdepth.md) adds two block-uniform runtime
// values to the same two kernels: a DILATION (3 x 3, stride 1: the tap's address delta and validity bit scale with it)
// and a PER-IMAGE bias (bias_pitch != 0: the epilogue reads the 8 bias values of every row's own image, since a row
// tile may hold pixels of several images).  With (1, 0) every output bit is the parent entry's, which forwards here.
// A tap that lies outside the image for every row of a tile is still multiplied (by zeros): not skipped.
#include "tile_mma.h"

namespace bevops {
namespace {

struct ConvSliceArgs {
  const void *x, *w, *bias, *res;
  void *out;
  int M, N, K, act, tiles_n, tiles_total;
  unsigned x_bytes, w_bytes;                   // extents of the input slice and the weight (the loads' range check)
  int x_pitch, res_pitch, out_pitch;           // elements between two pixels
  int cin, hin, win, hout, wout, stride, ks;
  int dil;                                     // tap (ky, kx) reads pixel (y + (ky - pad) dil, x + (kx - pad) dil)
  int bias_pitch;                              // 0: bias[co]; else the bias of output row m is bias[(m / per) bias_pitch + co]
};

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64)
template <int NI>
__global__ __launch_bounds__(256, 3) void conv_slice_kernel(ConvSliceArgs p) {
  constexpr int kStepK = 32;                   // k-values per step
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  const int M = p.M, N = p.N, K = p.K;
  const TilePos t(p.tiles_total, p.tiles_n);
  if (!t.valid) return;
  const int m0 = t.row_tile * kTM, n0 = t.col * 64 * NI;
  const int r0 = t.r0, r1 = t.r1;
  const int kce = t.lchunk / 2;                // this thread's first k-value inside a step
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
    off = (unsigned)((((size_t)b * p.hin + y) * p.win + x) * p.x_pitch + kce) * 2u;
    for (int tap = 0; tap < taps; ++tap) {
      const int yy = y + (tap / ksz - pad) * dil, xx = x + (tap % ksz - pad) * dil;
      mk |= (yy >= 0 && yy < p.hin && xx >= 0 && xx < p.win) ? (1u << tap) : 0u;
    }
  };
  place(m0 + r0, a_off0, tapmask0);
  place(m0 + r1, a_off1, tapmask1);
  int g_k = 0, g_tap = 0, g_c = 0;             // the k and the (tap, channel) position of the NEXT load
  const unsigned w_off0 = n0 + r0 < N ? (unsigned)(((size_t)(n0 + r0) * K + kce) * 2) : kGemmOob;
  const unsigned w_off1 = (NI == 2 && n0 + r1 < N) ? (unsigned)(((size_t)(n0 + r1) * K + kce) * 2) : kGemmOob;
  auto load = [&](TileStage &s) {
    const bool kok = g_k < K;
    const int delta = ((g_tap / ksz - pad) * p.win + (g_tap % ksz - pad)) * dil * p.x_pitch * 2;
    // (steps past the last one: g_tap >= taps, whose mask bits are clear)
    s.a0 = bload(rs_a, (tapmask0 >> g_tap) & 1u ? a_off0 + (unsigned)delta : kGemmOob, g_c * 2);
    s.a1 = bload(rs_a, (tapmask1 >> g_tap) & 1u ? a_off1 + (unsigned)delta : kGemmOob, g_c * 2);
    g_c += kStepK;
    if (g_c >= cin) { g_c = 0; ++g_tap; }
    s.b0 = bload(rs_w, kok ? w_off0 : kGemmOob, g_k * 2);
    if constexpr (NI == 2) s.b1 = bload(rs_w, kok ? w_off1 : kGemmOob, g_k * 2);
    g_k += kStepK;
  };
  BEVOPS_TILE_K_LOOP(smem, t, f32x16_t, NI, K / kStepK, acc, load)
  const int ncol = t.epi_col<NI, 8>(n0);
  const bool col_ok = ncol < N;                // N % 8 == 0: the chunk is all in or all out
  const __half *res = static_cast<const __half *>(p.res);
  const int act = p.act, bias_pitch = p.bias_pitch;
  float bs[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    bs[c] = (p.bias && col_ok) ? __half2float(static_cast<const __half *>(p.bias)[ncol + c]) : 0.f;
  tile_epilogue<NI, 8>(smem, t, acc, m0, M, col_ok, [&](int m, const f32x4 (&s)[2]) {
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (res) q = *reinterpret_cast<const uint4 *>(res + (size_t)m * p.res_pitch + ncol);
    if (bias_pitch) {                          // a per-image bias: the tile's rows may belong to several images
      const uint4 bq = *reinterpret_cast<const uint4 *>(static_cast<const __half *>(p.bias) +
                                                        (size_t)(m / per) * bias_pitch + ncol);
      bs[0] = h2f_lo(bq.x); bs[1] = h2f_hi(bq.x); bs[2] = h2f_lo(bq.y); bs[3] = h2f_hi(bq.y);
      bs[4] = h2f_lo(bq.z); bs[5] = h2f_hi(bq.z); bs[6] = h2f_lo(bq.w); bs[7] = h2f_hi(bq.w);
    }
    float v[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = s[0][c] + bs[c];
      v[4 + c] = s[1][c] + bs[4 + c];
    }
    if (act == kActRelu) {
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = fmaxf(v[c], 0.f);
    } else if (act == kActSilu) {
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = silu_f32(v[c]);
    }
    if (res) {                                 // the identity AFTER the activation
      v[0] += h2f_lo(q.x); v[1] += h2f_hi(q.x); v[2] += h2f_lo(q.y); v[3] += h2f_hi(q.y);
      v[4] += h2f_lo(q.z); v[5] += h2f_hi(q.z); v[6] += h2f_lo(q.w); v[7] += h2f_hi(q.w);
    }
    uint4 o;
    o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
    *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + (size_t)m * p.out_pitch + ncol) = o;
  });
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_conv_slice_f16_ex(const void *x, int x_pitch, const void *weight_taps, const void *bias,
                                        const void *residual, int res_pitch, void *out, int out_pitch, int B, int H, int W,
                                        int Cin, int Cout, int ksize, int stride, int act, int dilation, int bias_pitch,
                                        void *stream) {
  if (!x || !weight_taps || !out || B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return BEVOPS_BAD_PARAM;
  if (ksize <= 0 || stride <= 0 || dilation <= 0) return BEVOPS_BAD_PARAM;
  if (x_pitch < Cin || out_pitch < Cout || (residual && res_pitch < Cout)) return BEVOPS_BAD_PARAM;
  // a pitch that is no multiple of 8 elements leaves every other pixel's vectors unaligned
  if (x_pitch % 8 != 0 || out_pitch % 8 != 0 || (residual && res_pitch % 8 != 0)) return BEVOPS_BAD_PARAM;
  if (misaligned(x, 15u) || misaligned(weight_taps, 15u) || misaligned(out, 15u) || (residual && misaligned(residual, 15u)) ||
      (bias && misaligned(bias, 1u)))
    return BEVOPS_BAD_PARAM;
  // a per-image bias: rows of bias_pitch halves, each read as 16-byte vectors
  if (bias_pitch != 0 && (!bias || bias_pitch < Cout || bias_pitch % 8 != 0 || misaligned(bias, 15u))) return BEVOPS_BAD_PARAM;
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || act < kActNone || act > kActSilu) return BEVOPS_NOT_SUPPORTED;
  if (Cin % 32 != 0 || Cout % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  if (dilation > 1 && (ksize != 3 || stride != 1)) return BEVOPS_NOT_SUPPORTED;
  // x and the weight are addressed through 32-bit buffer offsets (identity and output through 64-bit pointers)
  const unsigned long long rows_in = (unsigned long long)B * H * W;
  if (gemm_over_limit(rows_in, x_pitch, 2) || gemm_over_limit((unsigned long long)Cout, ksize * ksize * Cin, 2))
    return BEVOPS_NOT_SUPPORTED;
  // the displacement of a tap is a signed 32-bit byte count, computed for taps outside the image too
  if (dilation > 1 && (unsigned long long)dilation * ((unsigned long long)W + 1) * (unsigned long long)x_pitch * 2 > 0x7fffffffull)
    return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  const int pad = ksize / 2;                   // at stride 1 a dilated 3 x 3 with pad = dilation keeps the size too
  ConvSliceArgs p;
  p.x = x; p.w = weight_taps; p.bias = bias; p.res = residual; p.out = out;
  p.hin = H; p.win = W; p.cin = Cin; p.stride = stride; p.ks = ksize;
  p.dil = dilation; p.bias_pitch = bias_pitch;
  p.hout = (H + 2 * pad - ksize) / stride + 1;
  p.wout = (W + 2 * pad - ksize) / stride + 1;
  const unsigned long long rows = (unsigned long long)B * p.hout * p.wout;
  p.M = (int)rows; p.N = Cout; p.K = ksize * ksize * Cin; p.act = act;
  p.x_pitch = x_pitch; p.res_pitch = residual ? res_pitch : 0; p.out_pitch = out_pitch;
  p.x_bytes = (unsigned)(((rows_in - 1) * x_pitch + Cin) * 2);      // the last pixel's slice ends here
  p.w_bytes = (unsigned)((size_t)Cout * p.K * 2);
  dim3 grid;
  if (!tile_grid(rows, Cout, 1, &p.tiles_n, &p.tiles_total, &grid)) return BEVOPS_NOT_SUPPORTED;
  if (Cout <= 64) hipLaunchKernelGGL(conv_slice_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(conv_slice_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}

extern "C" int bevops_conv_slice_f16(const void *x, int x_pitch, const void *weight_taps, const void *bias,
                                     const void *residual, int res_pitch, void *out, int out_pitch, int B, int H, int W,
                                     int Cin, int Cout, int ksize, int stride, int act, void *stream) {
  return bevops_conv_slice_f16_ex(x, x_pitch, weight_taps, bias, residual, res_pitch, out, out_pitch, B, H, W, Cin, Cout,
                                  ksize, stride, act, 1, 0, stream);
}
