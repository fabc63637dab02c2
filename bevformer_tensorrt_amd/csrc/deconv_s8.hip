// ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) + bias + ReLU on channels-last INT8 activations
// (bevops_deconv4x4s2_s8): the int8 sibling of bevops_deconv4x4s2_f16 (csrc/deconv.hip) for the INT8 build of CenterNet
// (quantization.build_int8_centernet; the up-sampling layers of mmdet's CTResNetNeck).  FOUR implicit GEMMs on the int8
// matrix cores, one per output parity (py, px):
//     sum[b, 2y+py, 2x+px, co] = sum_{dy,dx in {0,1}} sum_ci x_q[b, y-1+py+dy, x-1+px+dx, ci] * w_q[ci, co, 3-py-2dy, 3-px-2dx]
// M = B H W input-pixel rows, K = 4 Cin ordered [dy][dx][Cin], N = Cout, over the parity-major packed weight
// [parity 4][Cout][dy 2][dx 2][Cin] (functions/deconv.py: pack_deconv4x4s2, here int8): no column buffer, no zero-stuffed
// input, no multiply by a structural zero.
//
// EPILOGUE OPERATION ORDER: bevops_conv_slice_s8's (csrc/conv_slice_s8.hip), without an identity, every step one fp32
// operation written as explicit fma / separate operations (the compiler's contraction choice cannot matter):
//   s_aw  = scale_a * scale_w                        on the host, one fp32 rounding
//   inv   = 1.f / scale_out                          on the host, one fp32 rounding
//   sc    = s_aw * w_scales[co]                      one rounding (sc = s_aw without w_scales)
//   v     = fma((float)sum, sc, bias[co])            sum: the exact int32 sum; (float) exact for |sum| <= 2^24
//   v     = max(v, 0)                                with relu
//   int8:   q = clamp(rne(v * inv), -127, 127)       one rounding for the product, v_rndne_f32, max, min
//   fp16:   one rounding of v to binary16
// Non-finite values as bevops_conv_slice_s8: a NaN v leaves as -127, +inf as 127, -inf as -127 (int8); as fp16 they go
// through as they are; with ReLU a NaN becomes 0 before the requantisation.
//
// deconv.hip's geometry on conv_slice_s8.hip's operands, on the 128-row tile skeleton of csrc/tile_mma.h: 64 int8 k-values
// per step.  Cin % 64 == 0, so a step never straddles a tap: a tap is a block-uniform address delta plus a per-row
// validity bit.  All of an address goes into the buffer load's VGPR offset (the scalar offset takes no part in the range
// check).  Tile order [row tile][parity][column tile] as deconv.hip.  A thread of the epilogue owns 16 (int8 out) or 8
// (fp16 out) consecutive channels of one output pixel and stores them as one 16-byte vector.
#include "tile_mma.h"

namespace bevops {
namespace {

struct DeconvS8Args {
  const void *x, *w;
  const float *bias, *wscale;
  void *out;
  int M, N, K, relu, tiles_n, tiles_total;
  unsigned x_bytes, w_bytes;                   // sizes of the activation and packed-weight buffers (the loads' range check)
  int cin, h, wd;                              // input image [h, wd, cin]
  float s_aw, inv_s_out;
};

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64); OUT8: int8 output
template <int NI, bool OUT8>
__global__ __launch_bounds__(256, 3) void deconv4x4s2_s8_kernel(DeconvS8Args p) {
  constexpr int kStepK = 64;                   // k-values (bytes) per step
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  const int M = p.M, N = p.N, K = p.K;
  const TilePos t(p.tiles_total, p.tiles_n);    // [row tile][parity][column tile]: row_tile counts (row tile, parity)
  if (!t.valid) return;
  const int par = t.row_tile & 3, py = par >> 1, px = par & 1;
  const int m0 = (t.row_tile >> 2) * kTM, n0 = t.col * 64 * NI;
  const int r0 = t.r0, r1 = t.r1, lchunk = t.lchunk;   // lchunk: this thread's chunk, byte position in a step too
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.x), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w), 0, p.w_bytes, 0x00020000);
  // row m is input pixel (b, y, x); tap (dy, dx) of this block's parity reads pixel (y - 1 + py + dy, x - 1 + px + dx),
  // zero outside the image
  const int cin = p.cin, per = p.h * p.wd;
  unsigned a_off0, a_off1, tapmask0, tapmask1;
  auto place = [&](int m, unsigned &off, unsigned &mk) {
    off = kGemmOob; mk = 0;
    if (m >= M) return;
    const int b = m / per, pix = m - b * per;
    const int y = pix / p.wd, x = pix - y * p.wd;
    off = (unsigned)((((size_t)b * p.h + y) * p.wd + x) * cin + lchunk);
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
      const int yy = y - 1 + py + (tap >> 1), xx = x - 1 + px + (tap & 1);
      mk |= (yy >= 0 && yy < p.h && xx >= 0 && xx < p.wd) ? (1u << tap) : 0u;
    }
  };
  place(m0 + r0, a_off0, tapmask0);
  place(m0 + r1, a_off1, tapmask1);
  int g_tap = 0, g_c = 0, g_k = 0;             // the (tap, channel) position and the k of the NEXT load
  const size_t wrow = (size_t)par * N;         // first weight row of this parity class
  const bool w_ok0 = n0 + r0 < N, w_ok1 = NI == 2 && n0 + r1 < N;
  const unsigned w_off0 = (unsigned)((wrow + n0 + r0) * K + lchunk), w_off1 = (unsigned)((wrow + n0 + r1) * K + lchunk);
  auto load = [&](TileStage &s) {
    // (steps past the last one: g_tap >= 4, whose mask bits are clear; g_tap stays below 8 -- three steps past K)
    const unsigned delta = (unsigned)((((g_tap >> 1) + py - 1) * p.wd + ((g_tap & 1) + px - 1)) * cin + g_c);
    s.a0 = bload(rs_a, (tapmask0 >> g_tap) & 1u ? a_off0 + delta : kGemmOob);
    s.a1 = bload(rs_a, (tapmask1 >> g_tap) & 1u ? a_off1 + delta : kGemmOob);
    const bool kok = g_k < K;                  // a step behind a row's end would read the next row
    s.b0 = bload(rs_w, (kok && w_ok0) ? w_off0 + (unsigned)g_k : kGemmOob);
    if constexpr (NI == 2) s.b1 = bload(rs_w, (kok && w_ok1) ? w_off1 + (unsigned)g_k : kGemmOob);
    g_k += kStepK; g_c += kStepK;
    if (g_c >= cin) { g_c = 0; ++g_tap; }
  };
  BEVOPS_TILE_K_LOOP(smem, t, i32x16_t, NI, K / kStepK, acc, load)   // a multiple of 4 steps (K = 4 Cin, Cin % 64 == 0)
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
      float v[kCW];
#pragma unroll
      for (int c = 0; c < kCW; ++c) v[c] = __builtin_fmaf((float)s[c >> 2][c & 3], sc[c], bs[c]);
      if (p.relu) {
#pragma unroll
        for (int c = 0; c < kCW; ++c) v[c] = fmaxf(v[c], 0.f);
      }
      const int b = m / per, pix = m - b * per;
      const int y = pix / p.wd, x = pix - y * p.wd;
      const size_t opix = ((size_t)b * (2 * p.h) + 2 * y + py) * (2 * p.wd) + 2 * x + px;
      if constexpr (OUT8) {
        unsigned pk[4];
        requant_s8_pack(v, p.inv_s_out, pk);
        *reinterpret_cast<uint4 *>(static_cast<signed char *>(p.out) + opix * N + ncol) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      } else {
        uint4 o;
        o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
        *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + opix * N + ncol) = o;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_deconv4x4s2_s8(const void *x_q, float scale_a, const void *packed_w_q, const float *w_scales,
                                     float scale_w, const float *bias, int out_dtype, void *out, float scale_out, int B,
                                     int H, int W, int Cin, int Cout, int relu, void *stream) {
  if (!x_q || !packed_w_q || !out || B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return BEVOPS_BAD_PARAM;
  if (out_dtype != BEVOPS_I8 && out_dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  const bool out8 = out_dtype == BEVOPS_I8;
  if (misaligned(x_q, 15u) || misaligned(packed_w_q, 15u) || misaligned(out, 15u) || (bias && misaligned(bias, 3u)) ||
      (w_scales && misaligned(w_scales, 3u)))
    return BEVOPS_BAD_PARAM;
  if (bad_scale(scale_a) || bad_scale(scale_w) || (out8 && bad_scale(scale_out))) return BEVOPS_BAD_PARAM;
  if (Cin % 64 != 0 || Cout % (out8 ? 16 : 8) != 0) return BEVOPS_NOT_SUPPORTED;
  // the activation and the packed weight are addressed through 32-bit buffer offsets (the output through 64-bit pointers)
  const unsigned long long rows = (unsigned long long)B * H * W;
  if (gemm_over_limit(rows, Cin, 1) || gemm_over_limit(4ull * Cout, 4 * Cin, 1)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  DeconvS8Args p;
  p.x = x_q; p.w = packed_w_q; p.bias = bias; p.wscale = w_scales; p.out = out;
  p.M = (int)rows; p.N = Cout; p.K = 4 * Cin; p.relu = relu;
  p.x_bytes = (unsigned)(rows * Cin);
  p.w_bytes = (unsigned)((size_t)16 * Cin * Cout);
  p.cin = Cin; p.h = H; p.wd = W;
  p.s_aw = scale_a * scale_w;
  p.inv_s_out = out8 ? 1.f / scale_out : 1.f;
  dim3 grid;
  if (!tile_grid(rows, Cout, 4, &p.tiles_n, &p.tiles_total, &grid)) return BEVOPS_NOT_SUPPORTED;
  const bool narrow = Cout <= 64;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (out8) {
    if (narrow) hipLaunchKernelGGL((deconv4x4s2_s8_kernel<1, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((deconv4x4s2_s8_kernel<2, true>), grid, dim3(256), 0, st, p);
  } else {
    if (narrow) hipLaunchKernelGGL((deconv4x4s2_s8_kernel<1, false>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((deconv4x4s2_s8_kernel<2, false>), grid, dim3(256), 0, st, p);
  }
  return launch_status();
}
