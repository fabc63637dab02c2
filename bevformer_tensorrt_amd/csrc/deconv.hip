// ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) + bias + ReLU on channels-last fp16 activations (the up-sampling
// layers of mmdet's CTResNetNeck; not a reference plugin -- TensorRT owns the layer there) as FOUR implicit GEMMs on the
// matrix cores, one per output parity (py, px):
//     out[b, 2y+py, 2x+px, co] = act( bias[co] + sum_{dy,dx in {0,1}} sum_ci
//                                     x[b, y-1+py+dy, x-1+px+dx, ci] * w[ci, co, 3-py-2dy, 3-px-2dx] )
// M = B H W input-pixel rows, K = 4 Cin ordered [dy][dx][Cin], N = Cout: every output pixel of a parity class has exactly
// four taps, so there is no zero-stuffed input, no column buffer and no multiply by a structural zero.  The weight is packed
// once per weight tensor into [parity 4][Cout][dy 2][dx 2][Cin] (bevops_deconv4x4s2_pack_weight): each parity class then
// is a row-major [Cout, K] GEMM operand.
//
// On the 128-row tile skeleton of csrc/tile_mma.h, 32 fp16 k-values per step.  Its own: the parity geometry.  Cin % 32 == 0,
// so a step never straddles a tap: a tap is a block-uniform address delta plus a per-row validity bit.
// Tile order: [row tile][parity][column tile], the skeleton's numbering with (row tile, parity) as its row: the blocks
// that read the same 128 input pixels (and their neighbours) run back to back on one XCD, so the activation rows come from
// HBM once and from that XCD's L2 afterwards.  These layers are memory-bound at batch 1 (the last one reads 1 MB and writes
// 2 MB for 0.13 GFLOP; design/centernet.md).
// Epilogue, a thread on 8 consecutive channels of one output pixel: bias and ReLU in fp32, ONE rounding to fp16, one
// 16-byte store; NaN and inf go through (ReLU: NaN -> 0).
#include "tile_mma.h"

namespace bevops {
namespace {

struct DeconvArgs {
  const void *x, *w, *bias;
  void *out;
  int M, N, K, relu, tiles_n, tiles_total;
  unsigned x_bytes, w_bytes;                   // sizes of the activation and packed-weight buffers (the loads' range check)
  int cin, h, wd;                              // input image [h, wd, cin]
};

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64)
template <int NI>
__global__ __launch_bounds__(256, 3) void deconv4x4s2_kernel(DeconvArgs p) {
  constexpr int kStepK = 32;                   // k-values per step
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  const int M = p.M, N = p.N, K = p.K;
  const TilePos t(p.tiles_total, p.tiles_n);    // [row tile][parity][column tile]: row_tile counts (row tile, parity)
  if (!t.valid) return;
  const int par = t.row_tile & 3, py = par >> 1, px = par & 1;
  const int m0 = (t.row_tile >> 2) * kTM, n0 = t.col * 64 * NI;
  const int r0 = t.r0, r1 = t.r1;
  const int kce = t.lchunk / 2;                // this thread's first k-value inside a step
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
    off = (unsigned)((((size_t)b * p.h + y) * p.wd + x) * cin + kce) * 2u;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
      const int yy = y - 1 + py + (tap >> 1), xx = x - 1 + px + (tap & 1);
      mk |= (yy >= 0 && yy < p.h && xx >= 0 && xx < p.wd) ? (1u << tap) : 0u;
    }
  };
  place(m0 + r0, a_off0, tapmask0);
  place(m0 + r1, a_off1, tapmask1);
  int g_k = 0, g_tap = 0, g_c = 0;             // the k and the (tap, channel) position of the NEXT load
  const size_t wrow = (size_t)par * N;         // first weight row of this parity class
  const unsigned w_off0 = n0 + r0 < N ? (unsigned)(((wrow + n0 + r0) * K + kce) * 2) : kGemmOob;
  const unsigned w_off1 = (NI == 2 && n0 + r1 < N) ? (unsigned)(((wrow + n0 + r1) * K + kce) * 2) : kGemmOob;
  auto load = [&](TileStage &s) {
    const bool kok = g_k < K;
    const int delta = (((g_tap >> 1) + py - 1) * p.wd + ((g_tap & 1) + px - 1)) * cin * 2;
    // (steps past the last one: g_tap >= 4, whose mask bits are clear)
    s.a0 = bload(rs_a, (tapmask0 >> g_tap) & 1u ? a_off0 + (unsigned)delta : kGemmOob, g_c * 2);
    s.a1 = bload(rs_a, (tapmask1 >> g_tap) & 1u ? a_off1 + (unsigned)delta : kGemmOob, g_c * 2);
    g_c += kStepK;
    if (g_c >= cin) { g_c = 0; ++g_tap; }
    s.b0 = bload(rs_w, kok ? w_off0 : kGemmOob, g_k * 2);
    if constexpr (NI == 2) s.b1 = bload(rs_w, kok ? w_off1 : kGemmOob, g_k * 2);
    g_k += kStepK;
  };
  BEVOPS_TILE_K_LOOP(smem, t, f32x16_t, NI, K / kStepK, acc, load)   // a multiple of 4 steps (K = 4 Cin, Cin % 32 == 0)
  const int ncol = t.epi_col<NI, 8>(n0);
  const bool col_ok = ncol < N;                // N % 8 == 0: the chunk is all in or all out
  float bs[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    bs[c] = (p.bias && col_ok) ? __half2float(static_cast<const __half *>(p.bias)[ncol + c]) : 0.f;
  tile_epilogue<NI, 8>(smem, t, acc, m0, M, col_ok, [&](int m, const f32x4 (&s)[2]) {
    float v[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = s[0][c] + bs[c];
      v[4 + c] = s[1][c] + bs[4 + c];
    }
    if (p.relu) {
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = fmaxf(v[c], 0.f);
    }
    const int b = m / per, pix = m - b * per;
    const int y = pix / p.wd, x = pix - y * p.wd;
    const size_t opix = ((size_t)b * (2 * p.h) + 2 * y + py) * (2 * p.wd) + 2 * x + px;
    uint4 o;
    o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
    *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + opix * N + ncol) = o;
  });
}

// packed[par][co][dy][dx][ci] = weight[ci][co][3 - py - 2 dy][3 - px - 2 dx], par = 2 py + px
__global__ void deconv4x4s2_pack_kernel(const __half *__restrict__ w, __half *__restrict__ packed, int cin, int cout) {
  const size_t total = (size_t)16 * cin * cout;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin);
    const int t = (int)(i / cin % 4), dy = t >> 1, dx = t & 1;
    const int co = (int)(i / (4 * (size_t)cin) % cout);
    const int par = (int)(i / (4 * (size_t)cin * cout)), py = par >> 1, px = par & 1;
    packed[i] = w[(((size_t)ci * cout + co) * 4 + (3 - py - 2 * dy)) * 4 + (3 - px - 2 * dx)];
  }
}

// the layer shapes both the pack and the forward entry take: BAD_PARAM, NOT_SUPPORTED or SUCCESS
int deconv_domain(int dtype, int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0) return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F16 || Cin % 32 != 0 || Cout % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  if (gemm_over_limit(4ull * Cout, 4 * Cin, 2)) return BEVOPS_NOT_SUPPORTED;   // the packed weight behind 32-bit offsets
  return BEVOPS_SUCCESS;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_deconv4x4s2_packed_weight_size(int dtype, int Cin, int Cout) {
  return deconv_domain(dtype, Cin, Cout) == BEVOPS_SUCCESS ? (size_t)16 * Cin * Cout * 2 : 0;
}

extern "C" int bevops_deconv4x4s2_pack_weight(int dtype, const void *weight, void *packed, int Cin, int Cout,
                                              void *stream) {
  if (!weight || !packed) return BEVOPS_BAD_PARAM;
  const int rc = deconv_domain(dtype, Cin, Cout);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(weight, 1u) || misaligned(packed, 15u)) return BEVOPS_BAD_PARAM;
  const size_t total = (size_t)16 * Cin * Cout;
  const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(deconv4x4s2_pack_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const __half *>(weight), static_cast<__half *>(packed), Cin, Cout);
  return launch_status();
}

extern "C" int bevops_deconv4x4s2_f16(int dtype, const void *x, const void *packed_weight, const void *bias, void *out,
                                      int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int relu,
                                      void *stream) {
  if (!x || !packed_weight || !out || B < 0 || H <= 0 || W <= 0) return BEVOPS_BAD_PARAM;
  if (ksize <= 0 || stride <= 0 || pad < 0) return BEVOPS_BAD_PARAM;
  if (ksize != 4 || stride != 2 || pad != 1) return BEVOPS_NOT_SUPPORTED;
  const int rc = deconv_domain(dtype, Cin, Cout);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(x, 15u) || misaligned(packed_weight, 15u) || misaligned(out, 15u) || (bias && misaligned(bias, 1u)))
    return BEVOPS_BAD_PARAM;
  // the activation is addressed through 32-bit buffer offsets (the output through 64-bit pointers)
  const unsigned long long rows = (unsigned long long)B * H * W;
  if (gemm_over_limit(rows, Cin, 2)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  DeconvArgs p;
  p.x = x; p.w = packed_weight; p.bias = bias; p.out = out;
  p.M = (int)rows; p.N = Cout; p.K = 4 * Cin; p.relu = relu;
  p.x_bytes = (unsigned)(rows * Cin * 2);
  p.w_bytes = (unsigned)((size_t)16 * Cin * Cout * 2);
  p.cin = Cin; p.h = H; p.wd = W;
  dim3 grid;
  if (!tile_grid(rows, Cout, 4, &p.tiles_n, &p.tiles_total, &grid)) return BEVOPS_NOT_SUPPORTED;
  if (Cout <= 64) hipLaunchKernelGGL(deconv4x4s2_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(deconv4x4s2_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}
