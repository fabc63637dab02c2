// Implicit-GEMM 3-D convolution on CHANNEL SLICES of channels-last fp16 VOLUMES (bevops_conv3d_slice_f16; the layers of
// BEVDet-Occ's CustomResNet3D / LSSFPN3D / final_conv, bevformer_tensorrt_amd/bevdet_occ3d.py, design/conv3d.md):
//     out[b, zo, yo, xo, co] = act( bias[co] + residual[b, zo, yo, xo, co]
//                                   + sum_{kz,ky,kx,ci} x[b, s zo + kz - k/2, s yo + ky - k/2, s xo + kx - k/2, ci] w[co, kz, ky, kx, ci] )
// with k in {1, 3} and s in {1, 2} on all three axes, act in {none, ReLU}; the identity is added IN FRONT OF the
// activation (BasicBlock3D: relu(conv2 + identity)).  x, residual and out each point at the first channel of a slice of a
// wider channels-last volume: element (b, z, y, x, c) lives at base + (((b Z + z) Y + y) X + x) pitch + c, as
// csrc/conv_slice.hip addresses its images.  x and out may be disjoint channel slices of ONE buffer: every load is 16 bytes
// inside the input slice, every store 16 bytes inside the output slice.
//
// On the 128-row tile skeleton of csrc/tile_mma.h: M = B Zo Yo Xo output voxels, N = Cout, K = k^3 Cin, 32 fp16 k-values
// (64 bytes) per step and row, v_mfma_f32_32x32x16_f16, 128 x 64 tiles for Cout <= 64.  No column buffer, no workspace.
// Its own:
//   * ROW DECODE.  A staging thread decodes its two rows into (b, z, y, x) once; the byte offset of the centre tap and the
//     three input coordinates stay in registers (a row past M keeps coordinates no tap can make valid).
//   * K-LOOP.  Tap-major in ONE fixed order, (kz, ky, kx) outer, the 32-channel chunks of Cin inner; Cin % 32 == 0, so a step
//     never straddles a tap.  The tap is block-uniform: its address delta ((dz Y + dy) X + dx) pitch is scalar arithmetic,
//     its validity three unsigned range checks per row.  A tap outside the volume is given the beyond-the-buffer address
//     kGemmOob and reads zero: it is never addressed (the delta is computed for it, hence the entry's displacement limit).
//   * NO TAP IS SKIPPED, not even the kz planes a whole tile has outside the volume (z = 0, z = Zo - 1): every output sees
//     the same k^3 Cin / 32 steps in the same order whichever tile it falls in.
// Epilogue through LDS as in the skeleton, a thread on 8 consecutive channels of one output voxel: bias and identity added in
// fp32, ReLU as v < 0 ? 0 : v (a NaN stays a NaN, as torch's relu), ONE rounding to fp16, one 16-byte store.
#include "tile_mma.h"

namespace bevops {
namespace {

struct Conv3dArgs {
  const void *x, *w, *bias, *res;
  void *out;
  int M, N, K, act, tiles_n, tiles_total;
  unsigned x_bytes, w_bytes;                   // extents of the input slice and the weight (the loads' range check)
  int x_pitch, res_pitch, out_pitch;           // elements between two voxels
  int cin, zin, yin, xin, zout, yout, xout, stride, ks;
};

// where a staging row stands: byte offset of its centre tap (this thread's 16-byte chunk) and the tap's input coordinates
struct Conv3dRow { unsigned off; int z, y, x; };

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64)
template <int NI>
__global__ __launch_bounds__(256, 3) void conv3d_slice_kernel(Conv3dArgs p) {
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
  const int cin = p.cin, ksz = p.ks, pad = ksz >> 1;
  const int Z = p.zin, Y = p.yin, X = p.xin;
  auto place = [&](int m) {
    Conv3dRow r;
    r.off = kGemmOob; r.z = r.y = r.x = -0x40000000;          // a row past M: no tap passes the range checks
    if (m >= M) return r;
    const int xo = m % p.xout, q1 = m / p.xout;
    const int yo = q1 % p.yout, q2 = q1 / p.yout;
    const int zo = q2 % p.zout, b = q2 / p.zout;
    r.z = zo * p.stride; r.y = yo * p.stride; r.x = xo * p.stride;           // centre tap in the input volume
    r.off = (unsigned)(((((size_t)b * Z + r.z) * Y + r.y) * X + r.x) * p.x_pitch + kce) * 2u;
    return r;
  };
  const Conv3dRow row0 = place(m0 + r0), row1 = place(m0 + r1);
  int g_k = 0, g_c = 0;                        // the k and the channel position of the NEXT load
  int g_dz = -pad, g_dy = -pad, g_dx = -pad;   // its tap, as displacements from the centre
  const unsigned w_off0 = n0 + r0 < N ? (unsigned)(((size_t)(n0 + r0) * K + kce) * 2) : kGemmOob;
  const unsigned w_off1 = (NI == 2 && n0 + r1 < N) ? (unsigned)(((size_t)(n0 + r1) * K + kce) * 2) : kGemmOob;
  auto load = [&](TileStage &s) {
    const bool kok = g_k < K;                  // steps past the last one read zero
    // modulo 2^32: exact for every real tap (the entry's displacement limit), any value for the steps past the last
    const unsigned delta = (unsigned)((g_dz * Y + g_dy) * X + g_dx) * (unsigned)(p.x_pitch * 2);
    auto addr = [&](const Conv3dRow &r) {
      const bool in = (unsigned)(r.z + g_dz) < (unsigned)Z && (unsigned)(r.y + g_dy) < (unsigned)Y &&
                      (unsigned)(r.x + g_dx) < (unsigned)X;
      return in && kok ? r.off + delta : kGemmOob;
    };
    s.a0 = bload(rs_a, addr(row0), g_c * 2);
    s.a1 = bload(rs_a, addr(row1), g_c * 2);
    g_c += kStepK;
    if (g_c >= cin) {                          // next tap: kx fastest, then ky, then kz
      g_c = 0;
      if (++g_dx > pad) {
        g_dx = -pad;
        if (++g_dy > pad) { g_dy = -pad; ++g_dz; }
      }
    }
    s.b0 = bload(rs_w, kok ? w_off0 : kGemmOob, g_k * 2);
    if constexpr (NI == 2) s.b1 = bload(rs_w, kok ? w_off1 : kGemmOob, g_k * 2);
    g_k += kStepK;
  };
  BEVOPS_TILE_K_LOOP(smem, t, f32x16_t, NI, K / kStepK, acc, load)
  const int ncol = t.epi_col<NI, 8>(n0);
  const bool col_ok = ncol < N;                // N % 8 == 0: the chunk is all in or all out
  const __half *res = static_cast<const __half *>(p.res);
  const int act = p.act;
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
    if (res) {                                 // the identity IN FRONT OF the activation
      const uint4 q = *reinterpret_cast<const uint4 *>(res + (size_t)m * p.res_pitch + ncol);
      v[0] += h2f_lo(q.x); v[1] += h2f_hi(q.x); v[2] += h2f_lo(q.y); v[3] += h2f_hi(q.y);
      v[4] += h2f_lo(q.z); v[5] += h2f_hi(q.z); v[6] += h2f_lo(q.w); v[7] += h2f_hi(q.w);
    }
    if (act == kActRelu) {
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = v[c] < 0.f ? 0.f : v[c];
    }
    uint4 o;
    o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
    *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + (size_t)m * p.out_pitch + ncol) = o;
  });
}

// a * b, saturated well above every limit the entry compares with (the factors are non-negative ints)
inline unsigned long long mul_sat(unsigned long long a, unsigned long long b) {
  constexpr unsigned long long kCap = 1ull << 40;
  return (b != 0 && a > kCap / b) ? kCap : a * b;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_conv3d_slice_f16(const void *x, int x_pitch, const void *weight_taps, const void *bias,
                                       const void *residual, int res_pitch, void *out, int out_pitch, int B, int Z, int Y,
                                       int X, int Cin, int Cout, int ksize, int stride, int act, void *stream) {
  if (!x || !weight_taps || !out || Z <= 0 || Y <= 0 || X <= 0 || Cin <= 0 || Cout <= 0 || B < 0) return BEVOPS_BAD_PARAM;
  if (x_pitch < Cin || out_pitch < Cout || (residual && res_pitch < Cout)) return BEVOPS_BAD_PARAM;
  // a pitch that is no multiple of 8 elements leaves every other voxel's vectors unaligned
  if (x_pitch % 8 != 0 || out_pitch % 8 != 0 || (residual && res_pitch % 8 != 0)) return BEVOPS_BAD_PARAM;
  if (misaligned(x, 15u) || misaligned(weight_taps, 15u) || (residual && misaligned(residual, 15u)) ||
      (bias && misaligned(bias, 15u)) || misaligned(out, 15u))
    return BEVOPS_BAD_PARAM;
  if (Cin % 32 != 0 || Cout % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || (act != kActNone && act != kActRelu)) return BEVOPS_NOT_SUPPORTED;
  // x and the weight are addressed through 32-bit buffer offsets (identity and output through 64-bit pointers)
  const unsigned long long rows_in = mul_sat(mul_sat(mul_sat((unsigned long long)B, Z), Y), X);
  const unsigned long long k_total = (unsigned long long)ksize * ksize * ksize * Cin;
  if (mul_sat(mul_sat(rows_in, x_pitch), 2) >= kGemmOob || mul_sat(mul_sat((unsigned long long)Cout, k_total), 2) >= kGemmOob)
    return BEVOPS_NOT_SUPPORTED;
  // the displacement of a tap is a signed 32-bit byte count, computed for taps outside the volume too
  if (mul_sat(mul_sat(mul_sat((unsigned long long)Y, X) + X + 1, x_pitch), 2) > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  const int pad = ksize / 2;
  Conv3dArgs p;
  p.x = x; p.w = weight_taps; p.bias = bias; p.res = residual; p.out = out;
  p.zin = Z; p.yin = Y; p.xin = X; p.cin = Cin; p.stride = stride; p.ks = ksize;
  p.zout = (Z + 2 * pad - ksize) / stride + 1;
  p.yout = (Y + 2 * pad - ksize) / stride + 1;
  p.xout = (X + 2 * pad - ksize) / stride + 1;
  const unsigned long long rows = (unsigned long long)B * p.zout * p.yout * p.xout;   // <= rows_in
  p.M = (int)rows; p.N = Cout; p.K = (int)k_total; p.act = act;
  p.x_pitch = x_pitch; p.res_pitch = residual ? res_pitch : 0; p.out_pitch = out_pitch;
  p.x_bytes = (unsigned)(((rows_in - 1) * x_pitch + Cin) * 2);       // the last voxel's slice ends here
  p.w_bytes = (unsigned)((size_t)Cout * k_total * 2);
  dim3 grid;
  if (!tile_grid(rows, Cout, 1, &p.tiles_n, &p.tiles_total, &grid)) return BEVOPS_NOT_SUPPORTED;
  if (Cout <= 64) hipLaunchKernelGGL(conv3d_slice_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(conv3d_slice_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}
