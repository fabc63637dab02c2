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
// MI355X mapping: the skeleton csrc/deconv.hip restated from the convolution mode of tile_gemm.hip, restated once more
// for pitched rows, so that the kernels of those files keep their code.  128 x 128 output tiles (128 x 64 for
// Cout <= 64), 256 threads = 4 waves of 64 x 64 (64 x 32), v_mfma_f32_32x32x16_f16, 32 fp16 k-values = 64 bytes per
// step and row; operands register-staged through range-checked buffer loads (rows past M / N and taps outside the
// image read as zero, no branches) in two register sets, written to the other of two LDS images while the current
// one is multiplied: one barrier per step.  Cin % 32 == 0, so a step never straddles a tap: a tap is a block-uniform
// address delta plus a per-row validity bit.  The k-order and the MFMA sequence are bevops_conv_tile_f16's, so with
// pitch == channels, no identity and act in {0, 1} the two entries give equal bits (tests/test_conv_slice_gpu.py).
// XCD-contiguous tile order ([row tile][column tile]; block b runs on XCD b % 8).
// Epilogue: the raw sums go through LDS per wave (32 rows x 64 columns at a time) so that a thread owns 8 consecutive
// channels of one output pixel: bias, activation and identity in fp32, ONE rounding to fp16, one 16-byte store.
// SiLU is v * sigmoid(v) = v * rcp(1 + exp(-v)) with the hardware exponential (v_exp_f32 on the scaled argument) and
// the hardware reciprocal (v_rcp_f32, 1 ulp): exp(-v) overflows to +inf for v < -88.7, where the result is -0 (the
// true value is below 2^-120); for v > 88 it is v.  design/yolox.md derives the error bound the tests assert.
//
// bevops_conv_slice_f16_ex (the ASPP block of BEVDepth's DepthNet, design/bevdepth.md) adds two block-uniform runtime
// values to the same two kernels: a DILATION (3 x 3, stride 1: the tap's address delta and validity bit scale with it)
// and a PER-IMAGE bias (bias_pitch != 0: the epilogue reads the 8 bias values of every row's own image, since a row
// tile may hold pixels of several images).  With (1, 0) every output bit is the parent entry's, which forwards here.
// A tap that lies outside the image for every row of a tile is still multiplied (by zeros): not skipped.
#include "gemm_host.h"

namespace bevops {
namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr int kTM = 128;                       // rows (output pixels) per tile
constexpr int kTLd = 64 + 16;                  // LDS row: the step's 64 bytes + 16 (conflict-free 16-byte fragment reads)
constexpr int kEpiStride = 64 * 4 + 16;        // staging row: 64 x 4 bytes + pad
constexpr int kLds = 2 * (kTM + 128) * kTLd;   // two images of [A rows | W rows]; the epilogue's 4 x 32 staging rows fit
static_assert(kLds >= 4 * 32 * kEpiStride, "epilogue staging must fit in the operand images");

enum { kActNone = 0, kActRelu = 1, kActSilu = 2 };

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

__device__ __forceinline__ float silu_f32(float v) { return v * __builtin_amdgcn_rcpf(1.f + __expf(-v)); }

// NI: 32-column MFMA blocks per wave: 2 -> 128-column tiles, 1 -> 64-column tiles (Cout <= 64)
template <int NI>
__global__ __launch_bounds__(256, 3) void conv_slice_kernel(ConvSliceArgs p) {
  constexpr int MJ = 2;                        // 32-row MFMA blocks per wave
  constexpr int kTN = 64 * NI;
  constexpr int kStepK = 32;                   // k-values per step
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  const int M = p.M, N = p.N, K = p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int per_xcd = (p.tiles_total + 7) >> 3;
  const int logical = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if (logical >= p.tiles_total) return;
  const int m0 = (logical / p.tiles_n) * kTM, n0 = (logical % p.tiles_n) * kTN;
  const int r0 = tid >> 2, r1 = r0 + 64;       // 128 rows x 4 chunks of 16 bytes of k
  const int kce = (tid & 3) * 8;               // this thread's first k-value inside a step
  f32x16_t acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
  const int nk = K / kStepK;
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
    for (int t = 0; t < taps; ++t) {
      const int yy = y + (t / ksz - pad) * dil, xx = x + (t % ksz - pad) * dil;
      mk |= (yy >= 0 && yy < p.hin && xx >= 0 && xx < p.win) ? (1u << t) : 0u;
    }
  };
  place(m0 + r0, a_off0, tapmask0);
  place(m0 + r1, a_off1, tapmask1);
  int g_tap = 0, g_c = 0;                      // the (tap, channel) position of the NEXT gload
  const unsigned w_off0 = n0 + r0 < N ? (unsigned)(((size_t)(n0 + r0) * K + kce) * 2) : kGemmOob;
  const unsigned w_off1 = (NI == 2 && n0 + r1 < N) ? (unsigned)(((size_t)(n0 + r1) * K + kce) * 2) : kGemmOob;
  uint4 ra0[2], ra1[2], rb0[2], rb1[2];        // two register sets (set = step parity): the loads of two steps in flight
  auto bload = [](const __amdgpu_buffer_rsrc_t &rs, unsigned voff, int soff) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, soff, 0));
  };
  auto gload = [&](int kt, auto setc) {
    constexpr int S = decltype(setc)::value;
    const int ks = kt * kStepK;
    const bool kok = ks < K;
    const int delta = ((g_tap / ksz - pad) * p.win + (g_tap % ksz - pad)) * dil * p.x_pitch * 2;
    // (steps past the last one: g_tap >= taps, whose mask bits are clear)
    ra0[S] = bload(rs_a, (tapmask0 >> g_tap) & 1u ? a_off0 + (unsigned)delta : kGemmOob, g_c * 2);
    ra1[S] = bload(rs_a, (tapmask1 >> g_tap) & 1u ? a_off1 + (unsigned)delta : kGemmOob, g_c * 2);
    g_c += kStepK;
    if (g_c >= cin) { g_c = 0; ++g_tap; }
    rb0[S] = bload(rs_w, kok ? w_off0 : kGemmOob, ks * 2);
    if constexpr (NI == 2) rb1[S] = bload(rs_w, kok ? w_off1 : kGemmOob, ks * 2);
  };
  const int lchunk = (tid & 3) * 16;           // byte position of the thread's chunk in an LDS row
  auto lstore = [&](int buf, auto setc) {
    constexpr int S = decltype(setc)::value;
    char *As = smem + buf * (kTM + 128) * kTLd, *Ws = As + kTM * kTLd;
    *reinterpret_cast<uint4 *>(As + r0 * kTLd + lchunk) = ra0[S];
    *reinterpret_cast<uint4 *>(As + r1 * kTLd + lchunk) = ra1[S];
    *reinterpret_cast<uint4 *>(Ws + r0 * kTLd + lchunk) = rb0[S];
    if constexpr (NI == 2) *reinterpret_cast<uint4 *>(Ws + r1 * kTLd + lchunk) = rb1[S];
  };
  auto compute = [&](int kt) {
    const char *As = smem + (kt & 1) * (kTM + 128) * kTLd, *Ws = As + kTM * kTLd;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kk = ks * 32 + (lane >> 5) * 16;
      // MFMA operand A = the weight rows (output channels n), B = the activation rows (m): a lane's 4 consecutive
      // accumulator rows are then 4 consecutive channels of one output pixel
      i32x4_t a[NI], b[MJ];
#pragma unroll
      for (int i = 0; i < NI; ++i)
        a[i] = *reinterpret_cast<const i32x4_t *>(Ws + (wn * 32 * NI + i * 32 + (lane & 31)) * kTLd + kk);
#pragma unroll
      for (int j = 0; j < MJ; ++j)
        b[j] = *reinterpret_cast<const i32x4_t *>(As + (wm * 32 * MJ + j * 32 + (lane & 31)) * kTLd + kk);
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a[i]),
                                                             __builtin_bit_cast(f16x8_t, b[j]), acc[i][j], 0, 0, 0);
    }
  };
  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, 1>;
  // (loads past the last step are issued too -- beyond-the-buffer addresses, they read as zero -- and so are the LDS writes
  // of a step that does not exist, into the image nobody reads: no branches, exact wait counts)
  gload(0, Set0{});
  lstore(0, Set0{});
  gload(1, Set1{});
  gload(2, Set0{});
  __syncthreads();
  auto step = [&](int kt, auto next_set) {
    lstore((kt + 1) & 1, next_set);
    gload(kt + 3, next_set);
    compute(kt);
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += 2) {         // (an odd step count runs one step on zeros: adds nothing)
    step(kt, Set1{});
    step(kt + 1, Set0{});
  }
  // ---- epilogue.  acc[i][j][4 g + c]: n = n0 + wn*32*NI + i*32 + 8 g + 4 (lane >> 5) + c,
  //                                     m = m0 + wm*64 + j*32 + (lane & 31)
  // (the barrier that ended the last step also freed both LDS images)
  constexpr int kCH = 4 * NI;                  // 8-column chunks per row of the wave's 32 NI columns
  constexpr int kIT = kCH / 2;                 // read-back passes over the wave's 32 staged rows (64 / kCH rows each)
  const int c8 = lane & (kCH - 1);
  const int ncol = n0 + wn * 32 * NI + c8 * 8;
  const bool col_ok = ncol < N;                // N % 8 == 0: the chunk is all in or all out
  char *stage = smem + wave * 32 * kEpiStride;
  const __half *res = static_cast<const __half *>(p.res);
  const int act = p.act, bias_pitch = p.bias_pitch;
  float bs[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    bs[c] = (p.bias && col_ok) ? __half2float(static_cast<const __half *>(p.bias)[ncol + c]) : 0.f;
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4 *>(stage + (lane & 31) * kEpiStride + (i * 32 + 8 * g + 4 * (lane >> 5)) * 4) =
            f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < kIT; ++it) {
      const int row = it * (64 / kCH) + lane / kCH;
      const int m = m0 + wm * 32 * MJ + j * 32 + row;
      const f32x4 lo = *reinterpret_cast<const f32x4 *>(stage + row * kEpiStride + c8 * 32);
      const f32x4 hi = *reinterpret_cast<const f32x4 *>(stage + row * kEpiStride + c8 * 32 + 16);
      if (m >= M || !col_ok) continue;
      uint4 q = make_uint4(0u, 0u, 0u, 0u);
      if (res) q = *reinterpret_cast<const uint4 *>(res + (size_t)m * p.res_pitch + ncol);
      if (bias_pitch) {                        // a per-image bias: the tile's rows may belong to several images
        const uint4 bq = *reinterpret_cast<const uint4 *>(static_cast<const __half *>(p.bias) +
                                                          (size_t)(m / per) * bias_pitch + ncol);
        bs[0] = h2f_lo(bq.x); bs[1] = h2f_hi(bq.x); bs[2] = h2f_lo(bq.y); bs[3] = h2f_hi(bq.y);
        bs[4] = h2f_lo(bq.z); bs[5] = h2f_hi(bq.z); bs[6] = h2f_lo(bq.w); bs[7] = h2f_hi(bq.w);
      }
      float v[8];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[c] = lo[c] + bs[c];
        v[4 + c] = hi[c] + bs[4 + c];
      }
      if (act == kActRelu) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = fmaxf(v[c], 0.f);
      } else if (act == kActSilu) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = silu_f32(v[c]);
      }
      if (res) {                               // the identity AFTER the activation
        v[0] += h2f_lo(q.x); v[1] += h2f_hi(q.x); v[2] += h2f_lo(q.y); v[3] += h2f_hi(q.y);
        v[4] += h2f_lo(q.z); v[5] += h2f_hi(q.z); v[6] += h2f_lo(q.w); v[7] += h2f_hi(q.w);
      }
      uint4 o;
      o.x = pack_h2(v[0], v[1]); o.y = pack_h2(v[2], v[3]); o.z = pack_h2(v[4], v[5]); o.w = pack_h2(v[6], v[7]);
      *reinterpret_cast<uint4 *>(static_cast<__half *>(p.out) + (size_t)m * p.out_pitch + ncol) = o;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
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
  const bool narrow = Cout <= 64;
  p.tiles_n = (Cout + (narrow ? 64 : 128) - 1) / (narrow ? 64 : 128);
  const long long tiles = (long long)p.tiles_n * (long long)((rows + kTM - 1) / kTM);
  if (tiles > 0x3fffffffLL) return BEVOPS_NOT_SUPPORTED;
  p.tiles_total = (int)tiles;
  const dim3 grid((unsigned)((tiles + 7) / 8 * 8));
  if (narrow) hipLaunchKernelGGL(conv_slice_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(conv_slice_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}

extern "C" int bevops_conv_slice_f16(const void *x, int x_pitch, const void *weight_taps, const void *bias,
                                     const void *residual, int res_pitch, void *out, int out_pitch, int B, int H, int W,
                                     int Cin, int Cout, int ksize, int stride, int act, void *stream) {
  return bevops_conv_slice_f16_ex(x, x_pitch, weight_taps, bias, residual, res_pitch, out, out_pitch, B, H, W, Cin, Cout,
                                  ksize, stride, act, 1, 0, stream);
}
