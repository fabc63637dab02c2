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
// MI355X mapping: the skeleton of tile_gemm.hip's convolution mode, restated here for this geometry so that the kernels of
// that file keep their code.  128 x 128 output tiles (128 x 64 for Cout <= 64), 256 threads = 4 waves of 64 x 64 (64 x 32),
// v_mfma_f32_32x32x16_f16, 32 fp16 k-values per step and row; operands register-staged through range-checked buffer loads
// (rows past M / N and taps outside the image read as zero, no branches) in two register sets, written to the other of two
// LDS images while the current one is multiplied: one barrier per step.  Cin % 32 == 0, so a step never straddles a tap: a
// tap is a block-uniform address delta plus a per-row validity bit.  40 KB LDS and __launch_bounds__(256, 3): at least
// three blocks per CU (the compiler's 96 / 128 registers and the LDS allow four; design/centernet.md).
// Tile order: [row tile][parity][column tile], and the 8 XCDs take contiguous runs of that sequence (block b runs on XCD
// b % 8): the 4 * tiles_n blocks that read the same 128 input pixels (and their neighbours) run back to back on one XCD, so
// the activation rows come from HBM once and from that XCD's L2 afterwards.  These layers are memory-bound at batch 1
// (the last one reads 1 MB and writes 2 MB for 0.13 GFLOP).
// Epilogue: the raw sums go through LDS per wave (32 rows x 64 columns at a time) so that a thread owns 8 consecutive
// channels of one output pixel: bias and ReLU in fp32, ONE rounding to fp16, whole 16-byte channel vectors stored.
#include "gemm_host.h"

namespace bevops {
namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr int kTM = 128;                       // rows (input pixels) per tile
constexpr int kTLd = 64 + 16;                  // LDS row: the step's 64 bytes + 16 (conflict-free 16-byte fragment reads)
constexpr int kEpiStride = 64 * 4 + 16;        // staging row: 64 x 4 bytes + pad
constexpr int kLds = 2 * (kTM + 128) * kTLd;   // two images of [A rows | W rows]; the epilogue's 4 x 32 staging rows fit
static_assert(kLds >= 4 * 32 * kEpiStride, "epilogue staging must fit in the operand images");

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
  const int ct = logical % p.tiles_n, rp = logical / p.tiles_n;
  const int par = rp & 3, py = par >> 1, px = par & 1;
  const int m0 = (rp >> 2) * kTM, n0 = ct * kTN;
  const int r0 = tid >> 2, r1 = r0 + 64;       // 128 rows x 4 chunks of 16 bytes of k
  const int kce = (tid & 3) * 8;               // this thread's first k-value inside a step
  f32x16_t acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
  const int nk = K / kStepK;                   // a multiple of 4 (K = 4 Cin, Cin % 32 == 0)
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.x), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w), 0, p.w_bytes, 0x00020000);
  // row m is input pixel (b, y, x); tap t = (dy, dx) of this block's parity reads pixel (y - 1 + py + dy, x - 1 + px + dx),
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
    for (int t = 0; t < 4; ++t) {
      const int yy = y - 1 + py + (t >> 1), xx = x - 1 + px + (t & 1);
      mk |= (yy >= 0 && yy < p.h && xx >= 0 && xx < p.wd) ? (1u << t) : 0u;
    }
  };
  place(m0 + r0, a_off0, tapmask0);
  place(m0 + r1, a_off1, tapmask1);
  int g_tap = 0, g_c = 0;                      // the (tap, channel) position of the NEXT gload
  const size_t wrow = (size_t)par * N;         // first weight row of this parity class
  const unsigned w_off0 = n0 + r0 < N ? (unsigned)(((wrow + n0 + r0) * K + kce) * 2) : kGemmOob;
  const unsigned w_off1 = (NI == 2 && n0 + r1 < N) ? (unsigned)(((wrow + n0 + r1) * K + kce) * 2) : kGemmOob;
  uint4 ra0[2], ra1[2], rb0[2], rb1[2];        // two register sets (set = step parity): the loads of two steps in flight
  auto bload = [](const __amdgpu_buffer_rsrc_t &rs, unsigned voff, int soff) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, soff, 0));
  };
  auto gload = [&](int kt, auto setc) {
    constexpr int S = decltype(setc)::value;
    const int ks = kt * kStepK;
    const bool kok = ks < K;
    const int delta = (((g_tap >> 1) + py - 1) * p.wd + ((g_tap & 1) + px - 1)) * cin * 2;
    // (steps past the last one: g_tap >= 4, whose mask bits are clear)
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
  for (int kt = 0; kt < nk; kt += 2) {
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
      float v[8];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[c] = lo[c] + bs[c];
        v[4 + c] = hi[c] + bs[4 + c];
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
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
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
  const bool narrow = Cout <= 64;
  p.tiles_n = (Cout + (narrow ? 64 : 128) - 1) / (narrow ? 64 : 128);
  const long long tiles = 4ll * p.tiles_n * (long long)((rows + kTM - 1) / kTM);
  if (tiles > 0x3fffffffLL) return BEVOPS_NOT_SUPPORTED;
  p.tiles_total = (int)tiles;
  const dim3 grid((unsigned)((tiles + 7) / 8 * 8));
  if (narrow) hipLaunchKernelGGL(deconv4x4s2_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(deconv4x4s2_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return launch_status();
}
