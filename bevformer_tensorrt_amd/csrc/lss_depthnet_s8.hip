// The INT8 siblings of csrc/lss_depthnet.hip's two data-movement launches, for the INT8 build of BEVDepth's DepthNet
// (int8 channel slices as in csrc/conv_slice_s8.hip: 16-byte boundary, pitch a multiple of 16, real = q scale).  Neither
// allocates, synchronises or uses atomics; n == 0: BEVOPS_SUCCESS without a launch.
//
//  * se_gate2_nhwc_s8: both gated copies of an int8 slice, requantised with each output's own scale.  Thread = 16
//    channels of one pixel: x read once (16 bytes), two 16-byte stores.  Per value and output, every step ONE fp32
//    operation and none of them an addition, so nothing can be contracted into an fma (include/bevops.h repeats it):
//        t = (float)q * scale_x;   v = t * gate;   r = v * inv_out;   out = clamp(rne(r), -127, 127)
//    with inv_out = 1.f / scale_out computed once on the host.  A NaN (a NaN gate) leaves as -127: max(NaN, -127) = -127.
//  * global_avgpool_nhwc_s8: out[i, ch] = fp16(((float)sum * scale_x) / (float)hw), sum the EXACT int32 sum over the map
//    (hw <= 2^24: |sum| <= 127 * 2^24 < 2^31).  Integer partial sums: the result does not depend on the order or the
//    grid.  One block per image and 64 channels, 64 pixel lanes of 4 vectors of 16 channels; the lanes' partial sums meet
//    in LDS.  (float)sum rounds to nearest even (exact for |sum| <= 2^24), then one fp32 product, one IEEE division and
//    one rounding to binary16.
#include "common.h"
#include "gemm_host.h"

namespace bevops {
namespace {

__device__ __forceinline__ int s8_of(unsigned w, int c) { return (int)(w << (24 - 8 * c)) >> 24; }   // signed byte c

__device__ __forceinline__ unsigned requant4(const float t[4], const f32x4 g, float inv) {
  unsigned pk = 0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float r = (t[c] * g[c]) * inv;
    pk |= ((unsigned)(int)fminf(fmaxf(rintf(r), -127.f), 127.f) & 0xffu) << (8 * c);
  }
  return pk;
}

__global__ __launch_bounds__(256) void se_gate2_s8_kernel(const signed char *__restrict__ x, int x_pitch, float scale_x,
                                                          const float *__restrict__ gates, signed char *__restrict__ out_a,
                                                          int a_pitch, float inv_a, signed char *__restrict__ out_b,
                                                          int b_pitch, float inv_b, int n, int hw, int c) {
  const size_t cv = (size_t)c >> 4;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n * hw * cv) return;
  const size_t pix = i / cv;
  const int ch = (int)(i - pix * cv) * 16;
  const size_t img = pix / (size_t)hw;
  const uint4 v = *reinterpret_cast<const uint4 *>(x + pix * x_pitch + ch);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  const float *ga = gates + img * c + ch, *gb = ga + (size_t)n * c;
  unsigned oa[4], ob[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (float)s8_of(w[q], k) * scale_x;
    oa[q] = requant4(t, *reinterpret_cast<const f32x4 *>(ga + 4 * q), inv_a);
    ob[q] = requant4(t, *reinterpret_cast<const f32x4 *>(gb + 4 * q), inv_b);
  }
  *reinterpret_cast<uint4 *>(out_a + pix * a_pitch + ch) = make_uint4(oa[0], oa[1], oa[2], oa[3]);
  *reinterpret_cast<uint4 *>(out_b + pix * b_pitch + ch) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
}

constexpr int kPoolLanes = 64;               // pixel lanes of a block
constexpr int kPoolCh = 64;                  // channels of a block: 4 vectors of 16

__global__ __launch_bounds__(256) void global_avgpool_s8_kernel(const signed char *__restrict__ x, int x_pitch,
                                                                float scale_x, __half *__restrict__ out, int out_pitch,
                                                                int hw, int c, int chunks) {
  __shared__ int part[kPoolLanes][kPoolCh + 1];
  const int img = blockIdx.x / chunks, c0 = (blockIdx.x - img * chunks) * kPoolCh;
  const int lane = threadIdx.x >> 2, cl = (threadIdx.x & 3) * 16, ch = c0 + cl;
  int s[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = 0;
  if (ch < c) {                              // c % 16 == 0: the vector is all in or all out
    const signed char *src = x + (size_t)img * hw * x_pitch + ch;
    for (int p = lane; p < hw; p += kPoolLanes) {
      const uint4 v = *reinterpret_cast<const uint4 *>(src + (size_t)p * x_pitch);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) s[k] += s8_of(w[k >> 2], k & 3);
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) part[lane][cl + k] = s[k];
  __syncthreads();
  if (threadIdx.x < kPoolCh && c0 + (int)threadIdx.x < c) {
    int t = part[0][threadIdx.x];
    for (int l = 1; l < kPoolLanes; ++l) t += part[l][threadIdx.x];
    const float prod = (float)t * scale_x;
    out[(size_t)img * out_pitch + c0 + threadIdx.x] = __float2half_rn(prod / (float)hw);
  }
}

inline bool off16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
inline bool bad_pitch16(int pitch, int c) { return pitch < c || pitch % 16 != 0; }

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_se_gate2_nhwc_s8(const void *x_q, int x_pitch, float scale_x, const float *gates, void *out_a,
                                       int a_pitch, float scale_a, void *out_b, int b_pitch, float scale_b, int n, int hw,
                                       int c, void *stream) {
  if (!x_q || !gates || !out_a || !out_b || n < 0 || hw <= 0 || c <= 0) return BEVOPS_BAD_PARAM;
  if (bad_pitch16(x_pitch, c) || bad_pitch16(a_pitch, c) || bad_pitch16(b_pitch, c)) return BEVOPS_BAD_PARAM;
  if (off16(x_q) || off16(gates) || off16(out_a) || off16(out_b)) return BEVOPS_BAD_PARAM;
  if (bad_scale(scale_x) || bad_scale(scale_a) || bad_scale(scale_b)) return BEVOPS_BAD_PARAM;
  if (c % 16 != 0) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long nvec = (unsigned long long)n * hw * (c / 16);
  if ((nvec + 255) / 256 > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(se_gate2_s8_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const signed char *>(x_q), x_pitch, scale_x, gates,
                     static_cast<signed char *>(out_a), a_pitch, 1.f / scale_a, static_cast<signed char *>(out_b), b_pitch,
                     1.f / scale_b, n, hw, c);
  return launch_status();
}

extern "C" int bevops_global_avgpool_nhwc_s8(const void *x_q, int x_pitch, float scale_x, void *out, int out_pitch, int n,
                                             int hw, int c, void *stream) {
  if (!x_q || !out || n < 0 || hw <= 0 || c <= 0) return BEVOPS_BAD_PARAM;
  if (bad_pitch16(x_pitch, c) || out_pitch < c) return BEVOPS_BAD_PARAM;
  if (off16(x_q) || (reinterpret_cast<uintptr_t>(out) & 1u)) return BEVOPS_BAD_PARAM;
  if (bad_scale(scale_x)) return BEVOPS_BAD_PARAM;
  if (c % 16 != 0) return BEVOPS_NOT_SUPPORTED;
  if (hw > (1 << 24)) return BEVOPS_NOT_SUPPORTED;          // the int32 sum: 127 * 2^24 < 2^31
  const int chunks = (c + kPoolCh - 1) / kPoolCh;
  if ((unsigned long long)n * chunks > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(global_avgpool_s8_kernel, dim3((unsigned)(n * chunks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const signed char *>(x_q), x_pitch, scale_x, static_cast<__half *>(out), out_pitch, hw, c,
                     chunks);
  return launch_status();
}
