// The small layers of BEVDepth's DepthNet (LSSViewTransformerBEVDepth; bevformer_tensorrt_amd/bevdepth.py) that are no
// convolution (not reference plugins; TensorRT owns these layers there).  Three launches, none allocates, synchronises
// or uses atomics:
//
//  * lss_camera_gate: the camera-aware squeeze-excite gates.  Per camera and branch (0 depth, 1 context)
//        g = sigmoid(expand(relu(reduce(fc2(relu(fc1(bn(v))))))))      v: the camera's 27 calibration values
//    in fp32 throughout -- v holds focal lengths and principal points above 1000, where binary16 steps by 1.  The frozen
//    BatchNorm1d is folded into fc1 on the host (pack_camera_gate).  One block per (camera, branch); the vector of a
//    layer lives in LDS, thread j owns output j: acc = 0; for k ascending: acc = fma(w[k][j], in[k], acc); y = acc +
//    bias[j].  The packed weights are k-major ([k][mid]) so that the threads of a wave read consecutive words.
//  * se_gate2_nhwc: out_a = fp16(float(x) * gates[0][n][ch]), out_b = fp16(float(x) * gates[1][n][ch]); x read once,
//    thread = 8 channels of one pixel, one fp32 product and one rounding per value.
//  * global_avgpool_nhwc: out[n, ch] = fp16((sum_p float(x[n, p, ch])) / float(hw)).  One block per image and 64
//    channels, 32 pixel lanes: lane l adds pixels l, l + 32, l + 64, ... in ascending order into s_l (fp32); then
//    total = (((s_0 + s_1) + s_2) + ... + s_31), one IEEE division, one rounding.  The order is a function of
//    (hw, c) alone: two calls give equal bits.
#include "common.h"

namespace bevops {
namespace {

constexpr int kGateIn = 27;                  // calibration values per camera
constexpr int kGateMaxMid = 512;

// fp32 words of one branch's parameter block (include/bevops.h states the layout)
__host__ __device__ constexpr size_t gate_branch_words(int mid) { return (size_t)mid * (kGateIn + 1) + 3 * ((size_t)mid * mid + mid); }

// y[j] = act(sum_k w[k][j] in[k] + b[j]) for the block's threads' outputs j; in / out in LDS
template <bool RELU>
__device__ __forceinline__ void gate_layer(const float *__restrict__ w, const float *__restrict__ b, const float *in,
                                           float *out, int kdim, int mid) {
  for (int j = threadIdx.x; j < mid; j += blockDim.x) {
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < kdim; ++k) acc = fmaf(w[(size_t)k * mid + j], in[k], acc);
    acc = add_rn(acc, b[j]);
    out[j] = RELU ? fmaxf(acc, 0.f) : acc;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void lss_camera_gate_kernel(const float *__restrict__ mlp_input, int in_pitch,
                                                              const float *__restrict__ packed,
                                                              float *__restrict__ gates, int n, int mid) {
  __shared__ float va[kGateMaxMid], vb[kGateMaxMid];
  const int cam = blockIdx.x >> 1, branch = blockIdx.x & 1;
  const float *q = packed + (size_t)branch * gate_branch_words(mid);
  if (threadIdx.x < kGateIn) va[threadIdx.x] = mlp_input[(size_t)cam * in_pitch + threadIdx.x];
  __syncthreads();
  const size_t mm = (size_t)mid * mid;
  const float *w1 = q, *b1 = w1 + (size_t)kGateIn * mid;
  const float *w2 = b1 + mid, *b2 = w2 + mm;
  const float *wr = b2 + mid, *br = wr + mm;
  const float *we = br + mid, *be = we + mm;
  gate_layer<true>(w1, b1, va, vb, kGateIn, mid);       // relu(fc1(bn(v)))
  gate_layer<false>(w2, b2, vb, va, mid, mid);          // fc2
  gate_layer<true>(wr, br, va, vb, mid, mid);           // relu(conv_reduce)
  gate_layer<false>(we, be, vb, va, mid, mid);          // conv_expand
  float *dst = gates + ((size_t)branch * n + cam) * mid;
  for (int j = threadIdx.x; j < mid; j += blockDim.x) dst[j] = 1.f / (1.f + expf(-va[j]));
}

__global__ __launch_bounds__(256) void se_gate2_kernel(const __half *__restrict__ x, int x_pitch,
                                                       const float *__restrict__ gates, __half *__restrict__ out_a,
                                                       int a_pitch, __half *__restrict__ out_b, int b_pitch, int n, int hw,
                                                       int c) {
  const size_t cv = (size_t)c >> 3;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n * hw * cv) return;
  const size_t pix = i / cv;
  const int ch = (int)(i - pix * cv) * 8;
  const size_t img = pix / (size_t)hw;
  const uint4 v = *reinterpret_cast<const uint4 *>(x + pix * x_pitch + ch);
  const float f[8] = {h2f_lo(v.x), h2f_hi(v.x), h2f_lo(v.y), h2f_hi(v.y), h2f_lo(v.z), h2f_hi(v.z), h2f_lo(v.w), h2f_hi(v.w)};
  const float *ga = gates + img * c + ch, *gb = ga + (size_t)n * c;
  const f32x4 a0 = *reinterpret_cast<const f32x4 *>(ga), a1 = *reinterpret_cast<const f32x4 *>(ga + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4 *>(gb), b1 = *reinterpret_cast<const f32x4 *>(gb + 4);
  uint4 oa, ob;
  oa.x = pack_h2(f[0] * a0[0], f[1] * a0[1]); oa.y = pack_h2(f[2] * a0[2], f[3] * a0[3]);
  oa.z = pack_h2(f[4] * a1[0], f[5] * a1[1]); oa.w = pack_h2(f[6] * a1[2], f[7] * a1[3]);
  ob.x = pack_h2(f[0] * b0[0], f[1] * b0[1]); ob.y = pack_h2(f[2] * b0[2], f[3] * b0[3]);
  ob.z = pack_h2(f[4] * b1[0], f[5] * b1[1]); ob.w = pack_h2(f[6] * b1[2], f[7] * b1[3]);
  *reinterpret_cast<uint4 *>(out_a + pix * a_pitch + ch) = oa;
  *reinterpret_cast<uint4 *>(out_b + pix * b_pitch + ch) = ob;
}

constexpr int kPoolLanes = 32;               // pixel lanes of a block
constexpr int kPoolCh = 64;                  // channels of a block: 8 vectors of 8

__global__ __launch_bounds__(256) void global_avgpool_kernel(const __half *__restrict__ x, int x_pitch,
                                                             __half *__restrict__ out, int out_pitch, int hw, int c,
                                                             int chunks) {
  __shared__ float part[kPoolLanes][kPoolCh + 1];
  const int img = blockIdx.x / chunks, c0 = (blockIdx.x - img * chunks) * kPoolCh;
  const int lane = threadIdx.x >> 3, ch = c0 + (threadIdx.x & 7) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ch < c) {                              // c % 8 == 0: the vector is all in or all out
    const __half *src = x + (size_t)img * hw * x_pitch + ch;
    for (int p = lane; p < hw; p += kPoolLanes) {
      const uint4 v = *reinterpret_cast<const uint4 *>(src + (size_t)p * x_pitch);
      s[0] += h2f_lo(v.x); s[1] += h2f_hi(v.x); s[2] += h2f_lo(v.y); s[3] += h2f_hi(v.y);
      s[4] += h2f_lo(v.z); s[5] += h2f_hi(v.z); s[6] += h2f_lo(v.w); s[7] += h2f_hi(v.w);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) part[lane][(threadIdx.x & 7) * 8 + k] = s[k];
  __syncthreads();
  if (threadIdx.x < kPoolCh && c0 + (int)threadIdx.x < c) {
    float t = part[0][threadIdx.x];
    for (int l = 1; l < kPoolLanes; ++l) t += part[l][threadIdx.x];
    out[(size_t)img * out_pitch + c0 + threadIdx.x] = __float2half_rn(t / (float)hw);
  }
}

inline bool off16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
inline bool bad_pitch(int pitch, int c) { return pitch < c || pitch % 8 != 0; }

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_lss_camera_gate_packed_size(int mid) {
  if (mid < 8 || mid > kGateMaxMid || mid % 8 != 0) return 0;
  return 2 * gate_branch_words(mid) * sizeof(float);
}

extern "C" int bevops_lss_camera_gate(const float *mlp_input, int in_pitch, const void *packed, float *gates, int n,
                                      int mid, void *stream) {
  if (!mlp_input || !packed || !gates || n < 0 || mid <= 0 || in_pitch < kGateIn) return BEVOPS_BAD_PARAM;
  if ((reinterpret_cast<uintptr_t>(mlp_input) & 3u) || (reinterpret_cast<uintptr_t>(packed) & 3u) ||
      (reinterpret_cast<uintptr_t>(gates) & 3u))
    return BEVOPS_BAD_PARAM;
  if (mid < 8 || mid > kGateMaxMid || mid % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  if (n > 0x3fffffff) return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(lss_camera_gate_kernel, dim3(2u * (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream),
                     mlp_input, in_pitch, static_cast<const float *>(packed), gates, n, mid);
  return launch_status();
}

extern "C" int bevops_se_gate2_nhwc(const void *x, int x_pitch, const float *gates, void *out_a, int a_pitch, void *out_b,
                                    int b_pitch, int n, int hw, int c, void *stream) {
  if (!x || !gates || !out_a || !out_b || n < 0 || hw <= 0 || c <= 0) return BEVOPS_BAD_PARAM;
  if (bad_pitch(x_pitch, c) || bad_pitch(a_pitch, c) || bad_pitch(b_pitch, c)) return BEVOPS_BAD_PARAM;
  if (off16(x) || off16(gates) || off16(out_a) || off16(out_b)) return BEVOPS_BAD_PARAM;
  if (c % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long nvec = (unsigned long long)n * hw * (c / 8);
  if ((nvec + 255) / 256 > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(se_gate2_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const __half *>(x), x_pitch, gates, static_cast<__half *>(out_a), a_pitch,
                     static_cast<__half *>(out_b), b_pitch, n, hw, c);
  return launch_status();
}

extern "C" int bevops_global_avgpool_nhwc(const void *x, int x_pitch, void *out, int out_pitch, int n, int hw, int c,
                                          void *stream) {
  if (!x || !out || n < 0 || hw <= 0 || c <= 0) return BEVOPS_BAD_PARAM;
  if (bad_pitch(x_pitch, c) || out_pitch < c) return BEVOPS_BAD_PARAM;
  if (off16(x) || (reinterpret_cast<uintptr_t>(out) & 1u)) return BEVOPS_BAD_PARAM;
  if (c % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  const int chunks = (c + kPoolCh - 1) / kPoolCh;
  if ((unsigned long long)n * chunks > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)(n * chunks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const __half *>(x), x_pitch, static_cast<__half *>(out), out_pitch, hw, c, chunks);
  return launch_status();
}
