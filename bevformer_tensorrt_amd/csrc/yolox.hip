// The three data-movement layers of YOLOX (bevformer_tensorrt_amd/yolox.py) on channel slices of channels-last fp16
// tensors -- element (b, y, x, c) of a slice lives at base + ((b H + y) W + x) pitch + c, as in csrc/conv_slice.hip.
// All three are exact (copies and maxima), work in whole 16-byte vectors of 8 channels and are bound by memory.
//   bevops_focus_nhwc               mmdet's Focus (space to depth) from the planar image, padded to 32 channels
//   bevops_spp_maxpool_nhwc         SPPBottleneck's three stride-1 "same" max-pools, one launch
//   bevops_upsample_nearest2x_nhwc  nn.Upsample(scale_factor=2, mode="nearest")
#include "gemm_host.h"

namespace bevops {
namespace {

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

constexpr int kFocusC = 32;                    // 12 channels + 20 zeros: the stem convolution's Cin % 32 == 0

// out[b, y, x, 3 p + c] = image[b, c, 2 y + (p & 1), 2 x + (p >> 1)], p = 0 .. 3: (top-left, bottom-left, top-right,
// bottom-right); channels 12 .. 31 = 0.  One thread per output pixel and 8-channel vector.
__global__ void focus_kernel(const _Float16 *__restrict__ img, _Float16 *__restrict__ out, int out_pitch, int H, int W,
                             size_t pixels) {
  const int ho = H >> 1, wo = W >> 1;
  const size_t total = pixels * 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(i & 3);
    const size_t pix = i >> 2;
    const int x = (int)(pix % wo), y = (int)(pix / wo % ho);
    const size_t b = pix / ((size_t)wo * ho);
    h8_t v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ch = q * 8 + e;
      _Float16 s = (_Float16)0;
      if (ch < 12) {
        const int patch = ch / 3, c = ch - 3 * patch;
        s = img[((b * 3 + c) * H + 2 * y + (patch & 1)) * (size_t)W + 2 * x + (patch >> 1)];
      }
      v[e] = s;
    }
    *reinterpret_cast<h8_t *>(out + pix * out_pitch + q * 8) = v;
  }
}

// out slice j (channels [j C, (j + 1) C) behind `out`) = max over the (2 r_j + 1)^2 window, -inf outside the image.
// One thread per pixel and 8-channel vector walks the largest window once and feeds the three maxima by the
// Chebyshev distance of each element.  NaN: an element that is NaN replaces the running maximum and nothing replaces
// a NaN, so a NaN reaches every window that holds it (what F.max_pool2d does).
__global__ void spp_maxpool_kernel(const _Float16 *__restrict__ x, int x_pitch, _Float16 *__restrict__ out, int out_pitch,
                                   int H, int W, int C, int r0, int r1, int r2, size_t pixels) {
  const int c8n = C >> 3;
  const int rmax = max(r0, max(r1, r2));
  const size_t total = pixels * c8n;
  const _Float16 ninf = (_Float16)(-__builtin_huge_valf());
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c8n) * 8;
    const size_t pix = i / c8n;
    const int px = (int)(pix % W), py = (int)(pix / W % H);
    const size_t row0 = pix - (size_t)py * W - px;          // first pixel of this image
    h8_t m0, m1, m2;
#pragma unroll
    for (int e = 0; e < 8; ++e) m0[e] = m1[e] = m2[e] = ninf;
    const int ylo = max(py - rmax, 0), yhi = min(py + rmax, H - 1);
    const int xlo = max(px - rmax, 0), xhi = min(px + rmax, W - 1);
    for (int yy = ylo; yy <= yhi; ++yy) {
      const int dy = abs(yy - py);
      for (int xx = xlo; xx <= xhi; ++xx) {
        const int d = max(dy, abs(xx - px));
        const h8_t v = *reinterpret_cast<const h8_t *>(x + (row0 + (size_t)yy * W + xx) * x_pitch + c);
        const bool in0 = d <= r0, in1 = d <= r1, in2 = d <= r2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bool nan = v[e] != v[e];
          m0[e] = (in0 && (v[e] > m0[e] || nan)) ? v[e] : m0[e];
          m1[e] = (in1 && (v[e] > m1[e] || nan)) ? v[e] : m1[e];
          m2[e] = (in2 && (v[e] > m2[e] || nan)) ? v[e] : m2[e];
        }
      }
    }
    _Float16 *o = out + pix * out_pitch + c;
    *reinterpret_cast<h8_t *>(o) = m0;
    *reinterpret_cast<h8_t *>(o + C) = m1;
    *reinterpret_cast<h8_t *>(o + 2 * C) = m2;
  }
}

// out[b, Y, X, :] = x[b, Y / 2, X / 2, :]; one thread per output pixel and 8-channel vector
__global__ void upsample2x_kernel(const _Float16 *__restrict__ x, int x_pitch, _Float16 *__restrict__ out, int out_pitch,
                                  int H, int W, int C, size_t out_pixels) {
  const int c8n = C >> 3;
  const size_t total = out_pixels * c8n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c8n) * 8;
    const size_t pix = i / c8n;
    const int X = (int)(pix % (2 * W)), Y = (int)(pix / (2 * W) % (2 * H));
    const size_t b = pix / ((size_t)4 * W * H);
    const size_t src = (b * H + (Y >> 1)) * W + (X >> 1);
    *reinterpret_cast<h8_t *>(out + pix * out_pitch + c) = *reinterpret_cast<const h8_t *>(x + src * x_pitch + c);
  }
}

inline unsigned blocks_for(size_t total) {
  const size_t b = (total + 255) / 256;
  return (unsigned)(b < 65536 ? b : 65536);
}

// sizes every entry checks the same way: BAD_PARAM, NOT_SUPPORTED or SUCCESS
inline int slice_sizes(int B, int H, int W, int C, int x_pitch, int x_c, int out_pitch, int out_c) {
  if (B < 0 || H <= 0 || W <= 0 || C <= 0) return BEVOPS_BAD_PARAM;
  if (x_pitch < x_c || out_pitch < out_c || x_pitch % 8 != 0 || out_pitch % 8 != 0) return BEVOPS_BAD_PARAM;
  if (C % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  return BEVOPS_SUCCESS;
}

// ---- the same three layers on INT8 slices (the INT8 build of YOLOX, quantization.build_int8_yolox): 16 channels per
// 16-byte vector.  The pools and the copy are exact and keep the scale of their input.
typedef signed char s8x16_t __attribute__((ext_vector_type(16)));

// focus_kernel leaving as int8: q = clamp(rne(x * inv_scale), -127, 127), the product in fp32 (one rounding); channels
// 12 .. 31 = 0.  One thread per output pixel: two 16-byte vectors, the second all zeros.
__global__ void focus_q_kernel(const _Float16 *__restrict__ img, signed char *__restrict__ out, int out_pitch, int H, int W,
                               float inv_scale, size_t pixels) {
  const int ho = H >> 1, wo = W >> 1;
  for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(pix % wo), y = (int)(pix / wo % ho);
    const size_t b = pix / ((size_t)wo * ho);
    s8x16_t v, z;
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) {
      z[ch] = 0;
      v[ch] = 0;
      if (ch < 12) {
        const int patch = ch / 3, c = ch - 3 * patch;
        const float s = (float)img[((b * 3 + c) * H + 2 * y + (patch & 1)) * (size_t)W + 2 * x + (patch >> 1)];
        const float t = s * inv_scale;
        v[ch] = (signed char)(int)fminf(fmaxf(rintf(t), -127.f), 127.f);
      }
    }
    *reinterpret_cast<s8x16_t *>(out + pix * out_pitch) = v;
    *reinterpret_cast<s8x16_t *>(out + pix * out_pitch + 16) = z;
  }
}

// spp_maxpool_kernel on signed bytes: padding -128; a window always holds its centre, so -128 leaves only where the
// input holds it
__global__ void spp_maxpool_s8_kernel(const signed char *__restrict__ x, int x_pitch, signed char *__restrict__ out,
                                      int out_pitch, int H, int W, int C, int r0, int r1, int r2, size_t pixels) {
  const int c16n = C >> 4;
  const int rmax = max(r0, max(r1, r2));
  const size_t total = pixels * c16n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c16n) * 16;
    const size_t pix = i / c16n;
    const int px = (int)(pix % W), py = (int)(pix / W % H);
    const size_t row0 = pix - (size_t)py * W - px;          // first pixel of this image
    s8x16_t m0, m1, m2;
#pragma unroll
    for (int e = 0; e < 16; ++e) m0[e] = m1[e] = m2[e] = (signed char)-128;
    const int ylo = max(py - rmax, 0), yhi = min(py + rmax, H - 1);
    const int xlo = max(px - rmax, 0), xhi = min(px + rmax, W - 1);
    for (int yy = ylo; yy <= yhi; ++yy) {
      const int dy = abs(yy - py);
      for (int xx = xlo; xx <= xhi; ++xx) {
        const int d = max(dy, abs(xx - px));
        const s8x16_t v = *reinterpret_cast<const s8x16_t *>(x + (row0 + (size_t)yy * W + xx) * x_pitch + c);
        const bool in0 = d <= r0, in1 = d <= r1, in2 = d <= r2;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          m0[e] = (in0 && v[e] > m0[e]) ? v[e] : m0[e];
          m1[e] = (in1 && v[e] > m1[e]) ? v[e] : m1[e];
          m2[e] = (in2 && v[e] > m2[e]) ? v[e] : m2[e];
        }
      }
    }
    signed char *o = out + pix * out_pitch + c;
    *reinterpret_cast<s8x16_t *>(o) = m0;
    *reinterpret_cast<s8x16_t *>(o + C) = m1;
    *reinterpret_cast<s8x16_t *>(o + 2 * C) = m2;
  }
}

// upsample2x_kernel on bytes: one thread per output pixel and 16-channel vector
__global__ void upsample2x_s8_kernel(const signed char *__restrict__ x, int x_pitch, signed char *__restrict__ out,
                                     int out_pitch, int H, int W, int C, size_t out_pixels) {
  const int c16n = C >> 4;
  const size_t total = out_pixels * c16n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c16n) * 16;
    const size_t pix = i / c16n;
    const int X = (int)(pix % (2 * W)), Y = (int)(pix / (2 * W) % (2 * H));
    const size_t b = pix / ((size_t)4 * W * H);
    const size_t src = (b * H + (Y >> 1)) * W + (X >> 1);
    *reinterpret_cast<s8x16_t *>(out + pix * out_pitch + c) = *reinterpret_cast<const s8x16_t *>(x + src * x_pitch + c);
  }
}

// slice_sizes for int8 slices: pitches and channel counts in 16-byte vectors of 16 channels
inline int slice_sizes_s8(int B, int H, int W, int C, int x_pitch, int x_c, int out_pitch, int out_c) {
  if (B < 0 || H <= 0 || W <= 0 || C <= 0) return BEVOPS_BAD_PARAM;
  if (x_pitch < x_c || out_pitch < out_c || x_pitch % 16 != 0 || out_pitch % 16 != 0) return BEVOPS_BAD_PARAM;
  if (C % 16 != 0) return BEVOPS_NOT_SUPPORTED;
  return BEVOPS_SUCCESS;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_focus_nhwc_q(const void *image, float scale, void *out, int out_pitch, int B, int H, int W,
                                   void *stream) {
  if (!image || !out) return BEVOPS_BAD_PARAM;
  const int rc = slice_sizes_s8(B, H, W, kFocusC, 16, 16, out_pitch, kFocusC);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(image, 1u) || misaligned(out, 15u)) return BEVOPS_BAD_PARAM;
  if (!(scale > 0.f) || !(scale <= 3.4028234663852886e38f)) return BEVOPS_BAD_PARAM;
  if (H % 2 != 0 || W % 2 != 0) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long pixels = (unsigned long long)B * (H / 2) * (W / 2);
  if (gemm_over_limit(pixels, out_pitch, 1)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(focus_q_kernel, dim3(blocks_for(pixels)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const _Float16 *>(image), static_cast<signed char *>(out), out_pitch, H, W, 1.f / scale,
                     (size_t)pixels);
  return launch_status();
}

extern "C" int bevops_spp_maxpool_nhwc_s8(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W, int C,
                                          int k0, int k1, int k2, void *stream) {
  if (!x || !out || k0 <= 0 || k1 <= 0 || k2 <= 0) return BEVOPS_BAD_PARAM;
  const int rc = slice_sizes_s8(B, H, W, C, x_pitch, C, out_pitch, C > 0x2aaaaaaa ? 0x7fffffff : 3 * C);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(x, 15u) || misaligned(out, 15u)) return BEVOPS_BAD_PARAM;
  if (k0 % 2 == 0 || k1 % 2 == 0 || k2 % 2 == 0 || k0 > 13 || k1 > 13 || k2 > 13) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long pixels = (unsigned long long)B * H * W;
  if (gemm_over_limit(pixels, x_pitch, 1) || gemm_over_limit(pixels, out_pitch, 1)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(spp_maxpool_s8_kernel, dim3(blocks_for(pixels * (C / 16))), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const signed char *>(x), x_pitch, static_cast<signed char *>(out), out_pitch, H, W, C,
                     k0 / 2, k1 / 2, k2 / 2, (size_t)pixels);
  return launch_status();
}

extern "C" int bevops_upsample_nearest2x_nhwc_s8(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W,
                                                 int C, void *stream) {
  if (!x || !out) return BEVOPS_BAD_PARAM;
  const int rc = slice_sizes_s8(B, H, W, C, x_pitch, C, out_pitch, C);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(x, 15u) || misaligned(out, 15u)) return BEVOPS_BAD_PARAM;
  const unsigned long long out_pixels = 4ull * B * H * W;
  if (gemm_over_limit(out_pixels / 4, x_pitch, 1) || gemm_over_limit(out_pixels, out_pitch, 1)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(upsample2x_s8_kernel, dim3(blocks_for(out_pixels * (C / 16))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const signed char *>(x), x_pitch,
                     static_cast<signed char *>(out), out_pitch, H, W, C, (size_t)out_pixels);
  return launch_status();
}

extern "C" int bevops_focus_nhwc(const void *image, void *out, int out_pitch, int B, int H, int W, void *stream) {
  if (!image || !out) return BEVOPS_BAD_PARAM;
  const int rc = slice_sizes(B, H, W, kFocusC, 8, 8, out_pitch, kFocusC);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(image, 1u) || misaligned(out, 15u)) return BEVOPS_BAD_PARAM;
  if (H % 2 != 0 || W % 2 != 0) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long pixels = (unsigned long long)B * (H / 2) * (W / 2);
  if (gemm_over_limit(pixels, out_pitch, 2)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(focus_kernel, dim3(blocks_for(pixels * 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const _Float16 *>(image), static_cast<_Float16 *>(out), out_pitch, H, W, (size_t)pixels);
  return launch_status();
}

extern "C" int bevops_spp_maxpool_nhwc(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W, int C,
                                       int k0, int k1, int k2, void *stream) {
  if (!x || !out || k0 <= 0 || k1 <= 0 || k2 <= 0) return BEVOPS_BAD_PARAM;
  const int rc = slice_sizes(B, H, W, C, x_pitch, C, out_pitch, C > 0x2aaaaaaa ? 0x7fffffff : 3 * C);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(x, 15u) || misaligned(out, 15u)) return BEVOPS_BAD_PARAM;
  if (k0 % 2 == 0 || k1 % 2 == 0 || k2 % 2 == 0 || k0 > 13 || k1 > 13 || k2 > 13) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long pixels = (unsigned long long)B * H * W;
  if (gemm_over_limit(pixels, x_pitch, 2) || gemm_over_limit(pixels, out_pitch, 2)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(spp_maxpool_kernel, dim3(blocks_for(pixels * (C / 8))), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const _Float16 *>(x), x_pitch, static_cast<_Float16 *>(out), out_pitch, H, W, C, k0 / 2,
                     k1 / 2, k2 / 2, (size_t)pixels);
  return launch_status();
}

extern "C" int bevops_upsample_nearest2x_nhwc(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W,
                                              int C, void *stream) {
  if (!x || !out) return BEVOPS_BAD_PARAM;
  const int rc = slice_sizes(B, H, W, C, x_pitch, C, out_pitch, C);
  if (rc != BEVOPS_SUCCESS) return rc;
  if (misaligned(x, 15u) || misaligned(out, 15u)) return BEVOPS_BAD_PARAM;
  const unsigned long long out_pixels = 4ull * B * H * W;
  if (gemm_over_limit(out_pixels / 4, x_pitch, 2) || gemm_over_limit(out_pixels, out_pitch, 2)) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(upsample2x_kernel, dim3(blocks_for(out_pixels * (C / 8))), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const _Float16 *>(x), x_pitch, static_cast<_Float16 *>(out), out_pitch, H, W, C,
                     (size_t)out_pixels);
  return launch_status();
}
