// Glue of BEVDet's BEV half on channels-last fp16 activations (not reference plugins; TensorRT owns these layers there):
//
//  * lss_depth_split: the rows depth_net wrote -- [n * hw, row_stride], depth logits and context features side by side
//    -- to the two operands of bev_pool_v2: depth [n, D, hw] = softmax over the D logits of every pixel (plane-major:
//    what the pooling indexes by ranks_depth) and feat [n, hw, C] (pixel-major).  One launch instead of a softmax, two
//    slice / permute copies and their layout copies (det2trt/models/detector/bevdet.py:50-76).
//    The depth output is a transpose.  A block takes 64 pixels of one image: the logits are read row by row (lanes run
//    along the columns of a row), staged in LDS as [D][64 + 2], normalised there by four lanes per pixel, and written
//    plane by plane (lanes run along the pixels of a plane) -- both sides of the transpose move whole segments.
//  * upsample_bilinear_concat: FPN_LSS's cat([a, interpolate(b, bilinear, align_corners=True)], 1)
//    (models/necks/lss_fpn.py) in one pass with no up-sampled intermediate.  thread = 8 channels of one output pixel.
#include "common.h"
#include "lss_pos.h"

namespace bevops {
namespace {

constexpr int kSplitPix = 64;               // pixels per block
constexpr int kSplitLd = kSplitPix + 2;     // LDS row of one depth bin, in halves (33 words: rows fall on different banks)

__global__ __launch_bounds__(256) void lss_depth_split_kernel(const __half *__restrict__ x, __half *__restrict__ depth,
                                                              __half *__restrict__ feat, int hw, int tiles_per_image,
                                                              int row_stride, int depth_offset, int D, int feat_offset,
                                                              int C) {
  extern __shared__ __attribute__((aligned(16))) char split_smem[];
  __half *s = reinterpret_cast<__half *>(split_smem);     // [D][kSplitLd]
  const int tid = threadIdx.x;
  const int img = blockIdx.x / tiles_per_image, p0 = (blockIdx.x - img * tiles_per_image) * kSplitPix;
  const int np = min(kSplitPix, hw - p0);                 // live pixels of this tile (>= 1)
  const size_t row0 = (size_t)img * hw + p0;
  // (1) logits: lanes along the columns of a pixel row
  for (int i = tid; i < np * D; i += 256) {
    const int p = i / D, d = i - p * D;
    s[d * kSplitLd + p] = x[(row0 + p) * row_stride + depth_offset + d];
  }
  // (the features: pure data movement, 16 bytes per lane, independent of the LDS traffic)
  const int cv = C >> 3;
  for (int i = tid; i < np * cv; i += 256) {
    const int p = i / cv, v = i - p * cv;
    *reinterpret_cast<uint4 *>(feat + (row0 + p) * C + v * 8) =
        *reinterpret_cast<const uint4 *>(x + (row0 + p) * row_stride + feat_offset + v * 8);
  }
  __syncthreads();
  // (2) softmax in place: four lanes per pixel, bins q, q + 4, ...; fp32 maximum, exponentials and sum, one division
  // per value, one rounding.  Lanes of a dead pixel take part in the quad exchanges on neutral values.
  {
    const int p = tid >> 2, q = tid & 3;
    const bool live = p < np;
    float m = -INFINITY;
    if (live)
      for (int d = q; d < D; d += 4) m = fmaxf(m, __half2float(s[d * kSplitLd + p]));
    m = quad_max(m);
    float sum = 0.f;
    if (live)
      for (int d = q; d < D; d += 4) sum += expf(__half2float(s[d * kSplitLd + p]) - m);
    sum = quad_sum(sum);
    if (live)
      for (int d = q; d < D; d += 4) {
        const float e = expf(__half2float(s[d * kSplitLd + p]) - m);
        s[d * kSplitLd + p] = __float2half_rn(e / sum);
      }
  }
  __syncthreads();
  // (3) planes: lanes along the pixels of a depth bin
  __half *dst = depth + (size_t)img * D * hw + p0;
  for (int i = tid; i < D * kSplitPix; i += 256) {
    const int d = i / kSplitPix, p = i - d * kSplitPix;
    if (p < np) dst[(size_t)d * hw + p] = s[d * kSplitLd + p];
  }
}

__device__ __forceinline__ void unpack8(const uint4 v, float *f) {
  f[0] = h2f_lo(v.x); f[1] = h2f_hi(v.x); f[2] = h2f_lo(v.y); f[3] = h2f_hi(v.y);
  f[4] = h2f_lo(v.z); f[5] = h2f_hi(v.z); f[6] = h2f_lo(v.w); f[7] = h2f_hi(v.w);
}

__global__ __launch_bounds__(256) void upsample_bilinear_concat_f16_kernel(const __half *__restrict__ a,
                                                                           const __half *__restrict__ b,
                                                                           __half *__restrict__ out, int N, int H, int W,
                                                                           int Ca, int Hb, int Wb, int Cb) {
  const size_t cva = (size_t)Ca / 8, cv = (size_t)(Ca + Cb) / 8;
  const size_t nvec = (size_t)N * H * W * cv;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const size_t pix = i / cv;
  const size_t c8 = i - pix * cv;
  if (c8 < cva) {
    reinterpret_cast<uint4 *>(out)[i] = *reinterpret_cast<const uint4 *>(a + pix * Ca + c8 * 8);
    return;
  }
  const unsigned xo = (unsigned)(pix % (size_t)W);
  const size_t r = pix / (size_t)W;
  const unsigned yo = (unsigned)(r % (size_t)H);
  const size_t n = r / (size_t)H;
  unsigned y0, y1, x0, x1;
  float ly, lx;
  source_pos(yo, (unsigned)Hb, (unsigned)H, y0, y1, ly);
  source_pos(xo, (unsigned)Wb, (unsigned)W, x0, x1, lx);
  const size_t cb = (c8 - cva) * 8;
  const __half *bn = b + n * (size_t)Hb * Wb * Cb + cb;
  float v00[8], v01[8], v10[8], v11[8];
  unpack8(*reinterpret_cast<const uint4 *>(bn + ((size_t)y0 * Wb + x0) * Cb), v00);
  unpack8(*reinterpret_cast<const uint4 *>(bn + ((size_t)y0 * Wb + x1) * Cb), v01);
  unpack8(*reinterpret_cast<const uint4 *>(bn + ((size_t)y1 * Wb + x0) * Cb), v10);
  unpack8(*reinterpret_cast<const uint4 *>(bn + ((size_t)y1 * Wb + x1) * Cb), v11);
  const float hy = 1.f - ly, hx = 1.f - lx;
  float o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = hy * (hx * v00[k] + lx * v01[k]) + ly * (hx * v10[k] + lx * v11[k]);
  uint4 ov;
  ov.x = pack_h2(o[0], o[1]); ov.y = pack_h2(o[2], o[3]); ov.z = pack_h2(o[4], o[5]); ov.w = pack_h2(o[6], o[7]);
  reinterpret_cast<uint4 *>(out)[i] = ov;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_lss_depth_split(int dtype, const void *x, void *depth, void *feat, int n, int hw, int row_stride,
                                      int depth_offset, int D, int feat_offset, int C, void *stream) {
  if (!x || !depth || !feat || n < 0 || hw < 0) return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F16 || D < 1 || D > 256) return BEVOPS_NOT_SUPPORTED;
  if (C <= 0 || C % 8 != 0 || feat_offset < 0 || feat_offset % 8 != 0 || row_stride <= 0 || row_stride % 8 != 0 ||
      depth_offset < 0)
    return BEVOPS_BAD_PARAM;
  if ((long long)depth_offset + D > row_stride || (long long)feat_offset + C > row_stride) return BEVOPS_BAD_PARAM;
  if (!(depth_offset + D <= feat_offset || feat_offset + C <= depth_offset)) return BEVOPS_BAD_PARAM;   // overlap
  if (!aligned16(x) || !aligned16(feat) || (reinterpret_cast<uintptr_t>(depth) & 1u)) return BEVOPS_BAD_PARAM;
  if (n == 0 || hw == 0) return BEVOPS_SUCCESS;
  const long long tiles = (hw + kSplitPix - 1) / kSplitPix;
  if (tiles * n > 0x7fffffffLL) return BEVOPS_NOT_SUPPORTED;
  const size_t lds = (size_t)D * kSplitLd * sizeof(__half);   // <= 33 792 bytes
  hipLaunchKernelGGL(lss_depth_split_kernel, dim3((unsigned)(tiles * n)), dim3(256), lds,
                     static_cast<hipStream_t>(stream), (const __half *)x, (__half *)depth, (__half *)feat, hw, (int)tiles,
                     row_stride, depth_offset, D, feat_offset, C);
  return launch_status();
}

extern "C" int bevops_upsample_bilinear_concat_nhwc(int dtype, const void *a, const void *b, void *out, int n, int h,
                                                    int w, int ca, int hb, int wb, int cb, void *stream) {
  if (!b || !out || n <= 0 || h <= 0 || w <= 0 || hb <= 0 || wb <= 0 || ca < 0 || cb <= 0) return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  if (ca % 8 != 0 || cb % 8 != 0 || (ca > 0 && !a)) return BEVOPS_BAD_PARAM;
  if (!aligned16(b) || !aligned16(out) || (ca > 0 && !aligned16(a))) return BEVOPS_BAD_PARAM;
  // the source position is an exact 32-bit fraction: (h - 1) * (hb - 1) must fit
  if ((long long)h * hb > 0x7fffffffLL || (long long)w * wb > 0x7fffffffLL) return BEVOPS_NOT_SUPPORTED;
  const size_t nvec = (size_t)n * h * w * ((size_t)(ca + cb) / 8);
  if ((nvec + 255) / 256 > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  hipLaunchKernelGGL(upsample_bilinear_concat_f16_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), (const __half *)a, (const __half *)b, (__half *)out, n, h, w, ca,
                     hb, wb, cb);
  return launch_status();
}
