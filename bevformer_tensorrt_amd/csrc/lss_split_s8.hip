// The INT8 siblings of lss_split.hip's two launches (the BEV half of the INT8 build of BEVDet):
//
//  * lss_depth_split_s8: depth_net's fp16 pixel rows -> the two INT8 operands of bev_pool_v2 in BEVOPS_I8: depth_q
//    [n, D, hw] = the softmax over each pixel's D logits, quantised with scale_depth; feat_q [n, hw, C] = the feature
//    columns quantised with scale_feat.  The fp16 kernel's shape: a block takes 64 pixels of one image, stages the logits
//    in LDS as [D][64 + 2], four lanes normalise each pixel and leave the quantised byte in the logit's own LDS slot, and
//    the planes are written with lanes along the pixels -- a lane packs four neighbouring pixels of one plane into one
//    dword where the plane's address allows, and stores bytes where it does not.
//    Operation order, every step ONE fp32 operation (inv_d = 1.f / scale_depth, inv_f = 1.f / scale_feat on the host):
//      m     = max over the pixel's D logits                         (exact)
//      e_d   = expf(x_d - m)
//      sum   : lane j of the pixel's quad adds its bins j, j + 4, j + 8, ... in ascending order to 0.f; then
//              s = s + s[lane ^ 1]; s = s + s[lane ^ 2]              (the four lanes end on the same bits)
//      p     = e_d / sum                                             (IEEE division)
//      q     = min(max(rne(p * inv_d), -127), 127)
//      feat_q = min(max(rne((float)x * inv_f), -127), 127)
//    A NaN leaves as -127.  A non-finite logit spoils its own pixel's D bytes and nothing else.
//  * upsample_bilinear_s8: F.interpolate(b, (h, w), mode="bilinear", align_corners=True) on an INT8 channel slice,
//    requantised into a channel slice of the consumer's buffer.  thread = 16 channels of one output pixel: four 16-byte
//    loads, one 16-byte store.  The source position is lss_pos.h's exact fraction.  On the corners converted exactly to
//    fp32, in this order (r = scale_b * (1.f / scale_out) on the host in fp32):
//      hx = 1 - lx, hy = 1 - ly
//      t = hx * v00;  t = fma(lx, v01, t);  u = hx * v10;  u = fma(lx, v11, u);  o = hy * t;  o = fma(ly, u, o)
//      v = o * r;  q = min(max(rne(v), -127), 127)
#include "common.h"
#include "lss_pos.h"

namespace bevops {
namespace {

constexpr int kSplitPix = 64;               // pixels per block
constexpr int kSplitLd = kSplitPix + 2;     // LDS row of one depth bin, in halves (33 words: rows fall on different banks)

typedef signed char s8x16_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int quant_s8(float t) {   // NaN -> -127 (fmaxf drops the NaN)
  return (int)fminf(fmaxf(rintf(t), -127.f), 127.f);
}

__global__ __launch_bounds__(256) void lss_depth_split_s8_kernel(const __half *__restrict__ x,
                                                                 signed char *__restrict__ depth,
                                                                 signed char *__restrict__ feat, int hw,
                                                                 int tiles_per_image, int row_stride, int depth_offset,
                                                                 int D, int feat_offset, int C, float inv_d, float inv_f) {
  extern __shared__ __attribute__((aligned(16))) char split_s8_smem[];
  __half *s = reinterpret_cast<__half *>(split_s8_smem);     // [D][kSplitLd]: the logit, then its quantised byte
  short *sq = reinterpret_cast<short *>(split_s8_smem);
  const int tid = threadIdx.x;
  const int img = blockIdx.x / tiles_per_image, p0 = (blockIdx.x - img * tiles_per_image) * kSplitPix;
  const int np = min(kSplitPix, hw - p0);                 // live pixels of this tile (>= 1)
  const size_t row0 = (size_t)img * hw + p0;
  // (1) logits: lanes along the columns of a pixel row
  for (int i = tid; i < np * D; i += 256) {
    const int p = i / D, d = i - p * D;
    s[d * kSplitLd + p] = x[(row0 + p) * row_stride + depth_offset + d];
  }
  // (the features: 32 bytes in, 16 bytes out per lane, independent of the LDS traffic)
  const int cv = C >> 4;
  for (int i = tid; i < np * cv; i += 256) {
    const int p = i / cv, v = i - p * cv;
    const __half *src = x + (row0 + p) * row_stride + feat_offset + v * 16;
    const uint4 a = *reinterpret_cast<const uint4 *>(src), b = *reinterpret_cast<const uint4 *>(src + 8);
    const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    s8x16_t o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      o[2 * k] = (signed char)quant_s8(mul_rn(h2f_lo(w[k]), inv_f));
      o[2 * k + 1] = (signed char)quant_s8(mul_rn(h2f_hi(w[k]), inv_f));
    }
    *reinterpret_cast<s8x16_t *>(feat + (row0 + p) * C + v * 16) = o;
  }
  __syncthreads();
  // (2) softmax in place: four lanes per pixel, bins j, j + 4, ...; the quantised byte takes the logit's slot.  Lanes of
  // a dead pixel take part in the quad exchanges on neutral values.
  {
    const int p = tid >> 2, j = tid & 3;
    const bool live = p < np;
    float m = -INFINITY;
    if (live)
      for (int d = j; d < D; d += 4) m = fmaxf(m, __half2float(s[d * kSplitLd + p]));
    m = quad_max(m);
    float sum = 0.f;
    if (live)
      for (int d = j; d < D; d += 4) sum = add_rn(sum, expf(sub_rn(__half2float(s[d * kSplitLd + p]), m)));
    sum = quad_sum(sum);
    if (live)
      for (int d = j; d < D; d += 4) {
        const float e = expf(sub_rn(__half2float(s[d * kSplitLd + p]), m));
        sq[d * kSplitLd + p] = (short)quant_s8(mul_rn(e / sum, inv_d));
      }
  }
  __syncthreads();
  // (3) planes: lanes along the pixels of a depth bin, four pixels per lane
  signed char *dst = depth + (size_t)img * D * hw + p0;
  for (int i = tid; i < D * (kSplitPix / 4); i += 256) {
    const int d = i / (kSplitPix / 4), p = (i - d * (kSplitPix / 4)) * 4;
    if (p >= np) continue;
    signed char *o = dst + (size_t)d * hw + p;
    const short *q = sq + d * kSplitLd + p;
    if (p + 3 < np && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
      *reinterpret_cast<unsigned *>(o) = ((unsigned)q[0] & 0xffu) | (((unsigned)q[1] & 0xffu) << 8) |
                                         (((unsigned)q[2] & 0xffu) << 16) | (((unsigned)q[3] & 0xffu) << 24);
    } else {
      for (int k = 0; k < 4 && p + k < np; ++k) o[k] = (signed char)q[k];
    }
  }
}

__global__ __launch_bounds__(256) void upsample_bilinear_s8_kernel(const signed char *__restrict__ b, int b_pitch,
                                                                   signed char *__restrict__ out, int out_pitch, int H,
                                                                   int W, int Hb, int Wb, int C, float r, size_t nvec) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const size_t cv = (size_t)C >> 4;
  const size_t pix = i / cv;
  const size_t c = (i - pix * cv) * 16;
  const unsigned xo = (unsigned)(pix % (size_t)W);
  const size_t row = pix / (size_t)W;
  const unsigned yo = (unsigned)(row % (size_t)H);
  const size_t n = row / (size_t)H;
  unsigned y0, y1, x0, x1;
  float ly, lx;
  source_pos(yo, (unsigned)Hb, (unsigned)H, y0, y1, ly);
  source_pos(xo, (unsigned)Wb, (unsigned)W, x0, x1, lx);
  const signed char *bn = b + n * (size_t)Hb * Wb * b_pitch + c;
  const s8x16_t v00 = *reinterpret_cast<const s8x16_t *>(bn + ((size_t)y0 * Wb + x0) * b_pitch);
  const s8x16_t v01 = *reinterpret_cast<const s8x16_t *>(bn + ((size_t)y0 * Wb + x1) * b_pitch);
  const s8x16_t v10 = *reinterpret_cast<const s8x16_t *>(bn + ((size_t)y1 * Wb + x0) * b_pitch);
  const s8x16_t v11 = *reinterpret_cast<const s8x16_t *>(bn + ((size_t)y1 * Wb + x1) * b_pitch);
  const float hy = sub_rn(1.f, ly), hx = sub_rn(1.f, lx);
  s8x16_t q;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    float t = mul_rn(hx, (float)v00[k]);
    t = fmaf(lx, (float)v01[k], t);
    float u = mul_rn(hx, (float)v10[k]);
    u = fmaf(lx, (float)v11[k], u);
    float o = mul_rn(hy, t);
    o = fmaf(ly, u, o);
    q[k] = (signed char)quant_s8(mul_rn(o, r));
  }
  *reinterpret_cast<s8x16_t *>(out + pix * out_pitch + c) = q;
}

inline bool good_scale(float s) { return s > 0.f && s <= 3.4028234663852886e38f; }

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_lss_depth_split_s8(const void *x_f16, void *depth_q, void *feat_q, int n, int hw, int row_stride,
                                         int depth_offset, int D, int feat_offset, int C, float scale_depth,
                                         float scale_feat, void *stream) {
  if (!x_f16 || !depth_q || !feat_q || n < 0 || hw < 0) return BEVOPS_BAD_PARAM;
  if (D < 1 || D > 256) return BEVOPS_NOT_SUPPORTED;
  if (C <= 0 || C % 16 != 0 || feat_offset < 0 || feat_offset % 8 != 0 || row_stride <= 0 || row_stride % 8 != 0 ||
      depth_offset < 0)
    return BEVOPS_BAD_PARAM;
  if ((long long)depth_offset + D > row_stride || (long long)feat_offset + C > row_stride) return BEVOPS_BAD_PARAM;
  if (!(depth_offset + D <= feat_offset || feat_offset + C <= depth_offset)) return BEVOPS_BAD_PARAM;   // overlap
  if (!aligned16(x_f16) || !aligned16(feat_q)) return BEVOPS_BAD_PARAM;
  if (!good_scale(scale_depth) || !good_scale(scale_feat)) return BEVOPS_BAD_PARAM;
  if (n == 0 || hw == 0) return BEVOPS_SUCCESS;
  const long long tiles = (hw + kSplitPix - 1) / kSplitPix;
  if (tiles * n > 0x7fffffffLL) return BEVOPS_NOT_SUPPORTED;
  const size_t lds = (size_t)D * kSplitLd * sizeof(__half);   // <= 33 792 bytes
  hipLaunchKernelGGL(lss_depth_split_s8_kernel, dim3((unsigned)(tiles * n)), dim3(256), lds,
                     static_cast<hipStream_t>(stream), (const __half *)x_f16, (signed char *)depth_q,
                     (signed char *)feat_q, hw, (int)tiles, row_stride, depth_offset, D, feat_offset, C,
                     1.f / scale_depth, 1.f / scale_feat);
  return launch_status();
}

extern "C" int bevops_upsample_bilinear_s8(const void *b_q, int b_pitch, float scale_b, void *out_q, int out_pitch,
                                           float scale_out, int n, int h, int w, int hb, int wb, int C, void *stream) {
  if (!b_q || !out_q || n < 0 || h <= 0 || w <= 0 || hb <= 0 || wb <= 0 || C <= 0) return BEVOPS_BAD_PARAM;
  if (C % 16 != 0 || b_pitch < C || out_pitch < C || b_pitch % 16 != 0 || out_pitch % 16 != 0) return BEVOPS_BAD_PARAM;
  if (!aligned16(b_q) || !aligned16(out_q)) return BEVOPS_BAD_PARAM;
  if (!good_scale(scale_b) || !good_scale(scale_out)) return BEVOPS_BAD_PARAM;
  // the source position is an exact 32-bit fraction: (h - 1) * (hb - 1) must fit
  if ((long long)h * hb > 0x7fffffffLL || (long long)w * wb > 0x7fffffffLL) return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  const unsigned long long in_pix = (unsigned long long)n * hb * wb, out_pix = (unsigned long long)n * h * w;
  if (in_pix > 0x7fffffffull || out_pix > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  // b must not overlap out.  Two byte ranges that meet are still disjoint when they are channel slices of one buffer:
  // equal pitches, and the distance between their first channels, modulo the pitch, leaves room for C channels each way
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(b_q), o0 = reinterpret_cast<uintptr_t>(out_q);
  const uintptr_t b1 = b0 + (in_pix - 1) * (unsigned long long)b_pitch + C;
  const uintptr_t o1 = o0 + (out_pix - 1) * (unsigned long long)out_pitch + C;
  if (b0 < o1 && o0 < b1) {
    if (b_pitch != out_pitch) return BEVOPS_BAD_PARAM;
    const uintptr_t d = (o0 >= b0 ? o0 - b0 : (uintptr_t)b_pitch - (b0 - o0) % b_pitch) % b_pitch;
    if (d < (uintptr_t)C || d + C > (uintptr_t)b_pitch) return BEVOPS_BAD_PARAM;
  }
  const size_t nvec = (size_t)out_pix * ((size_t)C / 16);
  if ((nvec + 255) / 256 > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  const float r = scale_b * (1.f / scale_out);
  hipLaunchKernelGGL(upsample_bilinear_s8_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), (const signed char *)b_q, b_pitch, (signed char *)out_q, out_pitch,
                     h, w, hb, wb, C, r, nvec);
  return launch_status();
}
