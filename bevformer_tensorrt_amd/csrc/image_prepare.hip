// BEVDet's camera front end (design/image_prepare.md; not a reference plugin): the test branch of
// PrepareImageInputs (third_party/bev_mmdet3d/datasets/pipelines/loading.py:747-754 img_transform_core, :691-699
// mmlabNormalize) as ONE launch: raw [N, H0, W0, 3] uint8 RGB -> PIL's antialiased bicubic `Image.resize`
// (Pillow's Resample.c, 8 bits per channel: 22-bit fixed-point coefficients, int32 sums, horizontal pass first, the
// result clipped to uint8 after EACH pass) -> crop -> optional left-right flip -> mmcv.imnormalize -> [N, 3, fH, fW]
// fp16 / fp32 planes or channels-last, optionally also the uint8 canvas [N, fH, fW, 3].  Bit-exact to PIL: the
// arithmetic is integer, and the coefficient tables are built on the HOST in double, in Pillow's operation order
// (bevops_image_resize_plan_build), uploaded once per geometry.
//
// One block = one 32 x 16 tile of the cropped output of one image.  The tile's source window (the rows and columns
// its taps touch, nothing else: the crop limits what is read at all) is staged in LDS with aligned dword loads, the
// horizontal pass writes its uint8 result for every window row into LDS, the vertical pass reads that.
#include <math.h>
#include <string.h>

#include "image_resample.h"   // to_out

namespace bevops {
namespace {

constexpr int kTW = 32, kTH = 16, kThreads = 256;   // tile of cropped output pixels; 8 rows of 32 lanes per pass step
constexpr int kPrecBits = 22;                       // Resample.c PRECISION_BITS = 32 - 8 - 2
constexpr int kHeader = 16;                         // int32 words in front of the tables
constexpr int kMagic = 0x50524549;
constexpr size_t kMaxLds = 64 * 1024;

struct Geometry {
  int H0, W0, rW, rH, cx0, cy0, cW, cH;   // source, resized size, crop origin and size
  int ksx, ksy;                           // taps per output column / row (Pillow's ksize)
  int winW, winH;                         // largest source window of a tile, in pixels / rows
  int srcPitch, midPitch;                 // LDS row pitches in bytes (multiples of 4)
};

// ---------------------------------------------------------------- host: Pillow's precompute_coeffs, one axis
struct Axis {
  int in, out, ksize;
  double scale, filterscale, support;
};

inline double bicubic_filter(double x) {   // Resample.c bicubic_filter, a = -0.5
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

inline Axis make_axis(int in, int out) {
#pragma clang fp contract(off)
  Axis a;
  a.in = in, a.out = out;
  a.scale = a.filterscale = (double)in / out;
  if (a.filterscale < 1.0) a.filterscale = 1.0;
  a.support = 2.0 * a.filterscale;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  return a;
}

inline void axis_bounds(const Axis &a, int xx, int *xmin, int *count) {
#pragma clang fp contract(off)
  const double center = (xx + 0.5) * a.scale;
  int lo = (int)(center - a.support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + a.support + 0.5);
  if (hi > a.in) hi = a.in;
  *xmin = lo, *count = hi - lo;
}

// bounds [n][2] and coefficients [n][ksize] of output indices lo .. lo + n - 1; false if a coefficient leaves 24 bits
bool axis_tables(const Axis &a, int lo, int n, int *bounds, int *coef, double *w) {
#pragma clang fp contract(off)
  const double ss = 1.0 / a.filterscale;
  for (int i = 0; i < n; ++i) {
    int xmin, cnt;
    axis_bounds(a, lo + i, &xmin, &cnt);
    const double center = (lo + i + 0.5) * a.scale;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) {
      w[x] = bicubic_filter((x + xmin - center + 0.5) * ss);
      ww += w[x];                                        // in tap order
    }
    int *k = coef + (size_t)i * a.ksize;
    for (int x = 0; x < a.ksize; ++x) {
      double v = x < cnt ? w[x] : 0.0;
      if (x < cnt && ww != 0.0) v /= ww;
      const int q = v < 0 ? (int)(-0.5 + v * (1 << kPrecBits)) : (int)(0.5 + v * (1 << kPrecBits));
      if (q >= (1 << 23) || q < -(1 << 23)) return false;   // (the kernel multiplies with 24-bit operands)
      k[x] = q;
    }
    bounds[2 * i] = xmin, bounds[2 * i + 1] = cnt;
  }
  return true;
}

// Whether every coefficient of output indices lo .. lo + n - 1 stays within 24 bits, writing no table: what
// plan_size, plan_build and the launch agree on before any of them accepts a geometry's plan size.
bool axis_fits(const Axis &a, int lo, int n) {
  int *k = new int[a.ksize];
  double *w = new double[a.ksize];
  int b[2];
  bool ok = true;
  for (int i = 0; ok && i < n; ++i) ok = axis_tables(a, lo + i, 1, b, k, w);
  delete[] k;
  delete[] w;
  return ok;
}

// BEVOPS_SUCCESS and *g filled, or why not.  Pure host arithmetic.
int make_geometry(int H0, int W0, int rW, int rH, int cx0, int cy0, int cx1, int cy1, Geometry *g) {
  if (H0 <= 0 || W0 <= 0 || rW <= 0 || rH <= 0 || cx1 <= cx0 || cy1 <= cy0) return BEVOPS_BAD_PARAM;
  if (cx0 < 0 || cy0 < 0 || cx1 > rW || cy1 > rH) return BEVOPS_NOT_SUPPORTED;   // PIL zero-fills there: not restated
  if (H0 > (1 << 20) || W0 > (1 << 20) || rW > (1 << 20) || rH > (1 << 20)) return BEVOPS_NOT_SUPPORTED;
  const Axis ax = make_axis(W0, rW), ay = make_axis(H0, rH);
  g->H0 = H0, g->W0 = W0, g->rW = rW, g->rH = rH, g->cx0 = cx0, g->cy0 = cy0, g->cW = cx1 - cx0, g->cH = cy1 - cy0;
  g->ksx = ax.ksize, g->ksy = ay.ksize;
  g->winW = g->winH = 0;
  for (int t = 0; t < g->cW; t += kTW) {        // bounds are non-decreasing in the output index
    const int last = (t + kTW < g->cW ? t + kTW : g->cW) - 1;
    int a, b, c, d;
    axis_bounds(ax, cx0 + t, &a, &b);
    axis_bounds(ax, cx0 + last, &c, &d);
    if (c + d - a > g->winW) g->winW = c + d - a;
  }
  for (int t = 0; t < g->cH; t += kTH) {
    const int last = (t + kTH < g->cH ? t + kTH : g->cH) - 1;
    int a, b, c, d;
    axis_bounds(ay, cy0 + t, &a, &b);
    axis_bounds(ay, cy0 + last, &c, &d);
    if (c + d - a > g->winH) g->winH = c + d - a;
  }
  g->srcPitch = (g->winW * 3 + 3 + 3) & ~3;     // + up to 3 bytes in front of an unaligned row start
  const int tw = g->cW < kTW ? g->cW : kTW;
  g->midPitch = (tw * 3 + 3) & ~3;
  return BEVOPS_SUCCESS;
}

size_t lds_bytes(const Geometry &g) {
  const size_t tw = g.cW < kTW ? g.cW : kTW, th = g.cH < kTH ? g.cH : kTH;
  return (tw * g.ksx + th * g.ksy) * sizeof(int) + (size_t)g.winH * (g.srcPitch + g.midPitch);
}

size_t plan_words(const Geometry &g) {
  return (size_t)kHeader + (size_t)g.cW * (2 + g.ksx) + (size_t)g.cH * (2 + g.ksy);
}

// ---------------------------------------------------------------- device
__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kPrecBits;                  // arithmetic shift, as C's on Pillow's int
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// pixel * coefficient + acc with 24-bit operands (|coefficient| < 2^23, pixel < 2^8): one v_mad_i32_i24
__device__ __forceinline__ int mad24(int a, int b, int acc) { return __mul24(a, b) + acc; }

struct Norm {
  float m0, m1, m2, i0, i1, i2;
};

template <typename Out, bool NHWC>
__global__ __launch_bounds__(kThreads) void image_prepare_kernel(const uint8_t *__restrict__ img,
                                                                 const int *__restrict__ plan, Out *__restrict__ out,
                                                                 uint8_t *__restrict__ canvas, Geometry g, Norm nm,
                                                                 int to_rgb, int flip) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH, n = blockIdx.z;
  const int tw = min(kTW, g.cW - tx0), th = min(kTH, g.cH - ty0);
  const int *bx = plan + kHeader, *kx = bx + 2 * g.cW;
  const int *by = kx + (size_t)g.cW * g.ksx, *ky = by + 2 * g.cH;

  int *cxs = reinterpret_cast<int *>(smem);               // [tw][ksx]
  int *cys = cxs + min(kTW, g.cW) * g.ksx;                // [th][ksy]
  unsigned char *src = reinterpret_cast<unsigned char *>(cys + min(kTH, g.cH) * g.ksy);   // [winH][srcPitch]
  unsigned char *mid = src + (size_t)g.winH * g.srcPitch;                                 // [winH][midPitch]

  // the tile's source window; clamped so that a plan of another geometry cannot index outside the images or the LDS
  int x0 = bx[2 * tx0], x1 = bx[2 * (tx0 + tw - 1)] + bx[2 * (tx0 + tw - 1) + 1];
  int y0 = by[2 * ty0], y1 = by[2 * (ty0 + th - 1)] + by[2 * (ty0 + th - 1) + 1];
  x0 = max(0, min(x0, g.W0)), x1 = max(x0, min(x1, min(g.W0, x0 + g.winW)));
  y0 = max(0, min(y0, g.H0)), y1 = max(y0, min(y1, min(g.H0, y0 + g.winH)));
  const int ww = x1 - x0, wh = y1 - y0;

  // ---- stage: one wave per window row, aligned dwords (a dword that holds one byte of the image lies in that byte's
  // page, so the up to 3 bytes in front of / behind an unaligned row are readable)
  const int lane = tid & 63, wave = tid >> 6;
  for (int r = wave; r < wh; r += kThreads / 64) {
    const uint8_t *row = img + (((size_t)n * g.H0 + (y0 + r)) * g.W0 + x0) * 3;
    const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(row) & 3u);
    const int nd = ww > 0 ? (int)(shift + ww * 3 + 3) >> 2 : 0;   // every dword holds at least one byte of the row
    const unsigned *p = reinterpret_cast<const unsigned *>(row - shift);
    unsigned *d = reinterpret_cast<unsigned *>(src + (size_t)r * g.srcPitch);
    for (int i = lane; i < nd; i += 64) d[i] = p[i];
  }
  for (int i = tid; i < tw * g.ksx; i += kThreads) cxs[i] = kx[(size_t)tx0 * g.ksx + i];
  for (int i = tid; i < th * g.ksy; i += kThreads) cys[i] = ky[(size_t)ty0 * g.ksy + i];
  __syncthreads();

  const int i = tid & (kTW - 1), j = tid >> 5;     // column of the tile, row group (8 rows per step)
  // ---- horizontal pass over every window row: Σ pixel * k in int32, + 2^21, >> 22, clip
  if (i < tw) {
    int xmin = bx[2 * (tx0 + i)] - x0, cnt = bx[2 * (tx0 + i) + 1];
    xmin = max(0, min(xmin, ww)), cnt = max(0, min(cnt, min(g.ksx, ww - xmin)));
    const int *k = cxs + i * g.ksx;
    for (int r = j; r < wh; r += kThreads / kTW) {
      const uint8_t *row = img + (((size_t)n * g.H0 + (y0 + r)) * g.W0 + x0) * 3;
      const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(row) & 3u);
      const unsigned char *s = src + (size_t)r * g.srcPitch + shift + xmin * 3;
      int a0 = 1 << (kPrecBits - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < cnt; ++t) {
        const int c = k[t];                        // |c| < 2^23 and 8-bit pixels: 24-bit multiply-add
        a0 = mad24((int)s[3 * t], c, a0);
        a1 = mad24((int)s[3 * t + 1], c, a1);
        a2 = mad24((int)s[3 * t + 2], c, a2);
      }
      unsigned char *m = mid + (size_t)r * g.midPitch + i * 3;
      m[0] = (unsigned char)clip8(a0), m[1] = (unsigned char)clip8(a1), m[2] = (unsigned char)clip8(a2);
    }
  }
  __syncthreads();

  // ---- vertical pass on the uint8 intermediate, normalise, store
  if (i < tw) {
    const int col = flip ? g.cW - 1 - (tx0 + i) : tx0 + i;
    for (int jj = j; jj < th; jj += kThreads / kTW) {
      int ymin = by[2 * (ty0 + jj)] - y0, cnt = by[2 * (ty0 + jj) + 1];
      ymin = max(0, min(ymin, wh)), cnt = max(0, min(cnt, min(g.ksy, wh - ymin)));
      const int *k = cys + jj * g.ksy;
      const unsigned char *m = mid + (size_t)ymin * g.midPitch + i * 3;
      int a0 = 1 << (kPrecBits - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < cnt; ++t) {
        const int c = k[t];
        a0 = mad24((int)m[0], c, a0);
        a1 = mad24((int)m[1], c, a1);
        a2 = mad24((int)m[2], c, a2);
        m += g.midPitch;
      }
      const int p0 = clip8(a0), p1 = clip8(a1), p2 = clip8(a2);
      const size_t pix = ((size_t)n * g.cH + (ty0 + jj)) * g.cW + col;
      if (canvas) {
        uint8_t *cv = canvas + pix * 3;
        cv[0] = (uint8_t)p0, cv[1] = (uint8_t)p1, cv[2] = (uint8_t)p2;
      }
      float a = (float)p0, b = (float)p1, c = (float)p2, v0, v1, v2;
      if (to_rgb) { const float t = a; a = c; c = t; }
      {
#pragma clang fp contract(off)
        v0 = (a - nm.m0) * nm.i0;   // cv2.subtract, then cv2.multiply by 1 / std: two roundings
        v1 = (b - nm.m1) * nm.i1;
        v2 = (c - nm.m2) * nm.i2;
      }
      if constexpr (NHWC) {
        Out *o = out + pix * 3;
        o[0] = to_out(v0, (Out *)nullptr), o[1] = to_out(v1, (Out *)nullptr), o[2] = to_out(v2, (Out *)nullptr);
      } else {
        const size_t plane = (size_t)g.cH * g.cW;
        Out *o = out + (size_t)n * 3 * plane + (size_t)(ty0 + jj) * g.cW + col;
        o[0] = to_out(v0, (Out *)nullptr), o[plane] = to_out(v1, (Out *)nullptr), o[2 * plane] = to_out(v2, (Out *)nullptr);
      }
    }
  }
}

template <typename Out>
int launch(const void *img, const void *plan, void *out, void *canvas, int N, const Geometry &g, const Norm &nm,
           int to_rgb, int flip, int channels_last, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)((g.cW + kTW - 1) / kTW), (unsigned)((g.cH + kTH - 1) / kTH), (unsigned)N);
  if (channels_last)
    hipLaunchKernelGGL((image_prepare_kernel<Out, true>), grid, dim3(kThreads), lds, st, (const uint8_t *)img,
                       (const int *)plan, (Out *)out, (uint8_t *)canvas, g, nm, to_rgb, flip);
  else
    hipLaunchKernelGGL((image_prepare_kernel<Out, false>), grid, dim3(kThreads), lds, st, (const uint8_t *)img,
                       (const int *)plan, (Out *)out, (uint8_t *)canvas, g, nm, to_rgb, flip);
  return launch_status();
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_image_resize_plan_size(int H0, int W0, int resize_w, int resize_h, int crop_x0, int crop_y0,
                                                int crop_x1, int crop_y1) {
  Geometry g;
  if (make_geometry(H0, W0, resize_w, resize_h, crop_x0, crop_y0, crop_x1, crop_y1, &g) != BEVOPS_SUCCESS) return 0;
  if (lds_bytes(g) > kMaxLds) return 0;
  if (!axis_fits(make_axis(W0, resize_w), crop_x0, g.cW) || !axis_fits(make_axis(H0, resize_h), crop_y0, g.cH)) return 0;
  return plan_words(g) * sizeof(int);
}

extern "C" int bevops_image_resize_plan_build(int H0, int W0, int resize_w, int resize_h, int crop_x0, int crop_y0,
                                              int crop_x1, int crop_y1, void *plan_host, size_t plan_bytes) {
  if (!plan_host) return BEVOPS_BAD_PARAM;
  Geometry g;
  const int st = make_geometry(H0, W0, resize_w, resize_h, crop_x0, crop_y0, crop_x1, crop_y1, &g);
  if (st != BEVOPS_SUCCESS) return st;
  if (lds_bytes(g) > kMaxLds) return BEVOPS_NOT_SUPPORTED;
  if (plan_bytes != plan_words(g) * sizeof(int)) return BEVOPS_BAD_PARAM;
  const Axis ax = make_axis(W0, resize_w), ay = make_axis(H0, resize_h);
  if (!axis_fits(ax, crop_x0, g.cW) || !axis_fits(ay, crop_y0, g.cH)) return BEVOPS_NOT_SUPPORTED;   // nothing written
  int *p = static_cast<int *>(plan_host);
  const int head[kHeader] = {kMagic, H0, W0, resize_w, resize_h, crop_x0, crop_y0, crop_x1, crop_y1,
                             g.ksx, g.ksy, g.winW, g.winH, kTW, kTH, 0};
  memcpy(p, head, sizeof(head));
  int *bx = p + kHeader, *kx = bx + 2 * g.cW, *by = kx + (size_t)g.cW * g.ksx, *ky = by + 2 * g.cH;
  double *w = new double[g.ksx > g.ksy ? g.ksx : g.ksy];
  axis_tables(ax, crop_x0, g.cW, bx, kx, w);
  axis_tables(ay, crop_y0, g.cH, by, ky, w);
  delete[] w;
  return BEVOPS_SUCCESS;
}

extern "C" int bevops_image_resize_crop_normalize(const void *images, const void *plan_dev, size_t plan_bytes,
                                                  int out_dtype, void *output, void *canvas_or_null, int N, int H0,
                                                  int W0, int resize_w, int resize_h, int crop_x0, int crop_y0,
                                                  int crop_x1, int crop_y1, int rotate, const double *mean_host,
                                                  const double *std_host, int to_rgb, int flip, int channels_last,
                                                  void *stream) {
  if (!images || !plan_dev || !output || !mean_host || !std_host || N <= 0) return BEVOPS_BAD_PARAM;
  if (rotate != 0) return BEVOPS_NOT_SUPPORTED;
  Geometry g;
  const int gs = make_geometry(H0, W0, resize_w, resize_h, crop_x0, crop_y0, crop_x1, crop_y1, &g);
  if (gs != BEVOPS_SUCCESS) return gs;
  const size_t lds = lds_bytes(g);
  if (lds > kMaxLds || N > 65535 || (g.cH + kTH - 1) / kTH > 65535) return BEVOPS_NOT_SUPPORTED;
  if (plan_bytes != plan_words(g) * sizeof(int)) return BEVOPS_BAD_PARAM;
  if (reinterpret_cast<uintptr_t>(plan_dev) & 3u) return BEVOPS_BAD_PARAM;
  if (out_dtype != BEVOPS_F16 && out_dtype != BEVOPS_F32) return BEVOPS_NOT_SUPPORTED;
  if (reinterpret_cast<uintptr_t>(output) & (out_dtype == BEVOPS_F16 ? 1u : 3u)) return BEVOPS_BAD_PARAM;
  Norm nm;
  float inv[3], mean[3];
  for (int c = 0; c < 3; ++c) {
    if (!(std_host[c] > 0.0)) return BEVOPS_BAD_PARAM;
    inv[c] = (float)(1.0 / std_host[c]);   // mmcv.imnormalize: stdinv = 1 / float64(std), applied in float32
    mean[c] = (float)mean_host[c];
  }
  nm.m0 = mean[0], nm.m1 = mean[1], nm.m2 = mean[2], nm.i0 = inv[0], nm.i1 = inv[1], nm.i2 = inv[2];
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (out_dtype == BEVOPS_F16)
    return launch<__half>(images, plan_dev, output, canvas_or_null, N, g, nm, to_rgb, flip, channels_last, lds, st);
  return launch<float>(images, plan_dev, output, canvas_or_null, N, g, nm, to_rgb, flip, channels_last, lds, st);
}
