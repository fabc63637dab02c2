// Camera front end of the two 2-D detectors (design/letterbox.md; not a reference plugin): the test pipelines of
// configs/yolox/yolox_x_8x8_300e_coco.py:75-92 (Resize(keep_ratio) on uint8 -> Pad(pad_to_square, 114)) and
// configs/centernet/centernet_resnet18_dcnv2_140e_coco.py:69-110 (Resize(keep_ratio) on float32 -> RandomCenterCropPad
// (test_mode, logical_or 31): a CENTRED paste into a zero canvas -> Pad -> Normalize) as ONE launch: raw [N, H0, W0, 3]
// uint8 -> bilinear resize to [Hs, Ws] in the operation order of cv::resize(INTER_LINEAR) written from its specification
// (arith 0: the 8-bit fixed-point form, 11-bit coefficients, the vertical pass on D >> 4; arith 1: the float32 form of
// csrc/image_scale.hip; an exact 2 : 1 in both axes takes the four-tap area form) -> paste at (oy, ox) into a constant
// [Hp, Wp] canvas -> normalise the resized value AND the pad value as csrc/image.hip does -> fp16 / fp32 planes or
// channels-last.  Parity against cv2 / mmcv / mmdet themselves is UNPINNED (none is available to the tests); the contract
// is the restatement in tests/util_letterbox.py, which this kernel equals bit for bit.
//
// One block = one 64 x 8 tile of the PADDED output of one image, as in csrc/image_scale.hip: the source window of the
// tile's resized pixels is staged in LDS with aligned dword loads, the horizontal pass writes every window row to LDS as
// [row][64 x 3] interleaved (arith 0: D >> 4 as uint16, exact; arith 1: float32), the vertical pass, the normalisation,
// the pad value and the store are one step.  A tile that lies in the padding alone stages nothing.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace bevops {
namespace {

constexpr int kTW = 64, kTH = 8, kThreads = 256;   // tile of padded output pixels; 4 rows of 64 lanes per pass step
constexpr int kRowGroups = kThreads / kTW;
constexpr size_t kMaxLds = 64 * 1024;
constexpr int kCoefBits = 11;                      // cv::resize: INTER_RESIZE_COEF_BITS, weights scaled by 2048

struct Geometry {
  int H0, W0, Hs, Ws, Hp, Wp, oy, ox;   // source, resized and padded size; where the resized image is pasted
  int winW, winH;                       // largest source window of a tile, in pixels / rows
  int srcPitch;                         // LDS row pitch of the staged uint8 window in bytes (a multiple of 4)
  int area;                             // 2 : 1 in both axes
  double sx, sy;                        // 1 / (out / in) per axis
};

struct Norm {
  float m0, m1, m2, i0, i1, i2, p0, p1, p2;   // mean, 1 / std and raw pad value per OUTPUT channel
};

// tap index and weight of output index d (cv::resize, INTER_LINEAR): the position in double, ONE rounding to float32
__host__ __device__ __forceinline__ void tap(int d, double scale, int in, int *i0, int *i1, float *f) {
#pragma clang fp contract(off)
  const double p = (d + 0.5) * scale;
  float fx = (float)(p - 0.5);
  int s = (int)floorf(fx);
  fx = fx - (float)s;
  if (s < 0) s = 0, fx = 0.f;
  if (s >= in - 1) s = in - 1, fx = 0.f;
  *i0 = s, *i1 = s + 1 < in ? s + 1 : in - 1, *f = fx;
}

// source columns / rows [lo, hi) that the taps of output indices [t0, t0 + n) touch (tap indices do not decrease with d)
__host__ __device__ __forceinline__ void window(int t0, int n, double scale, int in, int *lo, int *hi) {
  int a, b, c, d;
  float f;
  tap(t0, scale, in, &a, &b, &f);
  tap(t0 + n - 1, scale, in, &c, &d, &f);
  *lo = a, *hi = d + 1;
}

// resized indices [d0, d1) that the padded tile [t0, t0 + tile) holds when the resized axis is pasted at `off`
__host__ __device__ __forceinline__ void tile_span(int t0, int tile, int off, int out, int *d0, int *d1) {
  const int a = t0 - off, b = t0 + tile - off;
  *d0 = a < 0 ? 0 : a, *d1 = b > out ? out : b;
}

inline int max_window(int padded, int tile, int off, int out, double scale, int in) {
  int w = 0;
  for (int t = 0; t < padded; t += tile) {
    int d0, d1, lo, hi;
    tile_span(t, tile, off, out, &d0, &d1);
    if (d1 <= d0) continue;
    window(d0, d1 - d0, scale, in, &lo, &hi);
    if (hi - lo > w) w = hi - lo;
  }
  return w;
}

__device__ __forceinline__ float to_out(float v, float *) { return v; }
__device__ __forceinline__ __half to_out(float v, __half *) {   // a rounding step of its own (csrc/image.hip)
  unsigned r;
  asm("v_cvt_f16_f32 %0, %1" : "=v"(r) : "v"(v));
  return __ushort_as_half((unsigned short)r);
}

__device__ __forceinline__ float normalise(float x, float mean, float inv) {
#pragma clang fp contract(off)
  const float t = x - mean;   // cv2.subtract, then cv2.multiply by 1 / std: two roundings
  return t * inv;
}

__device__ __forceinline__ float one_minus(float f) {
#pragma clang fp contract(off)
  return 1.f - f;
}

__device__ __forceinline__ float lerp2(float a, float b, float w0, float w1) {
#pragma clang fp contract(off)
  const float p = a * w0, q = b * w1;
  return p + q;
}

__device__ __forceinline__ float area4(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const float s = a + b, t = s + c, u = t + d;
  return u * 0.25f;
}

// the 8-bit form's weights: rint(fl(fl(1 - f) * 2048)), rint(fl(f * 2048)), half to even (saturate_cast<short>)
__device__ __forceinline__ void fixed_weights(float f, int *a0, int *a1) {
#pragma clang fp contract(off)
  const float w0 = 1.f - f, s0 = w0 * (float)(1 << kCoefBits), s1 = f * (float)(1 << kCoefBits);
  *a0 = (int)rintf(s0), *a1 = (int)rintf(s1);
}

template <int ARITH, typename Out, bool NHWC>
__global__ __launch_bounds__(kThreads) void image_letterbox_kernel(const uint8_t *__restrict__ img, Out *__restrict__ out,
                                                                   Geometry g, Norm nm, int to_rgb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Mid = typename std::conditional<ARITH == 0, unsigned short, float>::type;
  const int tid = threadIdx.x, lane = tid & (kTW - 1), j = tid / kTW;
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH, n = blockIdx.z;
  const int pw = min(kTW, g.Wp - tx0), ph = min(kTH, g.Hp - ty0);   // padded pixels in the tile
  int dx0, dx1, dy0, dy1;                                           // resized pixels in the tile
  tile_span(tx0, kTW, g.ox, g.Ws, &dx0, &dx1);
  tile_span(ty0, kTH, g.oy, g.Hs, &dy0, &dy1);
  const bool inside = dx1 > dx0 && dy1 > dy0;                       // (else: a tile of padding alone)

  unsigned char *src = smem;                                                      // [winH][srcPitch]
  Mid *mid = reinterpret_cast<Mid *>(smem + (size_t)g.winH * g.srcPitch);         // [winH][kTW * 3]

  // the tile's source window, clamped to the image and to the LDS allocation
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  if (inside) {
    window(dx0, dx1 - dx0, g.sx, g.W0, &x0, &x1);
    window(dy0, dy1 - dy0, g.sy, g.H0, &y0, &y1);
    x0 = max(0, min(x0, g.W0)), x1 = max(x0, min(x1, min(g.W0, x0 + g.winW)));
    y0 = max(0, min(y0, g.H0)), y1 = max(y0, min(y1, min(g.H0, y0 + g.winH)));
  }
  const int ww = x1 - x0, wh = y1 - y0;
  const uint8_t *base = img + (size_t)n * g.H0 * g.W0 * 3;

  // ---- stage: one wave per window row, aligned dwords (a dword that holds one byte of the image lies in that byte's
  // page, so the up to 3 bytes in front of / behind an unaligned row are readable)
  for (int r = j; r < wh; r += kRowGroups) {
    const uint8_t *row = base + ((size_t)(y0 + r) * g.W0 + x0) * 3;
    const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(row) & 3u);
    const int nd = ww > 0 ? (int)(shift + ww * 3 + 3) >> 2 : 0;   // every dword holds at least one byte of the row
    const unsigned *p = reinterpret_cast<const unsigned *>(row - shift);
    unsigned *d = reinterpret_cast<unsigned *>(src + (size_t)r * g.srcPitch);
    for (int i = lane; i < nd; i += kTW) d[i] = p[i];
  }
  __syncthreads();

  // a window row as the taps read it: LDS bytes behind the row's alignment shift
  auto row_of = [&](int r) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(base) + ((size_t)(y0 + r) * g.W0 + x0) * 3;
    return src + (size_t)r * g.srcPitch + (unsigned)(a & 3u);
  };
  auto mean_of = [&](int ch) { return ch == 0 ? nm.m0 : (ch == 1 ? nm.m1 : nm.m2); };
  auto inv_of = [&](int ch) { return ch == 0 ? nm.i0 : (ch == 1 ? nm.i1 : nm.i2); };
  auto pad_of = [&](int ch) { return ch == 0 ? nm.p0 : (ch == 1 ? nm.p1 : nm.p2); };

  // ---- horizontal pass over every window row (general path): lane = tile column, OUTPUT channel order
  if (!g.area) {
    const int d = tx0 + lane - g.ox;
    if (inside && d >= dx0 && d < dx1) {
      int i0, i1;
      float f;
      tap(d, g.sx, g.W0, &i0, &i1, &f);
      i0 = max(0, min(i0 - x0, ww - 1)), i1 = max(0, min(i1 - x0, ww - 1));
      const float w0 = one_minus(f);
      int a0, a1;
      fixed_weights(f, &a0, &a1);
      for (int r = j; r < wh; r += kRowGroups) {
        const unsigned char *row = row_of(r);
        Mid *m = mid + (size_t)r * (kTW * 3) + lane * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int sc = to_rgb ? 2 - ch : ch;
          const int a = row[i0 * 3 + sc], b = row[i1 * 3 + sc];
          if constexpr (ARITH == 0)
            m[ch] = (unsigned short)((a * a0 + b * a1) >> 4);   // at most 255 * 2049 >> 4 = 32 655
          else
            m[ch] = lerp2((float)a, (float)b, w0, f);
        }
      }
    }
    __syncthreads();
  }

  // ---- vertical pass (or the area form), normalisation, padding, store: three (column, channel) slots per lane and row
  for (int jj = j; jj < ph; jj += kRowGroups) {
    const int y = ty0 + jj, dy = y - g.oy;
    const bool row_in = inside && dy >= dy0 && dy < dy1;
    int r0 = 0, r1 = 0, b0 = 0, b1 = 0;
    float fy = 0.f, wy = 1.f;
    if (row_in) {
      if (g.area) {
        r0 = max(0, min(2 * dy - y0, wh - 1)), r1 = max(0, min(2 * dy + 1 - y0, wh - 1));
      } else {
        tap(dy, g.sy, g.H0, &r0, &r1, &fy);
        r0 = max(0, min(r0 - y0, wh - 1)), r1 = max(0, min(r1 - y0, wh - 1));
        wy = one_minus(fy);
        fixed_weights(fy, &b0, &b1);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = lane + kTW * k;                       // channels-last: element of the tile row
      const int col = NHWC ? e / 3 : lane, ch = NHWC ? e - col * 3 : k;
      const int d = tx0 + col - g.ox;
      float v = pad_of(ch);
      if (row_in && d >= dx0 && d < dx1) {
        if (g.area) {
          const int sc = to_rgb ? 2 - ch : ch;
          const int c0 = max(0, min(2 * d - x0, ww - 1)), c1 = max(0, min(2 * d + 1 - x0, ww - 1));
          const unsigned char *up = row_of(r0), *low = row_of(r1);
          const int a = up[c0 * 3 + sc], b = up[c1 * 3 + sc], c = low[c0 * 3 + sc], dd = low[c1 * 3 + sc];
          if constexpr (ARITH == 0)
            v = (float)((a + b + c + dd + 2) >> 2);
          else
            v = area4((float)a, (float)b, (float)c, (float)dd);
        } else {
          const Mid m0 = mid[(size_t)r0 * (kTW * 3) + col * 3 + ch], m1 = mid[(size_t)r1 * (kTW * 3) + col * 3 + ch];
          if constexpr (ARITH == 0)
            v = (float)((((b0 * (int)m0) >> 16) + ((b1 * (int)m1) >> 16) + 2) >> 2);
          else
            v = lerp2(m0, m1, wy, fy);
        }
      }
      v = normalise(v, mean_of(ch), inv_of(ch));
      if (col < pw) {
        if constexpr (NHWC) {
          out[(((size_t)n * g.Hp + y) * g.Wp + tx0) * 3 + e] = to_out(v, (Out *)nullptr);
        } else {
          out[(((size_t)n * 3 + ch) * g.Hp + y) * g.Wp + tx0 + col] = to_out(v, (Out *)nullptr);
        }
      }
    }
  }
}

template <int ARITH, typename Out>
int launch(const void *img, void *out, int N, const Geometry &g, const Norm &nm, int to_rgb, int channels_last,
           size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)((g.Wp + kTW - 1) / kTW), (unsigned)((g.Hp + kTH - 1) / kTH), (unsigned)N);
  if (channels_last)
    hipLaunchKernelGGL((image_letterbox_kernel<ARITH, Out, true>), grid, dim3(kThreads), lds, st, (const uint8_t *)img,
                       (Out *)out, g, nm, to_rgb);
  else
    hipLaunchKernelGGL((image_letterbox_kernel<ARITH, Out, false>), grid, dim3(kThreads), lds, st, (const uint8_t *)img,
                       (Out *)out, g, nm, to_rgb);
  return launch_status();
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_image_letterbox(int arith, const void *images, int out_dtype, void *output, int N, int H0, int W0,
                                      int Hs, int Ws, int Hp, int Wp, int oy, int ox, const double *pad_host,
                                      const double *mean_host, const double *std_host, int to_rgb, int channels_last,
                                      void *stream) {
  if (!images || !output || !pad_host || !mean_host || !std_host) return BEVOPS_BAD_PARAM;
  if (N <= 0 || H0 <= 0 || W0 <= 0 || Hs <= 0 || Ws <= 0 || Hp <= 0 || Wp <= 0) return BEVOPS_BAD_PARAM;
  if (oy < 0 || ox < 0 || (long long)oy + Hs > Hp || (long long)ox + Ws > Wp) return BEVOPS_BAD_PARAM;
  float inv[3], mean[3], pad[3];
  for (int c = 0; c < 3; ++c) {
    if (!(std_host[c] > 0.0)) return BEVOPS_BAD_PARAM;
    inv[c] = (float)(1.0 / std_host[c]);   // mmcv.imnormalize: stdinv = 1 / float64(std), applied in float32
    mean[c] = (float)mean_host[c];
    pad[c] = (float)pad_host[to_rgb ? 2 - c : c];   // the canvas is filled before the channel swap
  }
  const Norm nm = {mean[0], mean[1], mean[2], inv[0], inv[1], inv[2], pad[0], pad[1], pad[2]};
  if (arith != 0 && arith != 1) return BEVOPS_NOT_SUPPORTED;
  if (out_dtype != BEVOPS_F16 && out_dtype != BEVOPS_F32) return BEVOPS_NOT_SUPPORTED;
  if (H0 > (1 << 20) || W0 > (1 << 20) || Hp > (1 << 20) || Wp > (1 << 20)) return BEVOPS_NOT_SUPPORTED;
  if (N > 65535 || (Hp + kTH - 1) / kTH > 65535) return BEVOPS_NOT_SUPPORTED;
  if (reinterpret_cast<uintptr_t>(output) & (out_dtype == BEVOPS_F16 ? 1u : 3u)) return BEVOPS_BAD_PARAM;
  Geometry g;
  g.H0 = H0, g.W0 = W0, g.Hs = Hs, g.Ws = Ws, g.Hp = Hp, g.Wp = Wp, g.oy = oy, g.ox = ox;
  {
#pragma clang fp contract(off)
    g.sx = 1.0 / ((double)Ws / (double)W0);
    g.sy = 1.0 / ((double)Hs / (double)H0);
  }
  g.area = W0 == 2 * Ws && H0 == 2 * Hs;
  g.winW = max_window(Wp, kTW, ox, Ws, g.sx, W0);
  g.winH = max_window(Hp, kTH, oy, Hs, g.sy, H0);
  g.srcPitch = (g.winW * 3 + 3 + 3) & ~3;              // + up to 3 bytes in front of an unaligned row start
  const size_t mid = arith == 0 ? sizeof(unsigned short) : sizeof(float);
  const size_t lds = (size_t)g.winH * g.srcPitch + (g.area ? 0 : (size_t)g.winH * kTW * 3 * mid);
  if (lds > kMaxLds) return BEVOPS_NOT_SUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (arith == 0)
    return out_dtype == BEVOPS_F16 ? launch<0, __half>(images, output, N, g, nm, to_rgb, channels_last, lds, st)
                                   : launch<0, float>(images, output, N, g, nm, to_rgb, channels_last, lds, st);
  return out_dtype == BEVOPS_F16 ? launch<1, __half>(images, output, N, g, nm, to_rgb, channels_last, lds, st)
                                 : launch<1, float>(images, output, N, g, nm, to_rgb, channels_last, lds, st);
}
