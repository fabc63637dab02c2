// BEVFormer tiny / small camera front end (design/image_scale.md; not a reference plugin): the test pipeline
// NormalizeMultiviewImage -> RandomScaleImageMultiViewImage(scales=[s]) -> PadMultiViewImage(32) -> format bundle
// (configs/bevformer/bevformer_tiny.py:19-20,229-231, bevformer_small.py:19,231-233; third_party/bev_mmdet3d/datasets/
// pipelines/transform_3d.py:404-438) as ONE launch: raw [N, H0, W0, 3] uint8 / fp32 BGR -> every tap normalised as
// csrc/image.hip does it -> float32 bilinear resize in the operation order of cv::resize(INTER_LINEAR) written from its
// specification (coordinates in double, one rounding to float32, the horizontal pass first, two products and one sum per
// pass, no contraction; an exact 2 : 1 in both axes takes the four-tap area form) -> zero padding to [Hp, Wp] -> fp16 /
// fp32 planes or channels-last.  Parity against cv2 itself is UNPINNED (the library is not available to the tests); the
// contract is the restatement in tests/util_image_scale.py, which this kernel equals bit for bit.
//
// One block = one 64 x 8 tile of the padded output of one image.  uint8 input: the tile's source window (the rows and
// columns its taps touch) is staged in LDS with aligned dword loads; the horizontal pass writes its float32 result for
// every window row into LDS as [row][64 x 3] interleaved, the vertical pass reads that: with lane = column (planes) or
// lane = element of the row (channels-last) both are free of bank conflicts and both store consecutive addresses.
#include <math.h>

#include "common.h"

namespace bevops {
namespace {

constexpr int kTW = 64, kTH = 8, kThreads = 256;   // tile of padded output pixels; 4 rows of 64 lanes per pass step
constexpr int kRowGroups = kThreads / kTW;
constexpr size_t kMaxLds = 64 * 1024;

struct Geometry {
  int H0, W0, Hs, Ws, Hp, Wp;   // source, resized and padded size
  int winW, winH;               // largest source window of a tile, in pixels / rows
  int srcPitch;                 // LDS row pitch of the staged uint8 window in bytes (a multiple of 4)
  int area;                     // 2 : 1 in both axes
  double sx, sy;                // 1 / (out / in) per axis
};

struct Norm {
  float m0, m1, m2, i0, i1, i2;
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

inline int max_window(int out, int tile, double scale, int in) {
  int w = 0;
  for (int t = 0; t < out; t += tile) {
    int lo, hi;
    window(t, (t + tile < out ? t + tile : out) - t, scale, in, &lo, &hi);
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

template <typename In, typename Out, bool NHWC>
__global__ __launch_bounds__(kThreads) void image_scale_kernel(const In *__restrict__ img, Out *__restrict__ out,
                                                               Geometry g, Norm nm, int to_rgb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool U8IN = sizeof(In) == 1;
  const int tid = threadIdx.x, lane = tid & (kTW - 1), j = tid / kTW;
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH, n = blockIdx.z;
  const int tw = max(0, min(kTW, g.Ws - tx0)), th = max(0, min(kTH, g.Hs - ty0));   // resized pixels in the tile
  const int pw = min(kTW, g.Wp - tx0), ph = min(kTH, g.Hp - ty0);                    // padded pixels in the tile

  unsigned char *src = smem;                                                         // [winH][srcPitch] (uint8 input)
  float *mid = reinterpret_cast<float *>(smem + (U8IN ? (size_t)g.winH * g.srcPitch : 0));   // [winH][kTW * 3]

  // the tile's source window, clamped to the images and to the LDS allocation
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  if (tw > 0 && th > 0) {
    window(tx0, tw, g.sx, g.W0, &x0, &x1);
    window(ty0, th, g.sy, g.H0, &y0, &y1);
    x0 = max(0, min(x0, g.W0)), x1 = max(x0, min(x1, min(g.W0, x0 + g.winW)));
    y0 = max(0, min(y0, g.H0)), y1 = max(y0, min(y1, min(g.H0, y0 + g.winH)));
  }
  const int ww = x1 - x0, wh = y1 - y0;
  const In *base = img + (size_t)n * g.H0 * g.W0 * 3;

  // ---- stage (uint8): one wave per window row, aligned dwords (a dword that holds one byte of the image lies in that
  // byte's page, so the up to 3 bytes in front of / behind an unaligned row are readable)
  if constexpr (U8IN) {
    for (int r = j; r < wh; r += kRowGroups) {
      const uint8_t *row = reinterpret_cast<const uint8_t *>(base) + ((size_t)(y0 + r) * g.W0 + x0) * 3;
      const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(row) & 3u);
      const int nd = ww > 0 ? (int)(shift + ww * 3 + 3) >> 2 : 0;   // every dword holds at least one byte of the row
      const unsigned *p = reinterpret_cast<const unsigned *>(row - shift);
      unsigned *d = reinterpret_cast<unsigned *>(src + (size_t)r * g.srcPitch);
      for (int i = lane; i < nd; i += kTW) d[i] = p[i];
    }
    __syncthreads();
  }

  // a window row as the taps read it: LDS bytes behind the row's alignment shift (uint8) or the global row (fp32)
  auto row_of = [&](int r) {
    if constexpr (U8IN) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(base) + ((size_t)(y0 + r) * g.W0 + x0) * 3;
      return src + (size_t)r * g.srcPitch + (unsigned)(a & 3u);
    } else {
      return base + ((size_t)(y0 + r) * g.W0 + x0) * 3;
    }
  };
  // normalised tap (window column c, OUTPUT channel ch) of such a row
  auto fetch = [&](auto row, int c, int ch) -> float {
    const int sc = to_rgb ? 2 - ch : ch;
    const float mean = ch == 0 ? nm.m0 : (ch == 1 ? nm.m1 : nm.m2), inv = ch == 0 ? nm.i0 : (ch == 1 ? nm.i1 : nm.i2);
    return normalise((float)row[c * 3 + sc], mean, inv);
  };

  // ---- horizontal pass over every window row (general path): lane = tile column
  if (!g.area) {
    if (lane < tw) {
      int i0, i1;
      float f;
      tap(tx0 + lane, g.sx, g.W0, &i0, &i1, &f);
      i0 = max(0, min(i0 - x0, ww - 1)), i1 = max(0, min(i1 - x0, ww - 1));
      const float w0 = one_minus(f);
      for (int r = j; r < wh; r += kRowGroups) {
        const auto row = row_of(r);
        float *m = mid + (size_t)r * (kTW * 3) + lane * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) m[ch] = lerp2(fetch(row, i0, ch), fetch(row, i1, ch), w0, f);
      }
    }
    __syncthreads();
  }

  // ---- vertical pass (or the area form), padding, store: three (column, channel) slots per lane and row
  for (int jj = j; jj < ph; jj += kRowGroups) {
    const int y = ty0 + jj;
    int r0 = 0, r1 = 0;
    float fy = 0.f, wy = 1.f;
    if (jj < th) {
      if (g.area) {
        r0 = max(0, min(2 * jj, wh - 1)), r1 = max(0, min(2 * jj + 1, wh - 1));
      } else {
        tap(y, g.sy, g.H0, &r0, &r1, &fy);
        r0 = max(0, min(r0 - y0, wh - 1)), r1 = max(0, min(r1 - y0, wh - 1));
        wy = one_minus(fy);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = lane + kTW * k;                       // channels-last: element of the tile row
      const int col = NHWC ? e / 3 : lane, ch = NHWC ? e - col * 3 : k;
      float v = 0.f;
      if (jj < th && col < tw) {
        if (g.area) {
          const int c0 = max(0, min(2 * col, ww - 1)), c1 = max(0, min(2 * col + 1, ww - 1));
          const auto up = row_of(r0), low = row_of(r1);
          v = area4(fetch(up, c0, ch), fetch(up, c1, ch), fetch(low, c0, ch), fetch(low, c1, ch));
        } else {
          v = lerp2(mid[(size_t)r0 * (kTW * 3) + col * 3 + ch], mid[(size_t)r1 * (kTW * 3) + col * 3 + ch], wy, fy);
        }
      }
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

template <typename In, typename Out>
int launch(const void *img, void *out, int N, const Geometry &g, const Norm &nm, int to_rgb, int channels_last,
           size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)((g.Wp + kTW - 1) / kTW), (unsigned)((g.Hp + kTH - 1) / kTH), (unsigned)N);
  if (channels_last)
    hipLaunchKernelGGL((image_scale_kernel<In, Out, true>), grid, dim3(kThreads), lds, st, (const In *)img, (Out *)out, g,
                       nm, to_rgb);
  else
    hipLaunchKernelGGL((image_scale_kernel<In, Out, false>), grid, dim3(kThreads), lds, st, (const In *)img, (Out *)out, g,
                       nm, to_rgb);
  return launch_status();
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_image_normalize_resize_pad(int in_dtype, const void *images, int out_dtype, void *output, int N,
                                                 int H0, int W0, int Hs, int Ws, int Hp, int Wp, const double *mean_host,
                                                 const double *std_host, int to_rgb, int channels_last, void *stream) {
  if (!images || !output || !mean_host || !std_host) return BEVOPS_BAD_PARAM;
  if (N <= 0 || H0 <= 0 || W0 <= 0 || Hs <= 0 || Ws <= 0 || Hp < Hs || Wp < Ws) return BEVOPS_BAD_PARAM;
  float inv[3], mean[3];
  for (int c = 0; c < 3; ++c) {
    if (!(std_host[c] > 0.0)) return BEVOPS_BAD_PARAM;
    inv[c] = (float)(1.0 / std_host[c]);   // mmcv.imnormalize: stdinv = 1 / float64(std), applied in float32
    mean[c] = (float)mean_host[c];
  }
  const Norm nm = {mean[0], mean[1], mean[2], inv[0], inv[1], inv[2]};
  const bool u8 = in_dtype == BEVOPS_U8, f32in = in_dtype == BEVOPS_F32;
  if (!u8 && !f32in) return BEVOPS_NOT_SUPPORTED;
  if (out_dtype != BEVOPS_F16 && out_dtype != BEVOPS_F32) return BEVOPS_NOT_SUPPORTED;
  if (H0 > (1 << 20) || W0 > (1 << 20) || Hp > (1 << 20) || Wp > (1 << 20)) return BEVOPS_NOT_SUPPORTED;
  if (N > 65535 || (Hp + kTH - 1) / kTH > 65535) return BEVOPS_NOT_SUPPORTED;
  if (reinterpret_cast<uintptr_t>(output) & (out_dtype == BEVOPS_F16 ? 1u : 3u)) return BEVOPS_BAD_PARAM;
  if (f32in && (reinterpret_cast<uintptr_t>(images) & 3u)) return BEVOPS_BAD_PARAM;
  Geometry g;
  g.H0 = H0, g.W0 = W0, g.Hs = Hs, g.Ws = Ws, g.Hp = Hp, g.Wp = Wp;
  {
#pragma clang fp contract(off)
    g.sx = 1.0 / ((double)Ws / (double)W0);
    g.sy = 1.0 / ((double)Hs / (double)H0);
  }
  g.area = W0 == 2 * Ws && H0 == 2 * Hs;
  g.winW = max_window(Ws, kTW, g.sx, W0);
  g.winH = max_window(Hs, kTH, g.sy, H0);
  g.srcPitch = u8 ? (g.winW * 3 + 3 + 3) & ~3 : 0;     // + up to 3 bytes in front of an unaligned row start
  const size_t lds = (size_t)g.winH * g.srcPitch + (g.area ? 0 : (size_t)g.winH * kTW * 3 * sizeof(float));
  if (lds > kMaxLds) return BEVOPS_NOT_SUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (out_dtype == BEVOPS_F16)
    return u8 ? launch<uint8_t, __half>(images, output, N, g, nm, to_rgb, channels_last, lds, st)
              : launch<float, __half>(images, output, N, g, nm, to_rgb, channels_last, lds, st);
  return u8 ? launch<uint8_t, float>(images, output, N, g, nm, to_rgb, channels_last, lds, st)
            : launch<float, float>(images, output, N, g, nm, to_rgb, channels_last, lds, st);
}
