// What the two bilinear camera front ends share (design/image_scale.md: the tile / LDS scheme; design/letterbox.md: the
// paste, the 8-bit arithmetic, and why there are two kernels): csrc/image_scale.hip and csrc/image_letterbox.hip both
// take raw [N, H0, W0, 3] images -> bilinear resize to [Hs, Ws] in the operation order of cv::resize(INTER_LINEAR)
// written from its specification (coordinates in double, one rounding to float32, the horizontal pass first; an exact
// 2 : 1 in both axes takes the four-tap area form) -> paste at (oy, ox) into a constant [Hp, Wp] canvas -> fp16 / fp32
// planes or channels-last.  Here: the tile constants, Geometry / Norm, the tap and window functions, the arithmetic
// leaves, the device pieces of the kernels (window set-up, staging, row accessor, store loop) and the host set-up.
// Each file keeps its own __global__ function: the horizontal pass and the value of an output element, where the two
// differ (normalisation at fetch / last, fixed point / float32, the paste).  Both are bit-exact against a numpy
// restatement under tests/, so each `#pragma clang fp contract(off)` stays with the operation it protects.
//
// One block = one 64 x 8 tile of the PADDED output of one image.  uint8 input: the source window of the tile's resized
// pixels (the rows and columns their taps touch) is staged in LDS with aligned dword loads; the horizontal pass writes
// its result for every window row into LDS as [row][64 x 3] interleaved, the vertical pass reads that: with lane =
// column (planes) or lane = element of the row (channels-last) both are free of bank conflicts and both store
// consecutive addresses.  A tile that lies in the padding alone stages nothing.
//
// `to_out` is also what csrc/image.hip and csrc/image_prepare.hip take from here, and all they take.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"

namespace bevops {

// float -> output type as its OWN rounding step: a plain cast lets the compiler fold the multiply and
// the conversion into one v_fma_mixlo_f16 (single rounding of the exact product), while the
// reference multiplies in float32 and converts afterwards
__device__ __forceinline__ float to_out(float v, float *) { return v; }
__device__ __forceinline__ __half to_out(float v, __half *) {
  unsigned r;
  asm("v_cvt_f16_f32 %0, %1" : "=v"(r) : "v"(v));
  return __ushort_as_half((unsigned short)r);
}

namespace resample {

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

// At off = 0 the spans are [t, min(t + tile, out)) for t < out and empty behind: the tiles a plain walk over the
// resized axis visits, so an entry that pastes at (0, 0) gets the winW / winH (and with them the BEVOPS_NOT_SUPPORTED
// boundary) it had when it walked the resized axis itself.
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

// ---------------------------------------------------------------- device pieces of the two kernels
struct Window {
  int x0, y0, ww, wh;   // first source column / row of the tile's window, its width and height
};

// the source window of the tile's resized pixels [dx0, dx0 + nx) x [dy0, dy0 + ny), clamped to the image and to the LDS
// allocation; a tile without resized pixels (`inside` false) has an empty one
__device__ __forceinline__ Window tile_window(const Geometry &g, bool inside, int dx0, int nx, int dy0, int ny) {
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  if (inside) {
    window(dx0, nx, g.sx, g.W0, &x0, &x1);
    window(dy0, ny, g.sy, g.H0, &y0, &y1);
    x0 = max(0, min(x0, g.W0)), x1 = max(x0, min(x1, min(g.W0, x0 + g.winW)));
    y0 = max(0, min(y0, g.H0)), y1 = max(y0, min(y1, min(g.H0, y0 + g.winH)));
  }
  return {x0, y0, x1 - x0, y1 - y0};
}

// stage a uint8 window into src [winH][srcPitch]: one wave per window row, aligned dwords (a dword that holds one byte of
// the image lies in that byte's page, so the up to 3 bytes in front of / behind an unaligned row are readable)
__device__ __forceinline__ void stage_window(const uint8_t *base, const Geometry &g, const Window &w, unsigned char *src,
                                             int lane, int j) {
  for (int r = j; r < w.wh; r += kRowGroups) {
    const uint8_t *row = base + ((size_t)(w.y0 + r) * g.W0 + w.x0) * 3;
    const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(row) & 3u);
    const int nd = w.ww > 0 ? (int)(shift + w.ww * 3 + 3) >> 2 : 0;   // every dword holds at least one byte of the row
    const unsigned *p = reinterpret_cast<const unsigned *>(row - shift);
    unsigned *d = reinterpret_cast<unsigned *>(src + (size_t)r * g.srcPitch);
    for (int i = lane; i < nd; i += kTW) d[i] = p[i];
  }
}

// a window row as the taps read it: LDS bytes behind the row's alignment shift (uint8) or the global row (fp32)
__device__ __forceinline__ const unsigned char *window_row(const uint8_t *base, const Geometry &g, const Window &w,
                                                           const unsigned char *src, int r) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(base) + ((size_t)(w.y0 + r) * g.W0 + w.x0) * 3;
  return src + (size_t)r * g.srcPitch + (unsigned)(a & 3u);
}
__device__ __forceinline__ const float *window_row(const float *base, const Geometry &g, const Window &w,
                                                   const unsigned char *, int r) {
  return base + ((size_t)(w.y0 + r) * g.W0 + w.x0) * 3;
}

// one (column, channel) slot of the store loop: planes -- lane = column; channels-last -- lane = element e of the
// 192-element tile row; either way a wave stores 64 consecutive elements
template <typename Out, bool NHWC>
__device__ __forceinline__ void store_slot(Out *__restrict__ out, const Geometry &g, int n, int y, int tx0, int e, int col,
                                           int ch, float v) {
  if constexpr (NHWC) {
    out[(((size_t)n * g.Hp + y) * g.Wp + tx0) * 3 + e] = to_out(v, (Out *)nullptr);
  } else {
    out[(((size_t)n * 3 + ch) * g.Hp + y) * g.Wp + tx0 + col] = to_out(v, (Out *)nullptr);
  }
}

// ---------------------------------------------------------------- host, shared by both entries
// mean, 1 / std and pad (nullptr: zeros) per OUTPUT channel; a std that is not positive is BEVOPS_BAD_PARAM
inline int make_norm(const double *mean_host, const double *std_host, const double *pad_host, int to_rgb, Norm *nm) {
  float inv[3], mean[3], pad[3];
  for (int c = 0; c < 3; ++c) {
    if (!(std_host[c] > 0.0)) return BEVOPS_BAD_PARAM;
    inv[c] = (float)(1.0 / std_host[c]);   // mmcv.imnormalize: stdinv = 1 / float64(std), applied in float32
    mean[c] = (float)mean_host[c];
    pad[c] = pad_host ? (float)pad_host[to_rgb ? 2 - c : c] : 0.f;   // the canvas is filled before the channel swap
  }
  *nm = {mean[0], mean[1], mean[2], inv[0], inv[1], inv[2], pad[0], pad[1], pad[2]};
  return BEVOPS_SUCCESS;
}

// the output type, the sizes the index arithmetic and the grid take, the output's alignment
inline int check_output(int out_dtype, const void *output, int N, int H0, int W0, int Hp, int Wp) {
  if (out_dtype != BEVOPS_F16 && out_dtype != BEVOPS_F32) return BEVOPS_NOT_SUPPORTED;
  if (H0 > (1 << 20) || W0 > (1 << 20) || Hp > (1 << 20) || Wp > (1 << 20)) return BEVOPS_NOT_SUPPORTED;
  if (N > 65535 || (Hp + kTH - 1) / kTH > 65535) return BEVOPS_NOT_SUPPORTED;
  if (reinterpret_cast<uintptr_t>(output) & (out_dtype == BEVOPS_F16 ? 1u : 3u)) return BEVOPS_BAD_PARAM;
  return BEVOPS_SUCCESS;
}

// the geometry and the LDS bytes of one call; u8: the window is staged; mid: bytes per element of the horizontal
// pass's result.  A tile whose window and rows exceed 64 KiB of LDS is BEVOPS_NOT_SUPPORTED.
inline int make_geometry(int H0, int W0, int Hs, int Ws, int Hp, int Wp, int oy, int ox, bool u8, size_t mid, Geometry *g,
                         size_t *lds) {
  g->H0 = H0, g->W0 = W0, g->Hs = Hs, g->Ws = Ws, g->Hp = Hp, g->Wp = Wp, g->oy = oy, g->ox = ox;
  {
#pragma clang fp contract(off)
    g->sx = 1.0 / ((double)Ws / (double)W0);
    g->sy = 1.0 / ((double)Hs / (double)H0);
  }
  g->area = W0 == 2 * Ws && H0 == 2 * Hs;
  g->winW = max_window(Wp, kTW, ox, Ws, g->sx, W0);
  g->winH = max_window(Hp, kTH, oy, Hs, g->sy, H0);
  g->srcPitch = u8 ? (g->winW * 3 + 3 + 3) & ~3 : 0;   // + up to 3 bytes in front of an unaligned row start
  *lds = (size_t)g->winH * g->srcPitch + (g->area ? 0 : (size_t)g->winH * kTW * 3 * mid);
  return *lds > kMaxLds ? BEVOPS_NOT_SUPPORTED : BEVOPS_SUCCESS;
}

template <typename In, typename Out>
using Kernel = void (*)(const In *, Out *, Geometry, Norm, int);

// one of a kernel's two layout instances over the tile grid of the padded output
template <typename In, typename Out>
int launch(Kernel<In, Out> planes, Kernel<In, Out> nhwc, const void *img, void *out, int N, const Geometry &g,
           const Norm &nm, int to_rgb, int channels_last, size_t lds, void *stream) {
  const dim3 grid((unsigned)((g.Wp + kTW - 1) / kTW), (unsigned)((g.Hp + kTH - 1) / kTH), (unsigned)N);
  hipLaunchKernelGGL(channels_last ? nhwc : planes, grid, dim3(kThreads), lds, static_cast<hipStream_t>(stream),
                     (const In *)img, (Out *)out, g, nm, to_rgb);
  return launch_status();
}

}  // namespace resample
}  // namespace bevops
