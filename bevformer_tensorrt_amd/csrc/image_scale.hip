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
// The tile / LDS scheme, the shared device pieces and the host set-up are csrc/image_resample.h.  This kernel's own:
// every tap normalised when it is fetched (uint8 from the staged window, fp32 from global memory), the resized image at
// (0, 0) of the padded output, a literal zero behind it.
#include "image_resample.h"

using namespace bevops;
using namespace bevops::resample;

namespace {

template <typename In, typename Out, bool NHWC>
__global__ __launch_bounds__(kThreads) void image_scale_kernel(const In *__restrict__ img, Out *__restrict__ out,
                                                               Geometry g, Norm nm, int to_rgb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool U8IN = sizeof(In) == 1;
  const int tid = threadIdx.x, lane = tid & (kTW - 1), j = tid / kTW;
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH, n = blockIdx.z;
  const int tw = max(0, min(kTW, g.Ws - tx0)), th = max(0, min(kTH, g.Hs - ty0));   // resized pixels in the tile

  unsigned char *src = smem;                                                         // [winH][srcPitch] (uint8 input)
  float *mid = reinterpret_cast<float *>(smem + (U8IN ? (size_t)g.winH * g.srcPitch : 0));   // [winH][kTW * 3]
  const Window w = tile_window(g, tw > 0 && th > 0, tx0, tw, ty0, th);
  const In *base = img + (size_t)n * g.H0 * g.W0 * 3;
  if constexpr (U8IN) {
    stage_window(base, g, w, src, lane, j);
    __syncthreads();
  }

  // normalised tap (window column c, OUTPUT channel ch) of a window row
  auto fetch = [&](const In *row, int c, int ch) -> float {
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
      i0 = max(0, min(i0 - w.x0, w.ww - 1)), i1 = max(0, min(i1 - w.x0, w.ww - 1));
      const float w0 = one_minus(f);
      for (int r = j; r < w.wh; r += kRowGroups) {
        const In *row = window_row(base, g, w, src, r);
        float *m = mid + (size_t)r * (kTW * 3) + lane * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) m[ch] = lerp2(fetch(row, i0, ch), fetch(row, i1, ch), w0, f);
      }
    }
    __syncthreads();
  }

  // ---- vertical pass (or the area form), padding, store: three (column, channel) slots per lane and row
  const int pw = min(kTW, g.Wp - tx0), ph = min(kTH, g.Hp - ty0);                    // padded pixels in the tile
  for (int jj = j; jj < ph; jj += kRowGroups) {
    const int y = ty0 + jj;
    int r0 = 0, r1 = 0;
    float fy = 0.f, wy = 1.f;
    if (jj < th) {
      if (g.area) {
        r0 = max(0, min(2 * jj, w.wh - 1)), r1 = max(0, min(2 * jj + 1, w.wh - 1));
      } else {
        tap(y, g.sy, g.H0, &r0, &r1, &fy);
        r0 = max(0, min(r0 - w.y0, w.wh - 1)), r1 = max(0, min(r1 - w.y0, w.wh - 1));
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
          const int c0 = max(0, min(2 * col, w.ww - 1)), c1 = max(0, min(2 * col + 1, w.ww - 1));
          const In *up = window_row(base, g, w, src, r0), *low = window_row(base, g, w, src, r1);
          v = area4(fetch(up, c0, ch), fetch(up, c1, ch), fetch(low, c0, ch), fetch(low, c1, ch));
        } else {
          v = lerp2(mid[(size_t)r0 * (kTW * 3) + col * 3 + ch], mid[(size_t)r1 * (kTW * 3) + col * 3 + ch], wy, fy);
        }
      }
      if (col < pw) store_slot<Out, NHWC>(out, g, n, y, tx0, e, col, ch, v);
    }
  }
}

template <typename In>
int run(int out_dtype, const void *img, void *out, int N, const Geometry &g, const Norm &nm, int to_rgb,
        int channels_last, size_t lds, void *stream) {
  if (out_dtype == BEVOPS_F16)
    return launch<In, __half>(image_scale_kernel<In, __half, false>, image_scale_kernel<In, __half, true>, img, out, N, g,
                              nm, to_rgb, channels_last, lds, stream);
  return launch<In, float>(image_scale_kernel<In, float, false>, image_scale_kernel<In, float, true>, img, out, N, g, nm,
                           to_rgb, channels_last, lds, stream);
}

}  // namespace

extern "C" int bevops_image_normalize_resize_pad(int in_dtype, const void *images, int out_dtype, void *output, int N,
                                                 int H0, int W0, int Hs, int Ws, int Hp, int Wp, const double *mean_host,
                                                 const double *std_host, int to_rgb, int channels_last, void *stream) {
  if (!images || !output || !mean_host || !std_host) return BEVOPS_BAD_PARAM;
  if (N <= 0 || H0 <= 0 || W0 <= 0 || Hs <= 0 || Ws <= 0 || Hp < Hs || Wp < Ws) return BEVOPS_BAD_PARAM;
  Norm nm;
  if (int st = make_norm(mean_host, std_host, nullptr, to_rgb, &nm)) return st;
  const bool u8 = in_dtype == BEVOPS_U8, f32in = in_dtype == BEVOPS_F32;
  if (!u8 && !f32in) return BEVOPS_NOT_SUPPORTED;
  if (int st = check_output(out_dtype, output, N, H0, W0, Hp, Wp)) return st;
  if (f32in && (reinterpret_cast<uintptr_t>(images) & 3u)) return BEVOPS_BAD_PARAM;
  Geometry g;
  size_t lds;
  if (int st = make_geometry(H0, W0, Hs, Ws, Hp, Wp, 0, 0, u8, sizeof(float), &g, &lds)) return st;
  return u8 ? run<uint8_t>(out_dtype, images, output, N, g, nm, to_rgb, channels_last, lds, stream)
            : run<float>(out_dtype, images, output, N, g, nm, to_rgb, channels_last, lds, stream);
}
