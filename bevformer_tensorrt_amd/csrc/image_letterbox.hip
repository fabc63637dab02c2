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
// The tile / LDS scheme, the shared device pieces and the host set-up are csrc/image_resample.h.  This kernel's own:
// the paste at (oy, ox), raw taps (arith 0: the horizontal pass's D >> 4 lies in LDS as uint16, exact; arith 1: float32),
// the resized value and the pad value normalised last.  A tile that lies in the padding alone stages nothing.
#include "image_resample.h"

using namespace bevops;
using namespace bevops::resample;

namespace {

template <int ARITH, typename Out, bool NHWC>
__global__ __launch_bounds__(kThreads) void image_letterbox_kernel(const uint8_t *__restrict__ img, Out *__restrict__ out,
                                                                   Geometry g, Norm nm, int to_rgb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Mid = typename std::conditional<ARITH == 0, unsigned short, float>::type;
  const int tid = threadIdx.x, lane = tid & (kTW - 1), j = tid / kTW;
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH, n = blockIdx.z;
  int dx0, dx1, dy0, dy1;                                           // resized pixels in the tile
  tile_span(tx0, kTW, g.ox, g.Ws, &dx0, &dx1);
  tile_span(ty0, kTH, g.oy, g.Hs, &dy0, &dy1);
  const bool inside = dx1 > dx0 && dy1 > dy0;                       // (else: a tile of padding alone)

  unsigned char *src = smem;                                                      // [winH][srcPitch]
  Mid *mid = reinterpret_cast<Mid *>(smem + (size_t)g.winH * g.srcPitch);         // [winH][kTW * 3]
  const Window w = tile_window(g, inside, dx0, dx1 - dx0, dy0, dy1 - dy0);
  const uint8_t *base = img + (size_t)n * g.H0 * g.W0 * 3;
  stage_window(base, g, w, src, lane, j);
  __syncthreads();

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
      i0 = max(0, min(i0 - w.x0, w.ww - 1)), i1 = max(0, min(i1 - w.x0, w.ww - 1));
      const float w0 = one_minus(f);
      int a0, a1;
      fixed_weights(f, &a0, &a1);
      for (int r = j; r < w.wh; r += kRowGroups) {
        const unsigned char *row = window_row(base, g, w, src, r);
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
  const int pw = min(kTW, g.Wp - tx0), ph = min(kTH, g.Hp - ty0);   // padded pixels in the tile
  for (int jj = j; jj < ph; jj += kRowGroups) {
    const int y = ty0 + jj, dy = y - g.oy;
    const bool row_in = inside && dy >= dy0 && dy < dy1;
    int r0 = 0, r1 = 0, b0 = 0, b1 = 0;
    float fy = 0.f, wy = 1.f;
    if (row_in) {
      if (g.area) {
        r0 = max(0, min(2 * dy - w.y0, w.wh - 1)), r1 = max(0, min(2 * dy + 1 - w.y0, w.wh - 1));
      } else {
        tap(dy, g.sy, g.H0, &r0, &r1, &fy);
        r0 = max(0, min(r0 - w.y0, w.wh - 1)), r1 = max(0, min(r1 - w.y0, w.wh - 1));
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
          const int c0 = max(0, min(2 * d - w.x0, w.ww - 1)), c1 = max(0, min(2 * d + 1 - w.x0, w.ww - 1));
          const unsigned char *up = window_row(base, g, w, src, r0), *low = window_row(base, g, w, src, r1);
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
      if (col < pw) store_slot<Out, NHWC>(out, g, n, y, tx0, e, col, ch, v);
    }
  }
}

template <int ARITH>
int run(int out_dtype, const void *img, void *out, int N, const Geometry &g, const Norm &nm, int to_rgb,
        int channels_last, size_t lds, void *stream) {
  if (out_dtype == BEVOPS_F16)
    return launch<uint8_t, __half>(image_letterbox_kernel<ARITH, __half, false>, image_letterbox_kernel<ARITH, __half, true>,
                                   img, out, N, g, nm, to_rgb, channels_last, lds, stream);
  return launch<uint8_t, float>(image_letterbox_kernel<ARITH, float, false>, image_letterbox_kernel<ARITH, float, true>, img,
                                out, N, g, nm, to_rgb, channels_last, lds, stream);
}

}  // namespace

extern "C" int bevops_image_letterbox(int arith, const void *images, int out_dtype, void *output, int N, int H0, int W0,
                                      int Hs, int Ws, int Hp, int Wp, int oy, int ox, const double *pad_host,
                                      const double *mean_host, const double *std_host, int to_rgb, int channels_last,
                                      void *stream) {
  if (!images || !output || !pad_host || !mean_host || !std_host) return BEVOPS_BAD_PARAM;
  if (N <= 0 || H0 <= 0 || W0 <= 0 || Hs <= 0 || Ws <= 0 || Hp <= 0 || Wp <= 0) return BEVOPS_BAD_PARAM;
  if (oy < 0 || ox < 0 || (long long)oy + Hs > Hp || (long long)ox + Ws > Wp) return BEVOPS_BAD_PARAM;
  Norm nm;
  if (int st = make_norm(mean_host, std_host, pad_host, to_rgb, &nm)) return st;
  if (arith != 0 && arith != 1) return BEVOPS_NOT_SUPPORTED;
  if (int st = check_output(out_dtype, output, N, H0, W0, Hp, Wp)) return st;
  Geometry g;
  size_t lds;
  const size_t mid = arith == 0 ? sizeof(unsigned short) : sizeof(float);
  if (int st = make_geometry(H0, W0, Hs, Ws, Hp, Wp, oy, ox, true, mid, &g, &lds)) return st;
  return arith == 0 ? run<0>(out_dtype, images, output, N, g, nm, to_rgb, channels_last, lds, stream)
                    : run<1>(out_dtype, images, output, N, g, nm, to_rgb, channels_last, lds, stream);
}
