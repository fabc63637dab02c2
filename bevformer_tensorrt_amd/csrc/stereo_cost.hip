// BEVStereo's temporal-stereo cost volume (DepthNet.gen_grid + calculate_cost_volumn, third_party/bev_mmdet3d/models/
// necks/view_transformer.py:613-678) as ONE launch: no warped feature is written, no workspace, no atomics.
//
//   cost[n, :, h, w] = softmax_d -( sum_c |curr[n,h,w,c] - warp(prev)[n,d,h,w,c]|  +  bias [gate == 0] )
//
// warp = grid_sample(bilinear, zeros padding, align_corners=True); gate = the warped value of channel C - 4 (channel 0
// of the LAST group of four, what the reference's loop variable holds when its loop ends), tested for exact equality
// with zero and skipped when bias == 0.
//
// Mapping.  Block = 4 waves, pixel tile = 4 consecutive pixels of the flattened [n, Hc, Wc] index, ONE PIXEL PER WAVE.
// Lane l owns channels 4 l .. 4 l + 3 of a 256-channel chunk (8 bytes per corner, a wave reads a corner's 256 channels
// as one 512-byte line); the pixel's curr values of chunk 0 stay in registers, further chunks (C > 256) are re-read.
// Lanes 0 .. 63 first compute (or read) the grid of hypotheses 2 l, 2 l + 1 and leave the source positions in LDS; the
// wave then walks d = 0 .. D - 1: position -> SGPRs (readfirstlane), so corner validity and the address base are wave-
// uniform; four 8-byte loads; blend and |difference| in fp32; a butterfly sum over the 64 lanes.  Consecutive
// hypotheses of one pixel often share their corner rows (a depth step moves the sample by less than a pixel at range):
// the four corner vectors of chunk 0 are kept in registers and re-read only when floor(position) changes.  Lane d / 2
// keeps the cost of hypothesis d; the softmax over D (max, expf, butterfly sum, IEEE division) runs in those
// registers and lane l stores hypotheses 2 l, 2 l + 1 as one 32-bit word.  Columns D .. Dpad are written as zeros.
//
// fp32 operation order (every step one rounding unless it says fma):
//   ix = ((gx + 1) * 0.5) * (Wc - 1), iy likewise;  x0 = floor(ix), x1 = x0 + 1
//   nw = (x1 - ix) (y1 - iy), ne = (ix - x0) (y1 - iy), sw = (x1 - ix) (iy - y0), se = (ix - x0) (iy - y0)
//   v  = fma(se, p11, fma(sw, p10, fma(ne, p01, nw * p00)))       corners outside the image count as 0 and are not read
//   lane sum = (((|c0 - v0| + |c1 - v1|) + |c2 - v2|) + |c3 - v3|), added chunk after chunk; butterfly over xor 32 .. 1
//   cost += bias when gate == 0;  x = -cost;  m = max_d x;  e = expf(x - m);  s = butterfly sum of (e[2l] + e[2l+1]);
//   out = fp16(e / s)
#include <math.h>

#include "common.h"
#include "lss_pos.h"

namespace bevops {
namespace {

constexpr int kStBlock = 256;
constexpr int kStWaves = kStBlock / kWave;     // the pixel tile: one pixel per wave
constexpr int kStMaxD = 128;                   // two hypotheses per lane
constexpr int kStChunk = 4 * kWave;            // channels per pass of a wave
constexpr int kStConsts = 40;                  // floats per camera
constexpr int kStCvDown = 4;                   // stride of the stereo map: the grid is normalised by the image (4 Hc, 4 Wc),
                                               // as the reference hard-codes it (CV_DOWNSAMPLE in functions/stereo.py)

struct StereoArgs {
  const __half *prev, *curr;
  const float *grid, *consts, *xs, *ys, *ds;
  __half *out;
  int prev_pitch, curr_pitch, out_pitch;
  int hc, wc, c, d, dpad;
  int pixels;                                  // n * hc * wc
  float bias;
};

// One point of DepthNet.gen_grid, the reference's ops in its order, every product, sum and quotient rounded on its own.
// c: the camera's 40 floats [inverse(post_rots) 9 | post_trans 3 | k2s_R @ inverse(K) 9 | k2s_t 3 | K 9 |
// post_rots[:2,:2] 4 | post_trans[:2] 2 | pad].  wim1 = 4 Wc - 1, him1 = 4 Hc - 1 (the image the stride-4 map stands for).
__device__ __forceinline__ void stereo_grid_point(const float *__restrict__ c, float fx, float fy, float fd, float wim1,
                                                  float him1, float &gx, float &gy) {
  float x = sub_rn(fx, c[9]), y = sub_rn(fy, c[10]), z = sub_rn(fd, c[11]);
  lss_mat3(c, x, y, z);
  x = mul_rn(x, z);
  y = mul_rn(y, z);
  lss_mat3(c + 12, x, y, z);
  x = add_rn(x, c[21]);
  y = add_rn(y, c[22]);
  z = add_rn(z, c[23]);
  const bool behind = z < 1e-3f;
  lss_mat3(c + 24, x, y, z);
  const float px = lss_div(x, z), py = lss_div(y, z);
  const float qx = add_rn(add_rn(mul_rn(c[33], px), mul_rn(c[34], py)), c[37]);
  const float qy = add_rn(add_rn(mul_rn(c[35], px), mul_rn(c[36], py)), c[38]);
  gx = sub_rn(mul_rn(lss_div(qx, wim1), 2.f), 1.f);
  gy = sub_rn(mul_rn(lss_div(qy, him1), 2.f), 1.f);
  if (behind) gx = gy = -2.f;
}

__global__ __launch_bounds__(kStBlock) void stereo_grid_kernel(const float *__restrict__ consts, const float *__restrict__ xs,
                                                               const float *__restrict__ ys, const float *__restrict__ ds,
                                                               float *__restrict__ grid, int d_count, int hc, int wc,
                                                               long long total) {
  const long long i = (long long)blockIdx.x * kStBlock + threadIdx.x;
  if (i >= total) return;
  const int w = (int)(i % wc);
  const long long r = i / wc;
  const int h = (int)(r % hc);
  const long long r2 = r / hc;
  const int d = (int)(r2 % d_count);
  const int img = (int)(r2 / d_count);
  float gx, gy;
  stereo_grid_point(consts + (size_t)img * kStConsts, xs[w], ys[h], ds[d], (float)(kStCvDown * wc - 1),
                    (float)(kStCvDown * hc - 1), gx, gy);
  *reinterpret_cast<float2 *>(grid + (size_t)i * 2) = make_float2(gx, gy);
}

__device__ __forceinline__ float uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

struct Corners {
  u32x2 p00, p01, p10, p11;
};

// sum over the lane's four channels of |curr - blend|; g0 = the blend of the group's first channel
__device__ __forceinline__ float absdiff4(u32x2 cu, const Corners &k, float nw, float ne, float sw, float se, float &g0) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned sel = j >> 1;
    const bool hi = j & 1;
    const float a = hi ? h2f_hi(k.p00[sel]) : h2f_lo(k.p00[sel]);
    const float b = hi ? h2f_hi(k.p01[sel]) : h2f_lo(k.p01[sel]);
    const float c = hi ? h2f_hi(k.p10[sel]) : h2f_lo(k.p10[sel]);
    const float e = hi ? h2f_hi(k.p11[sel]) : h2f_lo(k.p11[sel]);
    const float v = fmaf(se, e, fmaf(sw, c, fmaf(ne, b, mul_rn(nw, a))));
    if (j == 0) g0 = v;
    const float cv = hi ? h2f_hi(cu[sel]) : h2f_lo(cu[sel]);
    s = add_rn(s, fabsf(sub_rn(cv, v)));
  }
  return s;
}

__device__ __forceinline__ float abs4(u32x2 cu) {     // the same sum against a zero warp
  return add_rn(add_rn(add_rn(add_rn(0.f, fabsf(h2f_lo(cu[0]))), fabsf(h2f_hi(cu[0]))), fabsf(h2f_lo(cu[1]))),
                fabsf(h2f_hi(cu[1])));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = kWave / 2; o >= 1; o >>= 1) v = add_rn(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = kWave / 2; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(kStBlock) void stereo_cost_kernel(StereoArgs p) {
  __shared__ float s_ix[kStWaves][kStMaxD];
  __shared__ float s_iy[kStWaves][kStMaxD];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long first = (long long)blockIdx.x * kStWaves + wave;
  const bool live = first < p.pixels;                 // a wave behind the last pixel repeats it and stores nothing
  const int pix = live ? (int)first : p.pixels - 1;
  const int w = pix % p.wc;
  const int r = pix / p.wc;
  const int h = r % p.hc;
  const int img = r / p.hc;
  const float wmax = (float)(p.wc - 1), hmax = (float)(p.hc - 1);

  // source positions of hypotheses 2 lane, 2 lane + 1
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int d = 2 * lane + j;
    if (d < p.d) {
      float gx, gy;
      if (p.grid) {
        const float2 g = *reinterpret_cast<const float2 *>(p.grid + ((((size_t)img * p.d + d) * p.hc + h) * p.wc + w) * 2);
        gx = g.x;
        gy = g.y;
      } else {
        stereo_grid_point(p.consts + (size_t)img * kStConsts, p.xs[w], p.ys[h], p.ds[d], (float)(kStCvDown * p.wc - 1),
                          (float)(kStCvDown * p.hc - 1), gx, gy);
      }
      s_ix[wave][d] = mul_rn(mul_rn(add_rn(gx, 1.f), 0.5f), wmax);
      s_iy[wave][d] = mul_rn(mul_rn(add_rn(gy, 1.f), 0.5f), hmax);
    }
  }
  __syncthreads();

  const int chunks = (p.c + kStChunk - 1) / kStChunk;
  const int gate_chunk = (p.c - 4) / kStChunk, gate_lane = ((p.c - 4) % kStChunk) / 4;
  const bool gated = p.bias != 0.f;
  const __half *curr_px = p.curr + (size_t)pix * p.curr_pitch;
  const __half *prev_img = p.prev + (size_t)img * p.hc * p.wc * p.prev_pitch;
  const int ch0 = 4 * lane;
  const bool act0 = ch0 < p.c;
  const u32x2 zero2 = {0u, 0u};
  const u32x2 curr0 = act0 ? *reinterpret_cast<const u32x2 *>(curr_px + ch0) : zero2;
  Corners keep = {zero2, zero2, zero2, zero2};
  float kx = __builtin_nanf(""), ky = __builtin_nanf("");      // floor(position) the kept corners belong to
  float c0 = 0.f, c1 = 0.f;                                    // costs of hypotheses 2 lane, 2 lane + 1

  for (int d = 0; d < p.d; ++d) {
    const float ix = uniform(s_ix[wave][d]), iy = uniform(s_iy[wave][d]);
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float x1 = add_rn(x0, 1.f), y1 = add_rn(y0, 1.f);
    // validity on the floats: a NaN or a huge position is outside and never becomes an address
    const bool vx0 = x0 >= 0.f && x0 <= wmax, vx1 = x1 >= 0.f && x1 <= wmax;
    const bool vy0 = y0 >= 0.f && y0 <= hmax, vy1 = y1 >= 0.f && y1 <= hmax;
    const bool any = (vx0 || vx1) && (vy0 || vy1);
    float part, g0 = 0.f, gate_v = 0.f;
    if (!any) {
      part = abs4(curr0);
      for (int ch = 1; ch < chunks; ++ch) {
        const int cc = ch * kStChunk + ch0;
        const u32x2 cu = cc < p.c ? *reinterpret_cast<const u32x2 *>(curr_px + cc) : zero2;
        part = add_rn(part, abs4(cu));
      }
    } else {
      const float tx1 = sub_rn(x1, ix), tx0 = sub_rn(ix, x0), ty1 = sub_rn(y1, iy), ty0 = sub_rn(iy, y0);
      const float nw = mul_rn(tx1, ty1), ne = mul_rn(tx0, ty1), sw = mul_rn(tx1, ty0), se = mul_rn(tx0, ty0);
      // valid coordinates only are converted; the others are never used
      const int xi0 = vx0 ? (int)x0 : 0, xi1 = vx1 ? (int)x1 : 0, yi0 = vy0 ? (int)y0 : 0, yi1 = vy1 ? (int)y1 : 0;
      const size_t o00 = ((size_t)yi0 * p.wc + xi0) * p.prev_pitch, o01 = ((size_t)yi0 * p.wc + xi1) * p.prev_pitch;
      const size_t o10 = ((size_t)yi1 * p.wc + xi0) * p.prev_pitch, o11 = ((size_t)yi1 * p.wc + xi1) * p.prev_pitch;
      if (x0 != kx || y0 != ky) {
        keep.p00 = (act0 && vx0 && vy0) ? *reinterpret_cast<const u32x2 *>(prev_img + o00 + ch0) : zero2;
        keep.p01 = (act0 && vx1 && vy0) ? *reinterpret_cast<const u32x2 *>(prev_img + o01 + ch0) : zero2;
        keep.p10 = (act0 && vx0 && vy1) ? *reinterpret_cast<const u32x2 *>(prev_img + o10 + ch0) : zero2;
        keep.p11 = (act0 && vx1 && vy1) ? *reinterpret_cast<const u32x2 *>(prev_img + o11 + ch0) : zero2;
        kx = x0;
        ky = y0;
      }
      part = absdiff4(curr0, keep, nw, ne, sw, se, g0);
      if (gate_chunk == 0) gate_v = g0;
      for (int ch = 1; ch < chunks; ++ch) {
        const int cc = ch * kStChunk + ch0;
        const bool act = cc < p.c;
        const u32x2 cu = act ? *reinterpret_cast<const u32x2 *>(curr_px + cc) : zero2;
        Corners k;
        k.p00 = (act && vx0 && vy0) ? *reinterpret_cast<const u32x2 *>(prev_img + o00 + cc) : zero2;
        k.p01 = (act && vx1 && vy0) ? *reinterpret_cast<const u32x2 *>(prev_img + o01 + cc) : zero2;
        k.p10 = (act && vx0 && vy1) ? *reinterpret_cast<const u32x2 *>(prev_img + o10 + cc) : zero2;
        k.p11 = (act && vx1 && vy1) ? *reinterpret_cast<const u32x2 *>(prev_img + o11 + cc) : zero2;
        part = add_rn(part, absdiff4(cu, k, nw, ne, sw, se, g0));
        if (ch == gate_chunk) gate_v = g0;
      }
    }
    float total = wave_sum(part);
    if (gated) {
      const float gv = __shfl(gate_v, gate_lane);
      if (gv == 0.f) total = add_rn(total, p.bias);
    }
    if (lane == (d >> 1)) {
      if (d & 1) c1 = total;
      else c0 = total;
    }
  }

  // softmax over the D costs, two per lane
  const bool has0 = 2 * lane < p.d, has1 = 2 * lane + 1 < p.d;
  const float xa = has0 ? -c0 : -INFINITY, xb = has1 ? -c1 : -INFINITY;
  const float m = wave_max(fmaxf(xa, xb));
  const float ea = has0 ? expf(sub_rn(xa, m)) : 0.f, eb = has1 ? expf(sub_rn(xb, m)) : 0.f;
  const float s = wave_sum(add_rn(ea, eb));
  const float ya = has0 ? lss_div(ea, s) : 0.f, yb = has1 ? lss_div(eb, s) : 0.f;
  if (live) {
    __half *o = p.out + (size_t)pix * p.out_pitch;
    for (int q = lane; 2 * q < p.dpad; q += kWave)
      *reinterpret_cast<unsigned *>(o + 2 * q) = q < kWave ? pack_h2(ya, yb) : 0u;
  }
}

inline bool st_off16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) != 0; }
inline bool st_off4(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 3u) != 0; }

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_stereo_grid(const float *consts, const float *xs, const float *ys, const float *ds, float *grid,
                                  int n, int D, int Hc, int Wc, void *stream) {
  if (!consts || !xs || !ys || !ds || !grid || n < 0 || D <= 0 || Hc <= 0 || Wc <= 0) return BEVOPS_BAD_PARAM;
  if (st_off4(consts) || st_off4(xs) || st_off4(ys) || st_off4(ds) || (reinterpret_cast<uintptr_t>(grid) & 7u))
    return BEVOPS_BAD_PARAM;
  if (D > kStMaxD) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long total = (unsigned long long)n * D * Hc * Wc;
  if ((unsigned long long)Hc * Wc > 0x3fffffffull || Hc > 0x00ffffff || Wc > 0x00ffffff ||
      (total + kStBlock - 1) / kStBlock > 0x7fffffffull)
    return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  hipLaunchKernelGGL(stereo_grid_kernel, dim3((unsigned)((total + kStBlock - 1) / kStBlock)), dim3(kStBlock), 0,
                     static_cast<hipStream_t>(stream), consts, xs, ys, ds, grid, D, Hc, Wc, (long long)total);
  return launch_status();
}

extern "C" int bevops_stereo_cost_volume_f16(const void *prev, int prev_pitch, const void *curr, int curr_pitch,
                                             const float *grid, const float *consts, const float *xs, const float *ys,
                                             const float *ds, void *out, int out_pitch, int n, int Hc, int Wc, int C, int D,
                                             int Dpad, float bias, void *stream) {
  if (!prev || !curr || !out || n < 0 || Hc <= 0 || Wc <= 0 || C <= 0 || D <= 0 || Dpad <= 0) return BEVOPS_BAD_PARAM;
  if (!grid && (!consts || !xs || !ys || !ds)) return BEVOPS_BAD_PARAM;
  if (prev_pitch < C || curr_pitch < C || out_pitch < Dpad || Dpad < D) return BEVOPS_BAD_PARAM;
  if (prev_pitch % 8 != 0 || curr_pitch % 8 != 0 || out_pitch % 8 != 0) return BEVOPS_BAD_PARAM;
  if (st_off16(prev) || st_off16(curr) || st_off16(out)) return BEVOPS_BAD_PARAM;
  if (grid ? (reinterpret_cast<uintptr_t>(grid) & 7u) != 0 : (st_off4(consts) || st_off4(xs) || st_off4(ys) || st_off4(ds)))
    return BEVOPS_BAD_PARAM;
  if (!(bias == bias)) return BEVOPS_BAD_PARAM;
  if (C % 8 != 0 || D > kStMaxD || Dpad % 8 != 0) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long pixels = (unsigned long long)n * Hc * Wc;
  if (pixels > 0x3fffffffull || Hc > 0x00ffffff || Wc > 0x00ffffff) return BEVOPS_NOT_SUPPORTED;
  if (n == 0) return BEVOPS_SUCCESS;
  StereoArgs p;
  p.prev = static_cast<const __half *>(prev);
  p.curr = static_cast<const __half *>(curr);
  p.grid = grid; p.consts = consts; p.xs = xs; p.ys = ys; p.ds = ds;
  p.out = static_cast<__half *>(out);
  p.prev_pitch = prev_pitch; p.curr_pitch = curr_pitch; p.out_pitch = out_pitch;
  p.hc = Hc; p.wc = Wc; p.c = C; p.d = D; p.dpad = Dpad;
  p.pixels = (int)pixels;
  p.bias = bias;
  hipLaunchKernelGGL(stereo_cost_kernel, dim3((unsigned)((pixels + kStWaves - 1) / kStWaves)), dim3(kStBlock), 0,
                     static_cast<hipStream_t>(stream), p);
  return launch_status();
}
