// What bev_align.hip (fp16) and bev_align_s8.hip (int8) share: the tile constants, the meta layout, a wave's work items and
// the per-pixel sampling footprint.  The footprint is the one place where a position becomes corner validity and
// weights; its fp32 operation order is stated in bev_align.hip's header and held bit for bit by both files' tests.
#pragma once
#include <math.h>

#include "common.h"

namespace bevops {
namespace balign {

constexpr int kBlock = 256;
constexpr int kTile = 8;                         // the pixel tile is kTile x kTile
constexpr int kWavePix = 16;                     // pixels per wave: two tile rows
constexpr int kMaxT = 15;
constexpr int kRegPasses = 4;                    // curr stays in registers up to this many passes
constexpr int kHead = 4, kEntry = 8;             // meta: words of the header and of one (sample, slice) entry

// The work item of `lane` in pass k of its wave: pixel (x, y) of the tile rows the wave owns and channel offset ch.
struct Item {
  unsigned pix;        // b * H * W + y * W + x
  int src, ch;         // the lane that holds the pixel's position and weights; first channel of the vector
  bool act;            // inside the wave's items and inside the map
};

// VEC: channels of a lane's 16-byte vector (8 halves, 16 bytes); vecs = C / VEC
template <int VEC>
__device__ __forceinline__ Item item_of(int vecs, int w, int h, int k, int lane, int x_base, int y_base, unsigned img) {
  const int it = k * kWave + lane;
  const int j = it / vecs;
  const int x = x_base + (j & (kTile - 1)), y = y_base + ((j / kTile) & 1);
  Item r;
  r.src = j & (kWavePix - 1);
  r.ch = (it - j * vecs) * VEC;
  r.act = j < kWavePix && x < w && y < h;
  r.pix = img + (unsigned)y * w + x;
  return r;
}

// The footprint of pixel (px, py) under the entry m (a00 .. a12 in words 2 .. 7): the four weights, (x0 + 1) | (y0 + 1) << 16
// with 0 for a coordinate outside, and the corner mask (bit 0: (y0, x0), 1: (y0, x1), 2: (y1, x0), 3: (y1, x1)).
// Validity is decided on the floats; only a valid coordinate is converted.  slot_ok false: no corner is inside.
struct Footprint {
  float w00, w01, w10, w11;
  unsigned pos, mask;
};

__device__ __forceinline__ Footprint footprint(const int *m, float px, float py, float wmax, float hmax, bool slot_ok) {
  const float a00 = __int_as_float(m[2]), a01 = __int_as_float(m[3]), a02 = __int_as_float(m[4]);
  const float a10 = __int_as_float(m[5]), a11 = __int_as_float(m[6]), a12 = __int_as_float(m[7]);
  const float sx = add_rn(add_rn(mul_rn(a00, px), mul_rn(a01, py)), a02);
  const float sy = add_rn(add_rn(mul_rn(a10, px), mul_rn(a11, py)), a12);
  const float x0 = floorf(sx), y0 = floorf(sy);
  const float x1 = add_rn(x0, 1.f), y1 = add_rn(y0, 1.f);
  const float fx = sub_rn(sx, x0), fy = sub_rn(sy, y0);
  const float gx = sub_rn(1.f, fx), gy = sub_rn(1.f, fy);
  Footprint f;
  f.w00 = mul_rn(gx, gy); f.w01 = mul_rn(fx, gy); f.w10 = mul_rn(gx, fy); f.w11 = mul_rn(fx, fy);
  const bool vx0 = x0 >= 0.f && x0 <= wmax, vx1 = x1 >= 0.f && x1 <= wmax;
  const bool vy0 = y0 >= 0.f && y0 <= hmax, vy1 = y1 >= 0.f && y1 <= hmax;
  f.pos = (unsigned)(vx0 ? (int)x0 + 1 : 0) | (unsigned)(vy0 ? (int)y0 + 1 : 0) << 16;
  f.mask = slot_ok ? ((unsigned)(vx0 && vy0) | (unsigned)(vx1 && vy0) << 1 | (unsigned)(vx0 && vy1) << 2 |
                      (unsigned)(vx1 && vy1) << 3)
                   : 0u;
  return f;
}

}  // namespace balign
}  // namespace bevops
