// BEVDet4D's temporal alignment and stacking on INT8 maps: bev_align.hip's statement on one byte per element, ONE launch,
// no workspace, no atomics, no LDS (design/bevdet4d_int8.md).
//
//   out[b, y, x, 0 : C]            = curr[b, y, x, :]                                   byte copy
//   hist[write_slot][b, y, x, :]   = curr[b, y, x, :]                                   byte copy, the frame kept for later
//   out[b, y, x, t C : (t + 1) C]  = valid(b, t) ? q8(bilinear(hist[slot(b, t)][b], sx, sy)) : curr[b, y, x, :]   t = 1 .. T
//
// No scale argument: PTQ scales are static, so every slot of the ring carries the scale of today's map, and a bilinear
// blend with zeros padding is a convex (at the border sub-convex) combination: the blended bytes stay in that scale.
//
// Positions, corner validity and weights are bev_align.hip's, operation for operation (fp32, every step ONE rounding,
// nothing contracted; meta has the same layout).  The blend on the int8 corner values p, converted exactly to fp32:
//   v = add(add(add(mul(w00, p00), mul(w01, p01)), mul(w10, p10)), mul(w11, p11))      byte = min(max(rne(v), -127), 127)
// A corner outside counts as p = 0 and is not read; a pixel with no corner inside is written as zero bytes.
//
// Mapping.  Block = 4 waves, pixel tile = 8 x 8 pixels of one sample; wave w owns tile rows 2 w and 2 w + 1 (16 pixels).
// A lane owns ONE 16-byte vector = 16 CHANNELS of one pixel: the wave's 16 V work items (V = C / 16, item = pixel * V +
// vector) are taken 64 at a time, ceil(V / 4) passes, so a pass stores consecutive vectors of consecutive pixels.  For
// each slice the position, the corner mask and the four weights of the wave's 16 pixels are computed once, by lane j for
// pixel j, and fetched by six shuffles per pass.  With at most four passes (C <= 256) the curr vectors stay in registers
// (16 VGPRs), read once and stored to slice 0, to hist[write_slot] and to every invalid slice; wider maps (NP = 0)
// re-read them.  A corner vector is one 16-byte load; its bytes are unpacked by sign-extending bit-field extraction
// and int -> float conversion (no fp16 on the way), the 16 results are repacked into four dwords: one 16-byte store.
// All element offsets are 32-bit: the entry refuses operands that reach 2^31 - 1 bytes.
#include "bev_align.h"

namespace bevops {
namespace {

using namespace balign;      // tile constants, meta layout, Item / item_of, Footprint / footprint

constexpr int kBqVec = 16;                       // channels (bytes) of a lane's vector: curr in registers for C <= 256

struct AlignArgsQ {
  const signed char *curr;
  signed char *hist, *out;
  const int *meta;
  unsigned curr_pitch, hist_pitch, out_pitch;
  int h, w, c, t, vecs, tiles_x, tiles_y;
  unsigned slot_stride;                          // bytes between two slots of the ring
};

__device__ __forceinline__ float s8f(unsigned word, int i) {      // byte i of word, sign-extended (v_bfe_i32), as a float
  return (float)((int)(word << (24 - 8 * i)) >> 24);
}

__device__ __forceinline__ unsigned q8(float v) {                 // min(max(rne(v), -127), 127) as a byte
  return (unsigned)(int)fminf(fmaxf(rintf(v), -127.f), 127.f) & 0xffu;
}

__device__ __forceinline__ unsigned blend4(unsigned a, unsigned b, unsigned c, unsigned d, float w00, float w01, float w10,
                                           float w11) {
  unsigned r = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v = add_rn(add_rn(add_rn(mul_rn(w00, s8f(a, i)), mul_rn(w01, s8f(b, i))), mul_rn(w10, s8f(c, i))),
                           mul_rn(w11, s8f(d, i)));
    r |= q8(v) << (8 * i);
  }
  return r;
}

__device__ __forceinline__ Item item_of(const AlignArgsQ &p, int k, int lane, int x_base, int y_base, unsigned img) {
  return balign::item_of<kBqVec>(p.vecs, p.w, p.h, k, lane, x_base, y_base, img);
}

__device__ __forceinline__ u32x4 ld16(const signed char *base, unsigned off) {
  return *reinterpret_cast<const u32x4 *>(base + off);
}
__device__ __forceinline__ void st16(signed char *base, unsigned off, u32x4 v) { *reinterpret_cast<u32x4 *>(base + off) = v; }

template <int NP>
__global__ __launch_bounds__(kBlock) void bev_align_s8_kernel(AlignArgsQ p) {
  constexpr int R = NP ? NP : 1;               // passes held in registers = the unroll count of the pass loops
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  unsigned blk = blockIdx.x;
  const int tx = blk % p.tiles_x;
  blk /= p.tiles_x;
  const int ty = blk % p.tiles_y;
  const int b = blk / p.tiles_y;
  const int x_base = tx * kTile, y_base = ty * kTile + 2 * wave;
  const unsigned img = (unsigned)b * p.h * p.w;
  const int passes = NP ? NP : (kWavePix * p.vecs + kWave - 1) / kWave;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  Item it[R];
  u32x4 cur[R];
  const int write_slot = p.meta[0];
  const bool keep = (unsigned)write_slot <= (unsigned)p.t;      // (a slot outside the ring: the frame is not kept)
  signed char *kept = p.hist + (keep ? (unsigned)write_slot : 0u) * p.slot_stride;

  // slice 0 and the ring's free slot, from the registers that also serve the invalid slices
#pragma unroll R
  for (int k = 0; k < passes; ++k) {
    const int r = NP ? k : 0;
    it[r] = item_of(p, k, lane, x_base, y_base, img);
    cur[r] = zero4;
    if (it[r].act) {
      cur[r] = ld16(p.curr, it[r].pix * p.curr_pitch + it[r].ch);
      st16(p.out, it[r].pix * p.out_pitch + it[r].ch, cur[r]);
      if (keep) st16(kept, it[r].pix * p.hist_pitch + it[r].ch, cur[r]);
    }
  }

  // the pixel this lane computes positions for: pixel (lane & 15) of the wave
  const int pj = lane & (kWavePix - 1);
  const float px = (float)(x_base + (pj & (kTile - 1))), py = (float)(y_base + pj / kTile);
  const float wmax = (float)(p.w - 1), hmax = (float)(p.h - 1);

  for (int t = 1; t <= p.t; ++t) {
    const int *m = p.meta + kHead + kEntry * (b * p.t + t - 1);      // wave-uniform
    const int slot = m[0];
    const bool valid = m[1] != 0;
    const unsigned col = (unsigned)(t * p.c);
    if (!valid) {
#pragma unroll R
      for (int k = 0; k < passes; ++k) {
        const int r = NP ? k : 0;
        if (!NP) {
          it[0] = item_of(p, k, lane, x_base, y_base, img);
          if (it[0].act) cur[0] = ld16(p.curr, it[0].pix * p.curr_pitch + it[0].ch);
        }
        if (it[r].act) st16(p.out, it[r].pix * p.out_pitch + col + it[r].ch, cur[r]);
      }
      continue;
    }
    const bool slot_ok = (unsigned)slot <= (unsigned)p.t;               // (a slot outside the ring: a slice of zeros)
    const signed char *src = p.hist + ((slot_ok ? (unsigned)slot : 0u) * p.slot_stride + img * p.hist_pitch);
    const Footprint f = footprint(m, px, py, wmax, hmax, slot_ok);

#pragma unroll R
    for (int k = 0; k < passes; ++k) {
      const int r = NP ? k : 0;
      if (!NP) it[0] = item_of(p, k, lane, x_base, y_base, img);
      const Item q = it[r];
      const float u00 = __shfl(f.w00, q.src), u01 = __shfl(f.w01, q.src);
      const float u10 = __shfl(f.w10, q.src), u11 = __shfl(f.w11, q.src);
      const unsigned qpos = (unsigned)__shfl((int)f.pos, q.src), qmask = (unsigned)__shfl((int)f.mask, q.src);
      if (!q.act) continue;
      u32x4 v = zero4;
      if (qmask) {
        // offsets modulo 2^32: a corner with x0 = -1 or y0 = -1 wraps below zero and its inside neighbour wraps back to the
        // true offset, which the entry keeps below 2^31; a corner is dereferenced only under its mask bit
        const int xi = (int)(qpos & 0xffffu) - 1, yi = (int)(qpos >> 16) - 1;
        const unsigned o00 = ((unsigned)yi * (unsigned)p.w + (unsigned)xi) * p.hist_pitch + (unsigned)q.ch;
        const unsigned o10 = o00 + (unsigned)p.w * p.hist_pitch;
        const u32x4 c00 = (qmask & 1u) ? ld16(src, o00) : zero4;
        const u32x4 c01 = (qmask & 2u) ? ld16(src, o00 + p.hist_pitch) : zero4;
        const u32x4 c10 = (qmask & 4u) ? ld16(src, o10) : zero4;
        const u32x4 c11 = (qmask & 8u) ? ld16(src, o10 + p.hist_pitch) : zero4;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = blend4(c00[i], c01[i], c10[i], c11[i], u00, u01, u10, u11);
      }
      st16(p.out, q.pix * p.out_pitch + col + q.ch, v);
    }
  }
}

// bytes from the first to behind the last element of `pixels` rows of `width` bytes, `pitch` apart
inline unsigned long long bq_extent(unsigned long long pixels, int pitch, unsigned long long width) {
  return pixels ? (pixels - 1) * (unsigned long long)pitch + width : 0ull;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_bev_align_stack_s8(const void *curr, int curr_pitch, void *hist, int hist_pitch, void *out, int out_pitch,
                                         const void *meta, int B, int H, int W, int C, int T, void *stream) {
  if (!curr || !hist || !out || !meta || B < 0 || H <= 0 || W <= 0 || C <= 0 || T < 1) return BEVOPS_BAD_PARAM;
  const long long width = (long long)(T + 1) * C;
  if (curr_pitch < C || hist_pitch < C || out_pitch < width) return BEVOPS_BAD_PARAM;
  if (curr_pitch % kBqVec != 0 || hist_pitch % kBqVec != 0 || out_pitch % kBqVec != 0) return BEVOPS_BAD_PARAM;
  if (!aligned16(curr) || !aligned16(hist) || !aligned16(out) || !aligned16(meta)) return BEVOPS_BAD_PARAM;
  if (C % kBqVec != 0 || T > kMaxT || H > 0xffff || W > 0xffff) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long pixels = (unsigned long long)B * H * W, limit = 0x7fffffffull;
  if (bq_extent(pixels, curr_pitch, C) >= limit || bq_extent(pixels * (T + 1), hist_pitch, C) >= limit ||
      bq_extent(pixels, out_pitch, width) >= limit)
    return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  AlignArgsQ p;
  p.curr = static_cast<const signed char *>(curr);
  p.hist = static_cast<signed char *>(hist);
  p.out = static_cast<signed char *>(out);
  p.meta = static_cast<const int *>(meta);
  p.curr_pitch = curr_pitch; p.hist_pitch = hist_pitch; p.out_pitch = out_pitch;
  p.h = H; p.w = W; p.c = C; p.t = T; p.vecs = C / kBqVec;
  p.tiles_x = (W + kTile - 1) / kTile;
  p.tiles_y = (H + kTile - 1) / kTile;
  p.slot_stride = (unsigned)(pixels * hist_pitch);
  const dim3 grid((unsigned)((unsigned long long)B * p.tiles_x * p.tiles_y)), block(kBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch ((kWavePix * p.vecs + kWave - 1) / kWave) {
    case 1: hipLaunchKernelGGL(bev_align_s8_kernel<1>, grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL(bev_align_s8_kernel<2>, grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL(bev_align_s8_kernel<3>, grid, block, 0, s, p); break;
    case kRegPasses: hipLaunchKernelGGL(bev_align_s8_kernel<kRegPasses>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(bev_align_s8_kernel<0>, grid, block, 0, s, p); break;
  }
  return launch_status();
}
