// BEVDet4D's temporal alignment and stacking (gen_grid / shift_feature of BEVDet4D, recalled: the reference tree has no
// BEVDet4D code) as ONE launch: no workspace, no atomics, no LDS.
//
//   out[b, y, x, 0 : C]            = curr[b, y, x, :]                                   bit copy
//   hist[write_slot][b, y, x, :]   = curr[b, y, x, :]                                   bit copy, the frame kept for later
//   out[b, y, x, t C : (t + 1) C]  = valid(b, t) ? bilinear(hist[slot(b, t)][b], sx, sy) : curr[b, y, x, :]     t = 1 .. T
//
// bilinear = zeros padding, align_corners=True, on PIXEL coordinates (torch normalises the position to [-1, 1] and
// un-normalises it again; this kernel does not: a stated deviation of a few ulps of the position).
//
// fp32 operation order, every step ONE rounding, nothing contracted (numpy float32 reproduces it bit for bit):
//   sx = add(add(mul(a00, x), mul(a01, y)), a02)          sy = add(add(mul(a10, x), mul(a11, y)), a12)
//   x0 = floor(sx), x1 = add(x0, 1), fx = sub(sx, x0), gx = sub(1, fx)        (y0, y1, fy, gy likewise)
//   w00 = mul(gx, gy)  corner (y0, x0)      w01 = mul(fx, gy)  corner (y0, x1)
//   w10 = mul(gx, fy)  corner (y1, x0)      w11 = mul(fx, fy)  corner (y1, x1)
//   v   = add(add(add(mul(w00, p00), mul(w01, p01)), mul(w10, p10)), mul(w11, p11))     rounded once to fp16 (RNE)
// A corner is inside when 0 <= its float coordinate <= W - 1 (H - 1), decided ON THE FLOATS: a NaN, infinite or huge
// position is outside and never becomes an address.  A corner outside counts as p = 0 and is not read; a pixel with no
// corner inside is written as zeros without its weights being used.
//
// Mapping.  Block = 4 waves, pixel tile = 8 x 8 pixels of one sample; wave w owns tile rows 2 w and 2 w + 1 (16 pixels,
// two runs of 8).  A lane owns ONE 16-byte channel vector (8 halves) of one pixel: the wave's 16 V work items (V = C / 8,
// item = pixel * V + vector) are taken 64 at a time, ceil(V / 4) passes, so a pass stores consecutive vectors of
// consecutive pixels: contiguous runs.  For each slice t the position, the corner mask and the four weights of the
// wave's 16 pixels are computed ONCE, by lane j for pixel j (the other three quarters of the wave mirror them in the
// same instructions), and a lane takes those of its pixel by six ds_bpermute shuffles per pass; the transform itself is
// wave-uniform (scalar loads from meta).  All T slices of a pixel are produced by the same lane: with at most four
// passes (C <= 128) the curr vectors stay in registers, read once and stored to slice 0, to hist[write_slot] and to
// every invalid slice; wider maps (NP = 0) re-read them (L1) where a slice needs them.  Corner vectors are 16-byte
// loads straight from global memory: the up-to-fourfold reuse between neighbouring pixels is left to L1 / L2 (a
// rotated footprint is no rectangle; no LDS window).
#include "bev_align.h"

namespace bevops {
namespace {

// bev_align.h: the tile constants, the meta layout, Item / item_of, Footprint / footprint (shared with bev_align_s8.hip)
constexpr int kBaBlock = balign::kBlock, kBaTile = balign::kTile, kBaWavePix = balign::kWavePix, kBaMaxT = balign::kMaxT;
constexpr int kBaRegPasses = balign::kRegPasses;      // curr stays in registers up to this many passes (C <= 128)
constexpr int kBaHead = balign::kHead, kBaEntry = balign::kEntry;
using balign::Item;

struct AlignArgs {
  const __half *curr;
  __half *hist, *out;
  const int *meta;
  int curr_pitch, hist_pitch, out_pitch;
  int h, w, c, t, vecs, tiles_x, tiles_y;
  unsigned slot_stride;                          // elements between two slots of the ring
};

__device__ __forceinline__ unsigned blend2(unsigned a, unsigned b, unsigned c, unsigned d, float w00, float w01, float w10,
                                           float w11) {
  const float lo = add_rn(add_rn(add_rn(mul_rn(w00, h2f_lo(a)), mul_rn(w01, h2f_lo(b))), mul_rn(w10, h2f_lo(c))),
                          mul_rn(w11, h2f_lo(d)));
  const float hi = add_rn(add_rn(add_rn(mul_rn(w00, h2f_hi(a)), mul_rn(w01, h2f_hi(b))), mul_rn(w10, h2f_hi(c))),
                          mul_rn(w11, h2f_hi(d)));
  return pack_h2(lo, hi);
}

__device__ __forceinline__ Item item_of(const AlignArgs &p, int k, int lane, int x_base, int y_base, unsigned img) {
  return balign::item_of<8>(p.vecs, p.w, p.h, k, lane, x_base, y_base, img);
}

template <int NP>
__global__ __launch_bounds__(kBaBlock) void bev_align_kernel(AlignArgs p) {
  constexpr int R = NP ? NP : 1;               // passes held in registers = the unroll count of the pass loops
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  unsigned blk = blockIdx.x;
  const int tx = blk % p.tiles_x;
  blk /= p.tiles_x;
  const int ty = blk % p.tiles_y;
  const int b = blk / p.tiles_y;
  const int x_base = tx * kBaTile, y_base = ty * kBaTile + 2 * wave;
  const unsigned img = (unsigned)b * p.h * p.w;
  const int passes = NP ? NP : (kBaWavePix * p.vecs + kWave - 1) / kWave;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  Item it[R];
  u32x4 cur[R];
  const int write_slot = p.meta[0];
  const bool keep = (unsigned)write_slot <= (unsigned)p.t;      // (a slot outside the ring: the frame is not kept)
  __half *kept = p.hist + (size_t)(keep ? write_slot : 0) * p.slot_stride;

  // slice 0 and the ring's free slot, from the registers that also serve the invalid slices
#pragma unroll R
  for (int k = 0; k < passes; ++k) {
    const int r = NP ? k : 0;
    it[r] = item_of(p, k, lane, x_base, y_base, img);
    cur[r] = zero4;
    if (it[r].act) {
      cur[r] = *reinterpret_cast<const u32x4 *>(p.curr + (size_t)it[r].pix * p.curr_pitch + it[r].ch);
      *reinterpret_cast<u32x4 *>(p.out + (size_t)it[r].pix * p.out_pitch + it[r].ch) = cur[r];
      if (keep) *reinterpret_cast<u32x4 *>(kept + (size_t)it[r].pix * p.hist_pitch + it[r].ch) = cur[r];
    }
  }

  // the pixel this lane computes positions for: pixel (lane & 15) of the wave
  const int pj = lane & (kBaWavePix - 1);
  const float px = (float)(x_base + (pj & (kBaTile - 1))), py = (float)(y_base + pj / kBaTile);
  const float wmax = (float)(p.w - 1), hmax = (float)(p.h - 1);

  for (int t = 1; t <= p.t; ++t) {
    const int *m = p.meta + kBaHead + kBaEntry * (b * p.t + t - 1);      // wave-uniform
    const int slot = m[0];
    const bool valid = m[1] != 0;
    const int col = t * p.c;
    if (!valid) {
#pragma unroll R
      for (int k = 0; k < passes; ++k) {
        const int r = NP ? k : 0;
        if (!NP) {
          it[0] = item_of(p, k, lane, x_base, y_base, img);
          if (it[0].act) cur[0] = *reinterpret_cast<const u32x4 *>(p.curr + (size_t)it[0].pix * p.curr_pitch + it[0].ch);
        }
        if (it[r].act) *reinterpret_cast<u32x4 *>(p.out + (size_t)it[r].pix * p.out_pitch + col + it[r].ch) = cur[r];
      }
      continue;
    }
    const bool slot_ok = (unsigned)slot <= (unsigned)p.t;               // (a slot outside the ring: a slice of zeros)
    const __half *src = p.hist + (size_t)(slot_ok ? slot : 0) * p.slot_stride + (size_t)img * p.hist_pitch;
    const balign::Footprint f = balign::footprint(m, px, py, wmax, hmax, slot_ok);
    const float w00 = f.w00, w01 = f.w01, w10 = f.w10, w11 = f.w11;
    const unsigned pos = f.pos, mask = f.mask;

#pragma unroll R
    for (int k = 0; k < passes; ++k) {
      const int r = NP ? k : 0;
      if (!NP) it[0] = item_of(p, k, lane, x_base, y_base, img);
      const Item q = it[r];
      const float u00 = __shfl(w00, q.src), u01 = __shfl(w01, q.src), u10 = __shfl(w10, q.src), u11 = __shfl(w11, q.src);
      const unsigned qpos = (unsigned)__shfl((int)pos, q.src), qmask = (unsigned)__shfl((int)mask, q.src);
      if (!q.act) continue;
      u32x4 v = zero4;
      if (qmask) {
        const int xi = (int)(qpos & 0xffffu) - 1, yi = (int)(qpos >> 16) - 1;
        const long long o00 = ((long long)yi * p.w + xi) * p.hist_pitch + q.ch;      // formed as a number; dereferenced
        const long long o10 = o00 + (long long)p.w * p.hist_pitch;                   // only under its mask bit
        const u32x4 c00 = (qmask & 1u) ? *reinterpret_cast<const u32x4 *>(src + o00) : zero4;
        const u32x4 c01 = (qmask & 2u) ? *reinterpret_cast<const u32x4 *>(src + o00 + p.hist_pitch) : zero4;
        const u32x4 c10 = (qmask & 4u) ? *reinterpret_cast<const u32x4 *>(src + o10) : zero4;
        const u32x4 c11 = (qmask & 8u) ? *reinterpret_cast<const u32x4 *>(src + o10 + p.hist_pitch) : zero4;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = blend2(c00[i], c01[i], c10[i], c11[i], u00, u01, u10, u11);
      }
      *reinterpret_cast<u32x4 *>(p.out + (size_t)q.pix * p.out_pitch + col + q.ch) = v;
    }
  }
}

// bytes from the first to behind the last element of `pixels` rows of `width` elements, `pitch` apart
inline unsigned long long ba_extent(unsigned long long pixels, int pitch, unsigned long long width) {
  return pixels ? ((pixels - 1) * (unsigned long long)pitch + width) * sizeof(__half) : 0ull;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_bev_align_stack_f16(int dtype, const void *curr, int curr_pitch, void *hist, int hist_pitch, void *out,
                                          int out_pitch, const void *meta, int B, int H, int W, int C, int T, void *stream) {
  if (!curr || !hist || !out || !meta || B < 0 || H <= 0 || W <= 0 || C <= 0 || T < 1) return BEVOPS_BAD_PARAM;
  const long long width = (long long)(T + 1) * C;
  if (curr_pitch < C || hist_pitch < C || out_pitch < width) return BEVOPS_BAD_PARAM;
  if (curr_pitch % 8 != 0 || hist_pitch % 8 != 0 || out_pitch % 8 != 0) return BEVOPS_BAD_PARAM;
  if (!aligned16(curr) || !aligned16(hist) || !aligned16(out) || !aligned16(meta)) return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F16 || C % 8 != 0 || T > kBaMaxT || H > 0xffff || W > 0xffff) return BEVOPS_NOT_SUPPORTED;
  const unsigned long long pixels = (unsigned long long)B * H * W, limit = 0x7fffffffull;
  if (ba_extent(pixels, curr_pitch, C) >= limit || ba_extent(pixels * (T + 1), hist_pitch, C) >= limit ||
      ba_extent(pixels, out_pitch, width) >= limit)
    return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  AlignArgs p;
  p.curr = static_cast<const __half *>(curr);
  p.hist = static_cast<__half *>(hist);
  p.out = static_cast<__half *>(out);
  p.meta = static_cast<const int *>(meta);
  p.curr_pitch = curr_pitch; p.hist_pitch = hist_pitch; p.out_pitch = out_pitch;
  p.h = H; p.w = W; p.c = C; p.t = T; p.vecs = C / 8;
  p.tiles_x = (W + kBaTile - 1) / kBaTile;
  p.tiles_y = (H + kBaTile - 1) / kBaTile;
  p.slot_stride = (unsigned)(pixels * hist_pitch);
  const dim3 grid((unsigned)((unsigned long long)B * p.tiles_x * p.tiles_y)), block(kBaBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch ((kBaWavePix * p.vecs + kWave - 1) / kWave) {
    case 1: hipLaunchKernelGGL(bev_align_kernel<1>, grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL(bev_align_kernel<2>, grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL(bev_align_kernel<3>, grid, block, 0, s, p); break;
    case kBaRegPasses: hipLaunchKernelGGL(bev_align_kernel<kBaRegPasses>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(bev_align_kernel<0>, grid, block, 0, s, p); break;
  }
  return launch_status();
}
