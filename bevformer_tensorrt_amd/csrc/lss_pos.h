// Source position of align_corners=True resampling, shared by the fp16 and the int8 bilinear up-samplers
// (lss_split.hip, lss_split_s8.hip), and the reference's fp32 order of a frustum point's 3 x 3 chain, shared by the
// view transformer's index build (lss_prepare.hip) and the BEVStereo warp grid (stereo_cost.hip).
#pragma once
#include "common.h"

namespace bevops {

// Source position of output index o on an axis of `dst` outputs over `src` inputs, align_corners=True:
// o * (src - 1) / (dst - 1) as an exact fraction -- integer part i0, remainder / (dst - 1) as the weight of i0 + 1 -- so
// the first and last outputs sit exactly on the first and last inputs and an equal-size axis is the identity.
__device__ __forceinline__ void source_pos(unsigned o, unsigned src, unsigned dst, unsigned &i0, unsigned &i1, float &l) {
  if (dst <= 1u) {
    i0 = i1 = 0u;
    l = 0.f;
    return;
  }
  const unsigned num = o * (src - 1u), den = dst - 1u;
  i0 = num / den;
  const unsigned rem = num - i0 * den;
  i1 = min(i0 + 1u, src - 1u);
  l = (float)rem / (float)den;
}

__device__ __forceinline__ float lss_div(float a, float b) {   // IEEE division, never a reciprocal multiply
#pragma clang fp reciprocal(off) contract(off)
  return __fdiv_rn(a, b);
}

__device__ __forceinline__ void lss_mat3(const float *__restrict__ m, float &x, float &y, float &z) {
  const float ox = add_rn(add_rn(mul_rn(m[0], x), mul_rn(m[1], y)), mul_rn(m[2], z));
  const float oy = add_rn(add_rn(mul_rn(m[3], x), mul_rn(m[4], y)), mul_rn(m[5], z));
  const float oz = add_rn(add_rn(mul_rn(m[6], x), mul_rn(m[7], y)), mul_rn(m[8], z));
  x = ox; y = oy; z = oz;
}

}  // namespace bevops
