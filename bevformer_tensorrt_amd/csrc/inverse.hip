// Batched inverse of small fp32 matrices: the InverseTRT plugin (inverseKernel.cu:9-41: LU with partial pivoting through
// cublasSgetrfBatched + cublasSgetriBatched; det2trt/models/functions/inverse.py: torch.linalg.inv), 1 <= n <= 32.
//
// One wave per matrix, Gauss-Jordan with partial pivoting on [A | I] without row exchanges: lane i holds row i (its n
// entries of A and n of the identity block in registers).  Step k picks, among the rows not yet used as a pivot, the one
// with the largest |a[., k]| (ties: the lowest row, as isamax) -- a wave-wide arg-max -- broadcasts that row with
// v_readlane (the pivot index is wave-uniform), scales it by 1 / pivot and subtracts a[i, k] times it from every other
// row.  After n steps the pivot row of column k holds row k of A^-1 in its identity block; the lane stores it there.
// The unused rows see exactly the updates of LU with partial pivoting, so the pivot sequence is LU's.
// An exactly zero pivot (a singular matrix) makes the whole matrix NaN; other matrices of the batch are unaffected.
// NB = 4 / 8 / 16 / 32 instances size the register rows to the matrix.
#include "common.h"

namespace bevops {
namespace {

constexpr int kInvWaves = 4;   // matrices per block

template <int NB>
__global__ __launch_bounds__(64 * kInvWaves) void inverse_f32_kernel(const float *__restrict__ in,
                                                                     float *__restrict__ out, int batch, int n) {
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * kInvWaves + (threadIdx.x >> 6);
  if (m >= batch) return;                              // wave-uniform
  const size_t base = (size_t)m * n * n;
  const bool live = lane < n;
  float a[NB], x[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    a[j] = (live && j < n) ? in[base + (size_t)lane * n + j] : 0.f;
    x[j] = (live && j == lane) ? 1.f : 0.f;
  }
  unsigned used = 0;        // rows already chosen as pivots (wave-uniform bit mask)
  int my_row = 0;           // the output row this lane's row becomes
  bool singular = false;    // wave-uniform
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    if (k >= n) continue;   // (wave-uniform; `break` would keep the loop from unrolling)
    // arg-max |a[i, k]| over the rows not used yet, ties to the lower row (NaN counts as the largest, so that it
    // spreads instead of breaking the order); every lane ends with the same (value, row)
    float v = -1.f;
    if (live && !((used >> lane) & 1u)) {
      v = fabsf(a[k]);
      if (v != v) v = INFINITY;
    }
    int idx = lane;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float v2 = __shfl_xor(v, off, 64);
      const int i2 = __shfl_xor(idx, off, 64);
      if (v2 > v || (v2 == v && i2 < idx)) v = v2, idx = i2;
    }
    const int p = __builtin_amdgcn_readfirstlane(idx);
    if (__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))) == 0.f) singular = true;
    used |= 1u << p;
    if (lane == p) my_row = k;
    float pa[NB], px[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      pa[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[j]), p));
      px[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[j]), p));
    }
    const float r = 1.f / pa[k];
#pragma unroll
    for (int j = 0; j < NB; ++j) pa[j] *= r, px[j] *= r;
    const float f = a[k];
    if (lane == p) {
#pragma unroll
      for (int j = 0; j < NB; ++j) a[j] = pa[j], x[j] = px[j];
    } else {
#pragma unroll
      for (int j = 0; j < NB; ++j) a[j] = fmaf(-f, pa[j], a[j]), x[j] = fmaf(-f, px[j], x[j]);
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < NB; ++j)
    if (j < n) out[base + (size_t)my_row * n + j] = singular ? __builtin_nanf("") : x[j];
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_inverse_forward(int dtype, const void *input, void *output, int batch, int n, void *stream) {
  if (!input || !output || batch <= 0 || n <= 0) return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F32 || n > 32) return BEVOPS_NOT_SUPPORTED;
  if (!aligned16(input) || !aligned16(output)) return BEVOPS_BAD_PARAM;
  const dim3 grid((unsigned)((batch + kInvWaves - 1) / kInvWaves)), block(64 * kInvWaves);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const float *in = static_cast<const float *>(input);
  float *out = static_cast<float *>(output);
  if (n <= 4)
    hipLaunchKernelGGL(inverse_f32_kernel<4>, grid, block, 0, st, in, out, batch, n);
  else if (n <= 8)
    hipLaunchKernelGGL(inverse_f32_kernel<8>, grid, block, 0, st, in, out, batch, n);
  else if (n <= 16)
    hipLaunchKernelGGL(inverse_f32_kernel<16>, grid, block, 0, st, in, out, batch, n);
  else
    hipLaunchKernelGGL(inverse_f32_kernel<32>, grid, block, 0, st, in, out, batch, n);
  return launch_status();
}
