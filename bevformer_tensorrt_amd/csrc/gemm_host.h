// Host layer of the dense GEMM families (tsgemm.hip, tile_gemm.hip, small_gemm.hip): the call descriptor an extern "C"
// entry builds once, and the checks and tables the families share.  An entry reads as: build the call, run the family's
// domain checks in their order, launch.  The per-family domains and statuses are tabulated in design/dense.md.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace bevops {

// out[m, n] = act(sum_k x[m, k] w[n, k] + bias[n] (+ res[m, n])), as the entry received it
struct GemmCall {
  const void *x, *w, *bias, *res;
  void *out;
  long long m;
  int n, k, relu;
  hipStream_t st;
};

// the int8 flavours: quantisation scales and the BEVOPS_F16 / BEVOPS_I8 codes of the identity and output rows
struct GemmCallS8 : GemmCall {
  const float *w_scales;   // per output channel, or null (then scale_w)
  float scale_a, scale_w, scale_res, scale_out;
  int res_dtype, out_dtype;
};

inline GemmCallS8 gemm_call_f16(const void *x, const void *w, const void *bias, const void *res, void *out, long long m,
                                int n, int k, int relu, void *stream) {
  return GemmCallS8{{x, w, bias, res, out, m, n, k, relu, static_cast<hipStream_t>(stream)},
                    nullptr, 1.f, 1.f, 1.f, 1.f, BEVOPS_F16, BEVOPS_F16};
}

// Operands are addressed through 32-bit buffer offsets.  Offsets from kGemmOob on lie beyond any buffer (the kernels use
// it as the address that reads as zero), so a buffer must end below it.
constexpr unsigned kGemmOob = 0xFFFFFF00u;
inline bool gemm_over_limit(unsigned long long rows, int cols, int elem_bytes) {
  return rows >= kGemmOob || rows * (unsigned long long)cols * (unsigned long long)elem_bytes >= kGemmOob;
}

inline bool misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// a quantisation scale the int8 entries refuse: non-positive, NaN or inf
inline bool bad_scale(float s) { return !(s > 0.f) || !(s <= 3.4028234663852886e38f); }

// Destination table of the _dst launches: column range [col_begin, col_end) of the launch is a pitched matrix of its own
// with an identity of its own.  Passed to the kernels by value.
constexpr int kGemmMaxDst = 8;
struct GemmDst { int col_begin, col_end; __half *out; const __half *res; int out_pitch, res_pitch; };
struct GemmDstTab { int count; GemmDst e[kGemmMaxDst]; };

// Validates dst[0 .. num_dst) (1 <= num_dst <= kGemmMaxDst: the entry's check) and fills tab.  A range begins on the
// 64-column block grid and ends on a multiple of `end_gran` (64, or 8: then nothing else may begin in that block); two
// ranges neither overlap nor share a 64-column block.  `res_range`: an identity's rows are read through a buffer
// descriptor, so its byte range is limited as the operands' are.
inline int gemm_dst_table(GemmDstTab &tab, const bevops_gemm_dst *dst, int num_dst, long long m, int n, int end_gran,
                          bool res_range) {
  tab = GemmDstTab{};
  tab.count = num_dst;
  for (int i = 0; i < num_dst; ++i) {
    const bevops_gemm_dst &e = dst[i];
    const long long width = (long long)e.col_end - e.col_begin;
    if (e.col_begin < 0 || e.col_end > n || width <= 0 || e.col_begin % 64 != 0 || e.col_end % end_gran != 0) return BEVOPS_BAD_PARAM;
    if (!e.out || !aligned16(e.out) || e.out_pitch < width || e.out_pitch % 8 != 0 || e.out_pitch > 0x7fffffffLL) return BEVOPS_BAD_PARAM;
    if (e.res && (!aligned16(e.res) || e.res_pitch < width || e.res_pitch % 8 != 0 || e.res_pitch > 0x7fffffffLL)) return BEVOPS_BAD_PARAM;
    if (res_range && e.res && gemm_over_limit((unsigned long long)m, (int)e.res_pitch, 2)) return BEVOPS_NOT_SUPPORTED;
    for (int j = 0; j < i; ++j)
      if (e.col_begin < (dst[j].col_end + 63) / 64 * 64 && dst[j].col_begin < (e.col_end + 63) / 64 * 64) return BEVOPS_BAD_PARAM;
    tab.e[i] = GemmDst{e.col_begin, e.col_end, static_cast<__half *>(e.out), static_cast<const __half *>(e.res),
                       (int)e.out_pitch, e.res ? (int)e.res_pitch : 0};
  }
  return BEVOPS_SUCCESS;
}

// bevops_gemm2_f16: one accumulation over two activation sources, as the entry received it.  a2 is a channels-last
// [B, H, W, k2] tensor whose row m is pixel (b, stride ho, stride wo), m = (b ho_n + ho) wo_n + wo.
struct Gemm2Call {
  const void *a1, *a2, *w, *bias;
  void *out;
  long long m;
  int n, k1, k2, B, H, W, stride;
  int ho, wo;   // filled by gemm2_check
  int relu;
  hipStream_t st;
};

// The entry's checks in their order (no device call): null / sign, domain, geometry, alignment, 32-bit byte ranges.
inline int gemm2_check(Gemm2Call &g) {
  if (!g.a1 || !g.a2 || !g.w || !g.out || g.m <= 0 || g.n <= 0 || g.k1 <= 0 || g.k2 <= 0 || g.B <= 0 || g.H <= 0 || g.W <= 0 ||
      g.stride <= 0)
    return BEVOPS_BAD_PARAM;
  if (g.k1 % 64 != 0 || g.k2 % 64 != 0 || g.n % 8 != 0 || g.stride > 2) return BEVOPS_NOT_SUPPORTED;
  g.ho = (g.H - 1) / g.stride + 1;
  g.wo = (g.W - 1) / g.stride + 1;
  if (g.m != (long long)g.B * g.ho * g.wo) return BEVOPS_BAD_PARAM;
  if (misaligned(g.a1, 15u) || misaligned(g.a2, 15u) || misaligned(g.w, 15u) || misaligned(g.out, 15u) ||
      (g.bias && misaligned(g.bias, 15u)))
    return BEVOPS_BAD_PARAM;
  if (g.m > 0x7fffffffLL || gemm_over_limit((unsigned long long)g.m, g.k1, 2) ||
      gemm_over_limit((unsigned long long)g.B * g.H * g.W, g.k2, 2) || gemm_over_limit((unsigned long long)g.n, g.k1 + g.k2, 2) ||
      (long long)g.k1 + g.k2 > 0x7fffffffLL / 4)
    return BEVOPS_NOT_SUPPORTED;
  return BEVOPS_SUCCESS;
}

// tsgemm.hip: the weight-stationary kernel with a second row source -- its domain, and the launch of a checked call
bool tsgemm_ws2_in_domain(const Gemm2Call &g);
int tsgemm_ws2_launch(const Gemm2Call &g);

// Kernels instantiated per k / 64: returns f(std::integral_constant<int, S>) for S == steps in 1 .. MAX, and
// BEVOPS_NOT_SUPPORTED for any other step count.
template <class F, int... I>
inline int gemm_k64_impl(int steps, F &f, std::integer_sequence<int, I...>) {
  int rc = BEVOPS_NOT_SUPPORTED;
  (void)((steps == I + 1 ? (rc = f(std::integral_constant<int, I + 1>{}), true) : false) || ...);
  return rc;
}
template <int MAX, class F>
inline int gemm_k64(int steps, F f) {
  return gemm_k64_impl(steps, f, std::make_integer_sequence<int, MAX>{});
}

}  // namespace bevops
