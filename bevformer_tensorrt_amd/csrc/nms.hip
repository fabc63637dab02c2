// BEV non-maximum suppression on the device: the rotated scale-NMS of CenterHead.get_task_detections and the circle
// NMS of CenterHead.get_bboxes, with the size restore and the z shift that follow them.  Reference:
//   third_party/bev_mmdet3d/models/dense_heads/centerpoint_head.py:747-806 (get_bboxes), :808-905 (get_task_detections),
//   third_party/bev_mmdet3d/core/post_processing/box3d_nms.py:182-221 (circle_nms), :227-273 (nms_bev).
// Fixed-capacity outputs like the decoders' (csrc/decode.hip): kept rows in rank order at the front, zero behind
// count[b]; nothing is read back by the host, no launch is sized by a device value, so the call can be captured.
//
// Three launches:
//   1. rank: one block per item sorts the valid rows by the 64-bit key of topk.h (score descending, lower row first),
//      cuts to pre_max_size and writes, per ranked row, the scaled box in the form the pair test reads.
//   2. mask: one WAVE per (ranked row i, 64-column word): lane = column j, the row's box is wave-uniform, the word is
//      the ballot of the pair test.  Only words on or above the diagonal are evaluated; the others are written zero.
//   3. scan: wave 0 of one block per item holds the running suppressed set, lane w owning word w; rows of the mask are
//      staged into LDS a chunk ahead by the whole block; then the whole block gathers the kept rows.
// No atomics apart from the histogram of the selection (topk.h, whose order cannot show).
//
// Pair test, rotate: IoU of the two rotated rectangles, evaluated in the frame of box i (centre at the origin, axes
// along the box): box j's four corners are clipped against the four axis-aligned edges of box i (Sutherland-Hodgman;
// the polygon lives in LDS, one column per thread, because its length is data-dependent).  Relative coordinates keep
// the fp32 error near 1e-6 where absolute coordinates at +-50 m lose three decades (design/postprocess.md).
#include "topk.h"

namespace bevops {
namespace {

constexpr int kNmsMaxRows = 4096;      // num of bevops_bev_nms: 64 words of 64 columns, one per lane of the scan wave
constexpr int kNmsMaxFactors = 64;     // rescale factors travel as a kernel argument
constexpr int kPairThreads = 256;      // block of the mask / IoU kernels
constexpr int kPolyMax = 8;            // a quadrilateral clipped by four half-planes has at most eight vertices
constexpr int kRowFloats = 12;         // x, y, w/2, l/2, cos, sin, ux, uy, vx, vy, area, circumradius
constexpr int kScanThreads = 1024;
constexpr int kScanChunkBytes = 48 * 1024;   // mask rows staged in LDS per round of the scan

struct Factors {
  float v[kNmsMaxFactors];
  int n;
};

struct ScoreSrc {
  const float *p;
  __device__ __forceinline__ u64 operator()(unsigned i) const { return ((u64)rank_bits(p[i]) << 32) | i; }
};

__device__ __forceinline__ float factor_of(const Factors &f, int label) {
  if (f.n == 1) return f.v[0];
  return (label >= 0 && label < f.n) ? f.v[label] : 1.0f;
}

struct PairBox {   // what the pair test reads of one box
  float x, y, hw, hl, c, s, ux, uy, vx, vy, area, rad;
};

// w along (cos, sin), l across it -- mmcv's (x, y, w, h, angle).  A box with a non-finite entry gets a NaN radius:
// every test it takes part in is then false.
__device__ __forceinline__ PairBox make_pair_box(float x, float y, float w, float l, float yaw) {
  PairBox b;
  b.x = x, b.y = y, b.hw = 0.5f * w, b.hl = 0.5f * l;
  b.c = cosf(yaw), b.s = sinf(yaw);
  b.ux = b.hw * b.c, b.uy = b.hw * b.s;
  b.vx = -b.hl * b.s, b.vy = b.hl * b.c;
  b.area = w * l;
  b.rad = sqrtf(b.hw * b.hw + b.hl * b.hl);
  const float all = x + y + w + l + b.c + b.s;
  if (!(fabsf(all) <= 3.0e38f)) b.rad = __uint_as_float(0x7fc00000u);
  return b;
}

// One Sutherland-Hodgman stage against the half-plane sign * p[AXIS] <= bound.  in / out: this thread's columns of
// the LDS polygon buffers (vertex k at [k * kPairThreads]).  Returns the new vertex count (<= kPolyMax).
template <int AXIS>
__device__ __forceinline__ int clip_stage(const float2 *in, int n, float2 *out, float sign, float bound) {
  if (n == 0) return 0;
  int m = 0;
  float2 cur = in[0];
  float dc = bound - sign * (AXIS == 0 ? cur.x : cur.y);
  for (int k = 1; k <= n; ++k) {
    const float2 nxt = in[(k == n ? 0 : k) * kPairThreads];
    const float dn = bound - sign * (AXIS == 0 ? nxt.x : nxt.y);
    const bool ic = dc >= 0.f, inx = dn >= 0.f;
    if (ic && m < kPolyMax) out[(m++) * kPairThreads] = cur;
    if (ic != inx && m < kPolyMax) {
      const float t = dc / (dc - dn);
      float2 p;
      p.x = AXIS == 0 ? sign * bound : cur.x + t * (nxt.x - cur.x);
      p.y = AXIS == 1 ? sign * bound : cur.y + t * (nxt.y - cur.y);
      out[(m++) * kPairThreads] = p;
    }
    cur = nxt, dc = dn;
  }
  return m;
}

// Intersection area of box b with box a, in a's frame.  poly: this thread's column of the two LDS polygon buffers.
__device__ float pair_intersection(const PairBox &a, const PairBox &b, float2 *poly) {
  const float dx = b.x - a.x, dy = b.y - a.y;
  const float ex = dx * a.c + dy * a.s, ey = dy * a.c - dx * a.s;
  const float ux = b.ux * a.c + b.uy * a.s, uy = b.uy * a.c - b.ux * a.s;
  const float vx = b.vx * a.c + b.vy * a.s, vy = b.vy * a.c - b.vx * a.s;
  float2 *p0 = poly, *p1 = poly + kPolyMax * kPairThreads;
  p0[0 * kPairThreads] = make_float2(ex + ux + vx, ey + uy + vy);
  p0[1 * kPairThreads] = make_float2(ex - ux + vx, ey - uy + vy);
  p0[2 * kPairThreads] = make_float2(ex - ux - vx, ey - uy - vy);
  p0[3 * kPairThreads] = make_float2(ex + ux - vx, ey + uy - vy);
  int n = clip_stage<0>(p0, 4, p1, 1.f, a.hw);
  n = clip_stage<0>(p1, n, p0, -1.f, a.hw);
  n = clip_stage<1>(p0, n, p1, 1.f, a.hl);
  n = clip_stage<1>(p1, n, p0, -1.f, a.hl);
  if (n < 3) return 0.f;
  float twice = 0.f;
  float2 cur = p0[0];
  for (int k = 1; k <= n; ++k) {
    const float2 nxt = p0[(k == n ? 0 : k) * kPairThreads];
    twice += cur.x * nxt.y - nxt.x * cur.y;
    cur = nxt;
  }
  return 0.5f * fabsf(twice);
}

// IoU of a and b; 0 when the circumcircles are apart, when the union is not positive or when a NaN is involved.
// nan: set when a NaN is involved (then no comparison with the result may hold).
__device__ __forceinline__ float pair_iou(const PairBox &a, const PairBox &b, float2 *poly, bool &nan) {
  const float dx = b.x - a.x, dy = b.y - a.y;
  const float d2 = dx * dx + dy * dy, r = a.rad + b.rad;
  nan = !(d2 + r == d2 + r);
  float iou = 0.f;
  if (d2 <= r * r) {   // (false for NaN)
    const float inter = pair_intersection(a, b, poly);
    const float uni = a.area + b.area - inter;
    if (uni > 0.f) iou = inter / uni;
  }
  return iou;
}

__device__ __forceinline__ PairBox load_pair_box(const float *row) {
  PairBox b;
  b.x = row[0], b.y = row[1], b.hw = row[2], b.hl = row[3], b.c = row[4], b.s = row[5];
  b.ux = row[6], b.uy = row[7], b.vx = row[8], b.vy = row[9], b.area = row[10], b.rad = row[11];
  return b;
}

struct NmsWs {   // carve of the caller's workspace; strides in rows of Kmax
  int32_t *ranked;   // [batch] rows that entered the scan
  int32_t *index;    // [batch, Kmax] input row of each ranked row
  float *rows;       // [batch, Kmax, kRowFloats]
  u64 *mask;         // [batch, Kmax, words]
};
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t nms_ws_bytes(size_t batch, size_t kmax) {
  const size_t words = (kmax + 63) / 64;
  return round_up(batch * 4, 16) + round_up(batch * kmax * 4, 16) + batch * kmax * kRowFloats * 4 +
         batch * kmax * words * 8;
}
inline NmsWs nms_ws_carve(void *ws, size_t batch, size_t kmax) {
  char *p = static_cast<char *>(ws);
  NmsWs w;
  w.ranked = reinterpret_cast<int32_t *>(p);
  p += round_up(batch * 4, 16);
  w.index = reinterpret_cast<int32_t *>(p);
  p += round_up(batch * kmax * 4, 16);
  w.rows = reinterpret_cast<float *>(p);
  p += batch * kmax * kRowFloats * 4;
  w.mask = reinterpret_cast<u64 *>(p);
  return w;
}

extern __shared__ __attribute__((aligned(16))) char nms_smem[];

// Launch 1: rank the valid rows of item b, cut to kmax, write the scaled boxes in pair-test form.
__global__ __launch_bounds__(kDecThreads) void nms_rank_kernel(const float *__restrict__ boxes_in,
                                                               const float *__restrict__ scores_in,
                                                               const int32_t *__restrict__ labels_in,
                                                               const int32_t *__restrict__ count_in, NmsWs ws,
                                                               unsigned num, unsigned kmax, unsigned cap, int idx_bytes,
                                                               Factors fac) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  int cnt = count_in ? count_in[b] : (int)num;
  cnt = cnt < 0 ? 0 : cnt;
  const unsigned n = min((unsigned)cnt, num);
  const unsigned K = min(n, kmax);
  if (t == 0) ws.ranked[b] = (int32_t)K;
  if (K == 0) return;   // (uniform: every thread read the same count)
  const DecLds l = carve(nms_smem, cap);
  const ScoreSrc src{scores_in + (size_t)b * num};
  if (K == n) {   // nothing to select: sort all of them
    for (unsigned i = t; i < cap; i += kDecThreads) l.list[i] = i < n ? src(i) : kSentinel;
    __syncthreads();
    block_sort(cap, l);
  } else {
    block_topk(src, n, K, cap, idx_bytes, true, l);
  }
  for (unsigned r = t; r < K; r += kDecThreads) {
    const unsigned idx = (unsigned)l.list[r];
    if (idx >= n) continue;   // (never: a sentinel must not become an address)
    const float *p = boxes_in + ((size_t)b * num + idx) * 9;
    const float f = fac.n ? factor_of(fac, labels_in[(size_t)b * num + idx]) : 1.0f;
    const PairBox pb = make_pair_box(p[0], p[1], mul_rn(p[3], f), mul_rn(p[4], f), p[6]);
    float *row = ws.rows + ((size_t)b * kmax + r) * kRowFloats;
    row[0] = pb.x, row[1] = pb.y, row[2] = pb.hw, row[3] = pb.hl, row[4] = pb.c, row[5] = pb.s;
    row[6] = pb.ux, row[7] = pb.uy, row[8] = pb.vx, row[9] = pb.vy, row[10] = pb.area, row[11] = pb.rad;
    ws.index[(size_t)b * kmax + r] = (int32_t)idx;
  }
}

// Launch 2: grid (words, ceil(kmax / 4), batch), one wave per (row i, word): bit j of the word = "row i suppresses
// column 64 * word + j".  MODE 0: IoU > thr; 1: squared centre distance <= thr.
template <int MODE>
__global__ __launch_bounds__(kPairThreads) void nms_mask_kernel(NmsWs ws, unsigned kmax, unsigned words, float thr) {
  __shared__ float2 poly[MODE == 0 ? 2 * kPolyMax * kPairThreads : 1];
  const unsigned b = blockIdx.z, word = blockIdx.x, lane = threadIdx.x & 63u;
  const unsigned i = __builtin_amdgcn_readfirstlane(blockIdx.y * (kPairThreads / kWave) + (threadIdx.x >> 6));
  if (i >= kmax) return;
  u64 *out = ws.mask + ((size_t)b * kmax + i) * words + word;
  const unsigned M = (unsigned)ws.ranked[b];
  const unsigned j = word * 64u + lane;
  if (i >= M || word * 64u + 63u <= i) {   // no row, or every column of the word at or before the row
    if (lane == 0) *out = 0;
    return;
  }
  const float *rows = ws.rows + (size_t)b * kmax * kRowFloats;
  const float *ri = rows + (size_t)i * kRowFloats;
  bool sup = false;
  if (j > i && j < M) {
    const float *rj = rows + (size_t)j * kRowFloats;
    if constexpr (MODE == 0) {
      const PairBox a = load_pair_box(ri), c = load_pair_box(rj);
      bool nan;
      const float iou = pair_iou(a, c, poly + threadIdx.x, nan);
      sup = !nan && iou > thr;
    } else {
      // (x_i - x_j)^2 + (y_i - y_j)^2, every operation rounded on its own (box3d_nms.py:216)
      const float dx = sub_rn(ri[0], rj[0]), dy = sub_rn(ri[1], rj[1]);
      sup = add_rn(mul_rn(dx, dx), mul_rn(dy, dy)) <= thr;
    }
  }
  const u64 m = __ballot(sup);
  if (lane == 0) *out = m;
}

__device__ __forceinline__ u64 readlane64(u64 v, unsigned lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)lane);
  return ((u64)hi << 32) | lo;
}

// Launch 3: one block per item.  Dynamic LDS: chunk_rows * words mask words, then kmax kept ranks, then the count.
__global__ __launch_bounds__(kScanThreads) void nms_scan_kernel(
    const float *__restrict__ boxes_in, const float *__restrict__ scores_in, const int32_t *__restrict__ labels_in,
    NmsWs ws, float *__restrict__ boxes, float *__restrict__ scores, int32_t *__restrict__ labels,
    int32_t *__restrict__ count, int32_t *__restrict__ index, unsigned num, unsigned kmax, unsigned words,
    unsigned chunk_rows, unsigned post, Factors fac, int bottom_center) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  u64 *stage = reinterpret_cast<u64 *>(nms_smem);
  unsigned *kept = reinterpret_cast<unsigned *>(nms_smem + (size_t)chunk_rows * words * 8);
  unsigned *total = kept + kmax;
  const unsigned M = min((unsigned)ws.ranked[b], kmax);
  const u64 *mask = ws.mask + (size_t)b * kmax * words;
  u64 removed = 0;   // wave 0, lane w: word w of the suppressed set
  unsigned nkept = 0;
  for (unsigned row0 = 0; row0 < M; row0 += chunk_rows) {   // (M, nkept, post uniform: every thread takes the same trips)
    const unsigned rows = min(chunk_rows, M - row0);
    for (unsigned e = t; e < rows * words; e += kScanThreads) stage[e] = mask[(size_t)row0 * words + e];
    __syncthreads();
    if (t < (unsigned)kWave) {
      for (unsigned w = row0 / 64u; w * 64u < row0 + rows && nkept < post; ++w) {
        const unsigned left = M - w * 64u;   // rows of this word that exist
        u64 cand = ~readlane64(removed, w) & (left >= 64u ? ~0ull : ((1ull << left) - 1ull));
        while (cand != 0 && nkept < post) {
          const unsigned bit = (unsigned)__ffsll((long long)cand) - 1u;
          const unsigned i = w * 64u + bit;
          if (t == 0) kept[nkept] = i;
          ++nkept;
          const u64 row = t < words ? stage[(size_t)(i - row0) * words + t] : 0ull;
          removed |= row;
          cand &= ~readlane64(row, w);
          cand &= ~((2ull << bit) - 1ull);   // rows at and before i are decided
        }
      }
      if (t == 0) *total = nkept;
    }
    __syncthreads();   // stage is refilled by the next round; total is rewritten only behind the next barrier
    if (*total >= post) break;   // (uniform)
  }
  if (t == 0) *total = nkept;
  __syncthreads();
  nkept = *total;
  const size_t out0 = (size_t)b * post;
  for (unsigned r = t; r < post; r += kScanThreads) {
    float box[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s = 0.f;
    int label = 0, idx = 0;
    if (r < nkept) {
      idx = ws.index[(size_t)b * kmax + kept[r]];
      const size_t at = (size_t)b * num + (unsigned)idx;
#pragma unroll
      for (int c = 0; c < 9; ++c) box[c] = boxes_in[at * 9 + c];
      s = scores_in[at];
      label = labels_in[at];
      if (fac.n) {   // the reference multiplies in place and divides back (centerpoint_head.py:836-876)
        const float f = factor_of(fac, label);
#pragma unroll
        for (int c = 3; c < 6; ++c) box[c] = mul_rn(box[c], f) / f;
      }
      if (bottom_center) box[2] = sub_rn(box[2], mul_rn(box[5], 0.5f));
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) boxes[(out0 + r) * 9 + c] = box[c];
    scores[out0 + r] = s;
    labels[out0 + r] = label;
    if (index) index[out0 + r] = idx;
  }
  if (t == 0) count[b] = (int32_t)nkept;
}

__global__ __launch_bounds__(kPairThreads) void bev_iou_kernel(const float *__restrict__ a, unsigned na,
                                                               const float *__restrict__ bx, unsigned nb,
                                                               float *__restrict__ iou) {
  __shared__ float2 poly[2 * kPolyMax * kPairThreads];
  const size_t e = (size_t)blockIdx.x * kPairThreads + threadIdx.x;
  if (e >= (size_t)na * nb) return;
  const float *pa = a + (e / nb) * 5, *pb = bx + (e % nb) * 5;
  const PairBox A = make_pair_box(pa[0], pa[1], pa[2], pa[3], pa[4]);
  const PairBox B = make_pair_box(pb[0], pb[1], pb[2], pb[3], pb[4]);
  bool nan;
  const float v = pair_iou(A, B, poly + threadIdx.x, nan);
  iou[e] = nan ? __uint_as_float(0x7fc00000u) : v;
}

inline bool finite_f(float v) { return v == v && v <= 3.4028234e38f && v >= -3.4028234e38f; }
inline unsigned nms_kmax(int num, int pre_max_size) {
  return (unsigned)((pre_max_size > 0 && pre_max_size < num) ? pre_max_size : num);
}
inline unsigned scan_chunk_rows(unsigned kmax, unsigned words) {
  unsigned rows = (unsigned)(kScanChunkBytes / (words * 8)) / 64u * 64u;
  if (rows < 64u) rows = 64u;
  const unsigned all = (kmax + 63u) / 64u * 64u;
  return rows < all ? rows : all;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_bev_nms_workspace_size(int batch, int num) {
  if (batch < 1 || num < 1 || num > kNmsMaxRows) return 0;
  return nms_ws_bytes((size_t)batch, (size_t)num);
}

extern "C" int bevops_bev_nms(int mode, const float *boxes_in, const float *scores_in, const int32_t *labels_in,
                              const int32_t *count_in, float *boxes, float *scores, int32_t *labels, int32_t *count,
                              int32_t *index, int batch, int num, int pre_max_size, int post_max_size, float threshold,
                              const float *rescale_factor_host, int num_factors, int bottom_center, void *workspace,
                              size_t workspace_bytes, void *stream) {
  if (!boxes_in || !scores_in || !labels_in || !boxes || !scores || !labels || !count || !workspace)
    return BEVOPS_BAD_PARAM;
  if (mode != 0 && mode != 1) return BEVOPS_BAD_PARAM;
  if (batch < 1 || num < 1 || num_factors < 0 || (num_factors > 0 && !rescale_factor_host)) return BEVOPS_BAD_PARAM;
  if (num > kNmsMaxRows || batch > 65535 || num_factors > kNmsMaxFactors) return BEVOPS_NOT_SUPPORTED;
  if (post_max_size < 1 || post_max_size > num || !finite_f(threshold)) return BEVOPS_BAD_PARAM;
  Factors fac;
  fac.n = num_factors;
  for (int i = 0; i < kNmsMaxFactors; ++i) fac.v[i] = 1.0f;
  for (int i = 0; i < num_factors; ++i) {
    if (!finite_f(rescale_factor_host[i]) || !(rescale_factor_host[i] > 0.f)) return BEVOPS_BAD_PARAM;
    fac.v[i] = rescale_factor_host[i];
  }
  if (workspace_bytes < bevops_bev_nms_workspace_size(batch, num) || (reinterpret_cast<uintptr_t>(workspace) & 7u))
    return BEVOPS_BAD_PARAM;
  const unsigned kmax = nms_kmax(num, pre_max_size), words = (kmax + 63u) / 64u;
  const NmsWs ws = nms_ws_carve(workspace, (size_t)batch, kmax);   // (kmax <= num: inside the checked size)
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned cap = pow2_at_least(kmax);
  hipLaunchKernelGGL(nms_rank_kernel, dim3((unsigned)batch), dim3(kDecThreads), lds_bytes(cap), st, boxes_in, scores_in,
                     labels_in, count_in, ws, (unsigned)num, kmax, cap, index_bytes((unsigned)num), fac);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  const dim3 grid(words, (kmax + kPairThreads / kWave - 1) / (kPairThreads / kWave), (unsigned)batch);
  if (mode == 0)
    hipLaunchKernelGGL(nms_mask_kernel<0>, grid, dim3(kPairThreads), 0, st, ws, kmax, words, threshold);
  else
    hipLaunchKernelGGL(nms_mask_kernel<1>, grid, dim3(kPairThreads), 0, st, ws, kmax, words, threshold);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  const unsigned chunk = scan_chunk_rows(kmax, words);
  const size_t lds = (size_t)chunk * words * 8 + (size_t)kmax * 4 + 16;   // <= 48 KiB + 16 KiB + 16
  hipLaunchKernelGGL(nms_scan_kernel, dim3((unsigned)batch), dim3(kScanThreads), lds, st, boxes_in, scores_in, labels_in,
                     ws, boxes, scores, labels, count, index, (unsigned)num, kmax, words, chunk, (unsigned)post_max_size,
                     fac, bottom_center);
  return launch_status();
}

extern "C" int bevops_bev_iou(const float *boxes_a, int num_a, const float *boxes_b, int num_b, float *iou,
                              void *stream) {
  if (!boxes_a || !boxes_b || !iou || num_a < 1 || num_b < 1) return BEVOPS_BAD_PARAM;
  const long long pairs = (long long)num_a * num_b;
  if (pairs > (1ll << 30)) return BEVOPS_NOT_SUPPORTED;
  const unsigned blocks = (unsigned)((pairs + kPairThreads - 1) / kPairThreads);
  hipLaunchKernelGGL(bev_iou_kernel, dim3(blocks), dim3(kPairThreads), 0, static_cast<hipStream_t>(stream), boxes_a,
                     (unsigned)num_a, boxes_b, (unsigned)num_b, iou);
  return launch_status();
}
