// Non-maximum suppression on the device, one pipeline with two entries.
// bevops_bev_nms: the rotated scale-NMS of CenterHead.get_task_detections and the circle NMS of CenterHead.get_bboxes,
// with the size restore and the z shift that follow them.  Reference:
//   third_party/bev_mmdet3d/models/dense_heads/centerpoint_head.py:747-806 (get_bboxes), :808-905 (get_task_detections),
//   third_party/bev_mmdet3d/core/post_processing/box3d_nms.py:182-221 (circle_nms), :227-273 (nms_bev).
// bevops_box_nms: the axis-aligned batched NMS behind the 2-D decoders of csrc/decode2d.hip (mmcv.ops.batched_nms with
// mmdet's valid_mask in front, as det2trt/models/detector/{centernet,yolox}.py call it; design/postprocess.md).
// Fixed-capacity outputs like the decoders' (csrc/decode.hip): kept rows in rank order at the front, zero behind
// count[b]; nothing is read back by the host, no launch is sized by a device value, so the call can be captured.
//
// Three launches, each one kernel template (design/postprocess.md has the table of the two instantiations):
//   1. rank: one block per item puts the candidates' 64-bit keys of topk.h (score descending, lower row first) in order
//      -- BEV: the rows below count, cut to pre_max_size; box: the rows below count with score >= threshold, as many as
//      there are -- and writes, per ranked row, the floats the pair test reads and the input row number.
//   2. mask: a grid of waves strides over the (ranked row i, 64-column word) pairs on or above the diagonal among the M
//      ranked rows: lane = column j, the row is wave-uniform, the word is the ballot of the pair test (rotated IoU,
//      circle distance, axis-aligned IoU with label test).  Nothing else of the mask is written, nothing else read.
//   3. scan: wave 0 of one block per item holds the running suppressed set, lane w owning words w, w + 64, ...; rows of
//      the mask are staged into LDS a round ahead by the whole block; then the whole block gathers the kept rows.
// No atomics apart from LDS integer counters whose order is erased by a sort (the histogram of topk.h, the candidate
// collection of the box entry's launch 1).
//
// Pair test, rotate: IoU of the two rotated rectangles, evaluated in the frame of box i (centre at the origin, axes
// along the box): box j's four corners are clipped against the four axis-aligned edges of box i (Sutherland-Hodgman;
// the polygon lives in LDS, one column per thread, because its length is data-dependent).  Relative coordinates keep
// the fp32 error near 1e-6 where absolute coordinates at +-50 m lose three decades (design/postprocess.md).
#include "detect.h"

namespace bevops {
namespace {

constexpr int kNmsMaxRows = 4096;      // num of bevops_bev_nms: 64 words of 64 columns, one per lane of the scan wave
constexpr int kBoxMaxRows = 16384;     // num of bevops_box_nms: 256 words, four per lane
constexpr int kNmsMaxFactors = 64;     // rescale factors travel as a kernel argument
constexpr int kPairThreads = 256;      // block of the mask / IoU kernels
constexpr int kMaskBlocks = 2048;      // at most 8 192 waves stride over the (row, word) pairs
constexpr int kPolyMax = 8;            // a quadrilateral clipped by four half-planes has at most eight vertices
constexpr int kBevRowFloats = 12;      // x, y, w/2, l/2, cos, sin, ux, uy, vx, vy, area, circumradius
constexpr int kBoxRowFloats = 6;       // x1, y1, x2, y2, area, label (as bits)
constexpr int kScanThreads = kDecThreads;    // (write_row / zero_tail of detect.h stride by it)
constexpr int kBevStageBytes = 48 * 1024;    // mask rows staged in LDS per round of the scan: as many as fit
constexpr int kBoxStageBytes = 64 * 1024;    // ... and for the box entry at most
constexpr int kBoxStageRows = 64;            // one 64-row word per round

__device__ __forceinline__ bool finite_dev(float v) { return fabsf(v) <= 3.4028234e38f; }   // (false for NaN)

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

struct NmsWs {   // carve of the caller's workspace; stride = rows an item can rank, words = ceil(stride / 64)
  int32_t *ranked;   // [batch] rows that entered the scan
  int32_t *index;    // [batch, stride] input row of each ranked row
  float *rows;       // [batch, stride, row floats] what the pair test reads
  u64 *mask;         // [batch, stride, words]; written on and above the diagonal of the ranked rows only
  unsigned stride, words;
};
inline size_t nms_ws_bytes(size_t batch, size_t stride, size_t row_floats) {
  const size_t words = (stride + 63) / 64;
  return round_up(batch * 4, 16) + round_up(batch * stride * 4, 16) + round_up(batch * stride * row_floats * 4, 16) +
         batch * stride * words * 8;
}
inline NmsWs nms_ws_carve(void *ws, size_t batch, size_t stride, size_t row_floats) {
  char *p = static_cast<char *>(ws);
  NmsWs w;
  w.ranked = reinterpret_cast<int32_t *>(p);
  p += round_up(batch * 4, 16);
  w.index = reinterpret_cast<int32_t *>(p);
  p += round_up(batch * stride * 4, 16);
  w.rows = reinterpret_cast<float *>(p);
  p += round_up(batch * stride * row_floats * 4, 16);
  w.mask = reinterpret_cast<u64 *>(p);
  w.stride = (unsigned)stride, w.words = (unsigned)((stride + 63) / 64);
  return w;
}

// ---- launch 1, candidate policies: leave the item's candidates among scores[0..n) as ascending keys in
// l.list[0..M) and return M (uniform).  Every thread of the block calls them.
struct TopCandidates {   // every row below count, cut to kmax
  unsigned kmax;
  int idx_bytes;
  __device__ __forceinline__ unsigned operator()(const DecLds &l, const float *scores, unsigned n, unsigned cap) const {
    const unsigned t = threadIdx.x;
    const unsigned K = min(n, kmax);
    if (K == 0) return 0;
    const ScoreSrc src{scores};
    if (K == n) {   // nothing to select: sort all of them
      for (unsigned i = t; i < cap; i += kDecThreads) l.list[i] = i < n ? src(i) : kSentinel;
      __syncthreads();
      block_sort(cap, l);
    } else {
      block_topk(src, n, K, cap, idx_bytes, true, l);
    }
    return K;
  }
};
struct ThresholdCandidates {   // rows below count with score >= threshold, as many as there are
  float score_threshold;
  __device__ __forceinline__ unsigned operator()(const DecLds &l, const float *scores, unsigned n, unsigned) const {
    const unsigned t = threadIdx.x;
    if (t == 0) l.sel[2] = 0;
    __syncthreads();
    for (unsigned i = t; i < n; i += kDecThreads) {
      const float s = scores[i];
      if (s >= score_threshold) {   // (false for NaN)
        const unsigned slot = atomicAdd(&l.sel[2], 1u);   // the order is erased by the sort
        l.list[slot] = ((u64)rank_bits(s) << 32) | i;
      }
    }
    __syncthreads();
    const unsigned M = l.sel[2];
    if (M == 0) return 0;
    unsigned cap = 1;
    while (cap < M) cap <<= 1;   // <= the carve's capacity: M <= num
    for (unsigned i = M + t; i < cap; i += kDecThreads) l.list[i] = kSentinel;
    __syncthreads();
    block_sort(cap, l);
    return M;
  }
};

// ---- launch 1, row writers: input row p (kIn columns) and its label -> the kFloats the pair test reads
struct PairRow {   // the scaled box in pair-box form
  static constexpr int kIn = 9, kFloats = kBevRowFloats;
  Factors fac;
  __device__ __forceinline__ void operator()(const float *p, int label, float *row) const {
    const float f = fac.n ? factor_of(fac, label) : 1.0f;
    const PairBox pb = make_pair_box(p[0], p[1], mul_rn(p[3], f), mul_rn(p[4], f), p[6]);
    row[0] = pb.x, row[1] = pb.y, row[2] = pb.hw, row[3] = pb.hl, row[4] = pb.c, row[5] = pb.s;
    row[6] = pb.ux, row[7] = pb.uy, row[8] = pb.vx, row[9] = pb.vy, row[10] = pb.area, row[11] = pb.rad;
  }
};
struct CornerRow {   // x1, y1, x2, y2, area (NaN for a non-finite corner), label as bits
  static constexpr int kIn = 4, kFloats = kBoxRowFloats;
  __device__ __forceinline__ void operator()(const float *p, int label, float *row) const {
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    float area = mul_rn(sub_rn(x2, x1), sub_rn(y2, y1));
    if (!(finite_dev(x1) && finite_dev(y1) && finite_dev(x2) && finite_dev(y2))) area = __uint_as_float(0x7fc00000u);
    row[0] = x1, row[1] = y1, row[2] = x2, row[3] = y2, row[4] = area;
    row[5] = __int_as_float(label);
  }
};

// Launch 1: one block per item ranks its candidates and writes, per ranked row, the pair-test row and the input row.
// Dynamic LDS: the selection's carve for cap keys.
template <class Cand, class Row>
__global__ __launch_bounds__(kDecThreads) void nms_rank_kernel(const float *__restrict__ boxes_in,
                                                               const float *__restrict__ scores_in,
                                                               const int32_t *__restrict__ labels_in,
                                                               const int32_t *__restrict__ count_in, NmsWs ws, unsigned num,
                                                               unsigned cap, Cand cand, Row row) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  int cnt = count_in ? count_in[b] : (int)num;
  cnt = cnt < 0 ? 0 : cnt;
  const unsigned n = min((unsigned)cnt, num);
  const DecLds l = carve(det_smem, cap);
  const unsigned M = cand(l, scores_in + (size_t)b * num, n, cap);
  if (t == 0) ws.ranked[b] = (int32_t)M;
  for (unsigned r = t; r < M; r += kDecThreads) {
    const unsigned idx = (unsigned)l.list[r];
    if (idx >= n) continue;   // (never: a sentinel must not become an address)
    row(boxes_in + ((size_t)b * num + idx) * Row::kIn, labels_in[(size_t)b * num + idx],
        ws.rows + ((size_t)b * ws.stride + r) * Row::kFloats);
    ws.index[(size_t)b * ws.stride + r] = (int32_t)idx;
  }
}

// ---- launch 2, pair tests: does ranked row ri suppress the later row rj?  poly: this thread's LDS polygon column.
struct RotatedIou {
  static constexpr int kFloats = kBevRowFloats;
  static constexpr bool kPoly = true;
  float thr;
  __device__ __forceinline__ bool operator()(const float *ri, const float *rj, float2 *poly) const {
    const PairBox a = load_pair_box(ri), c = load_pair_box(rj);
    bool nan;
    const float iou = pair_iou(a, c, poly, nan);
    return !nan && iou > thr;
  }
};
struct CircleDistance {   // (x_i - x_j)^2 + (y_i - y_j)^2, every operation rounded on its own (box3d_nms.py:216)
  static constexpr int kFloats = kBevRowFloats;
  static constexpr bool kPoly = false;
  float thr;
  __device__ __forceinline__ bool operator()(const float *ri, const float *rj, float2 *) const {
    const float dx = sub_rn(ri[0], rj[0]), dy = sub_rn(ri[1], rj[1]);
    return add_rn(mul_rn(dx, dx), mul_rn(dy, dy)) <= thr;
  }
};
struct AlignedIou {
  static constexpr int kFloats = kBoxRowFloats;
  static constexpr bool kPoly = false;
  float thr;
  int class_aware;
  __device__ __forceinline__ bool operator()(const float *ri, const float *rj, float2 *) const {
    const float iw = fmaxf(sub_rn(fminf(ri[2], rj[2]), fmaxf(ri[0], rj[0])), 0.f);
    const float ih = fmaxf(sub_rn(fminf(ri[3], rj[3]), fmaxf(ri[1], rj[1])), 0.f);
    const float inter = mul_rn(iw, ih);
    const float iou = inter / sub_rn(add_rn(ri[4], rj[4]), inter);   // NaN area: NaN, compares false
    return iou > thr && (!class_aware || __float_as_int(ri[5]) == __float_as_int(rj[5]));
  }
};

// Launch 2: grid (blocks, batch); wave v takes the pairs v, v + waves, ... of (row i, word) with i < M and
// word < ceil(M / 64), and evaluates those on or above the diagonal: lane = column, the row is wave-uniform, the word
// is the ballot of the pair test.  Nothing is written for rows >= M or below the diagonal; launch 3 never reads there.
template <class Pair>
__global__ __launch_bounds__(kPairThreads) void nms_mask_kernel(NmsWs ws, Pair pair) {
  __shared__ float2 poly[Pair::kPoly ? 2 * kPolyMax * kPairThreads : 1];
  const unsigned b = blockIdx.y, lane = threadIdx.x & 63u;
  const unsigned M = min((unsigned)max(ws.ranked[b], 0), ws.stride);
  const unsigned Mw = (M + 63u) / 64u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kPairThreads / kWave) + (threadIdx.x >> 6));
  const unsigned nwaves = gridDim.x * (kPairThreads / kWave);
  const float *rows = ws.rows + (size_t)b * ws.stride * Pair::kFloats;
  u64 *mask = ws.mask + (size_t)b * ws.stride * ws.words;
  for (unsigned task = wave; task < M * Mw; task += nwaves) {   // (M Mw <= 2^22)
    const unsigned i = task / Mw, word = task % Mw;
    if (word < i / 64u) continue;   // below the diagonal; the diagonal word is always written (launch 3 reads it)
    const unsigned j = word * 64u + lane;
    bool sup = false;
    if (j > i && j < M) sup = pair(rows + (size_t)i * Pair::kFloats, rows + (size_t)j * Pair::kFloats, poly + threadIdx.x);
    const u64 m = __ballot(sup);
    if (lane == 0) mask[(size_t)i * ws.words + word] = m;
  }
}

// ---- launch 3, fix-ups of a gathered row
struct NoFix {
  __device__ __forceinline__ void operator()(float *, int) const {}
};
struct SizeRestore {   // the reference multiplies in place and divides back (centerpoint_head.py:836-876); z shift of :793
  Factors fac;
  int bottom_center;
  __device__ __forceinline__ void operator()(float *box, int label) const {
    if (fac.n) {
      const float f = factor_of(fac, label);
#pragma unroll
      for (int c = 3; c < 6; ++c) box[c] = mul_rn(box[c], f) / f;
    }
    if (bottom_center) box[2] = sub_rn(box[2], mul_rn(box[5], 0.5f));
  }
};

// Launch 3: one block per item.  Wave 0 holds the suppressed set, lane w owning words w, w + 64, .. (WPL of them: 1
// covers 4 096 rows, 4 covers 16 384); the block stages stage_rows mask rows per round in LDS (a multiple of 64, or 32);
// then the block gathers the kept rows (W box columns) and zeroes the rest.
// Dynamic LDS: stage_rows * words mask words, then post kept ranks, then the count.
template <int WPL, int W, class Fix>
__global__ __launch_bounds__(kScanThreads) void nms_scan_kernel(
    const float *__restrict__ boxes_in, const float *__restrict__ scores_in, const int32_t *__restrict__ labels_in,
    NmsWs ws, float *__restrict__ boxes, float *__restrict__ scores, int32_t *__restrict__ labels,
    int32_t *__restrict__ count, int32_t *__restrict__ index, unsigned num, unsigned stage_rows, unsigned post, Fix fix) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  u64 *stage = reinterpret_cast<u64 *>(det_smem);
  unsigned *kept = reinterpret_cast<unsigned *>(det_smem + (size_t)stage_rows * ws.words * 8);
  unsigned *total = kept + post;
  const unsigned M = min((unsigned)max(ws.ranked[b], 0), ws.stride);
  const unsigned Mw = (M + 63u) / 64u;
  const u64 *mask = ws.mask + (size_t)b * ws.stride * ws.words;
  u64 removed[WPL];
#pragma unroll
  for (int s = 0; s < WPL; ++s) removed[s] = 0;
  unsigned nkept = 0;
  for (unsigned row0 = 0; row0 < M; row0 += stage_rows) {   // (M, nkept, post uniform: every thread takes the same trips)
    const unsigned rows = min(stage_rows, M - row0);
    const unsigned w0 = __builtin_amdgcn_readfirstlane(row0 / 64u);   // the first word these rows are bits of
    for (unsigned e = t; e < rows * Mw; e += kScanThreads) {   // staged row r at pitch Mw
      const unsigned r = e / Mw, c = e % Mw;
      if (c >= w0) stage[e] = mask[(size_t)(row0 + r) * ws.words + c];   // words below the round's diagonal: never read
    }
    __syncthreads();
    if (t < (unsigned)kWave) {
      for (unsigned wv = w0; wv * 64u < row0 + rows && nkept < post; ++wv) {
        const unsigned w = __builtin_amdgcn_readfirstlane(wv);   // the word whose bits these rows are
        const unsigned lo = max(row0, w * 64u) - w * 64u, hi = min(row0 + rows, w * 64u + 64u) - w * 64u;
        const u64 range = (hi - lo >= 64u ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo;   // this round's rows of the word
        u64 mine = removed[0];   // the lane's word of the class word w is in; then lane w & 63 holds word w
#pragma unroll
        for (unsigned s = 1; s < (unsigned)WPL; ++s) mine = (w >> 6) == s ? removed[s] : mine;
        u64 cand = ~readlane64(mine, w & 63u) & range;
        while (cand != 0 && nkept < post) {
          const unsigned bit = (unsigned)__ffsll((long long)cand) - 1u;
          const unsigned i = w * 64u + bit;
          if (t == 0) kept[nkept] = i;
          ++nkept;
          u64 own = 0;   // row i's bits of the class word w is in
#pragma unroll
          for (unsigned s = 0; s < (unsigned)WPL; ++s) {
            const unsigned c = s * 64u + t;
            const u64 row = (c >= w && c < Mw) ? stage[(size_t)(i - row0) * Mw + c] : 0ull;
            removed[s] |= row;
            own = (s == 0 || (w >> 6) == s) ? row : own;
          }
          cand &= ~readlane64(own, w & 63u);
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
  for (unsigned r = t; r < nkept; r += kScanThreads) {
    const int idx = ws.index[(size_t)b * ws.stride + kept[r]];
    const size_t at = (size_t)b * num + (unsigned)idx;
    float box[W];
#pragma unroll
    for (int c = 0; c < W; ++c) box[c] = boxes_in[at * W + c];
    const int label = labels_in[at];
    fix(box, label);
    write_row<W>(boxes, scores, labels, out0 + r, box, scores_in[at], label);
    if (index) index[out0 + r] = idx;
  }
  zero_tail<W>(boxes, scores, labels, index, out0, nkept, post);
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

inline unsigned nms_kmax(int num, int pre_max_size) {
  return (unsigned)((pre_max_size > 0 && pre_max_size < num) ? pre_max_size : num);
}
// Mask rows per round of the scan: what fits the budget, in whole 64-row words (32 rows where not even one word
// fits), at most `most` and no more than there are rows.
inline unsigned scan_stage_rows(const NmsWs &ws, unsigned budget_bytes, unsigned most) {
  unsigned rows = budget_bytes / (ws.words * 8u) / 64u * 64u;
  if (rows < 64u) rows = 32u;
  if (rows > most) rows = most;
  const unsigned all = (ws.stride + 63u) / 64u * 64u;
  return rows < all ? rows : all;
}

// The three launches.  MAXROWS: the entry's row limit (decides whether the 4-words-per-lane scan exists for it).
template <int MAXROWS, int W, class Cand, class Row, class Pair, class Fix>
int launch_nms(const float *boxes_in, const float *scores_in, const int32_t *labels_in, const int32_t *count_in,
               float *boxes, float *scores, int32_t *labels, int32_t *count, int32_t *index, const NmsWs &ws, int batch,
               int num, unsigned cap, unsigned stage_rows, int post, const Cand &cand, const Row &row, const Pair &pair,
               const Fix &fix, hipStream_t st) {
  const size_t lds1 = lds_bytes(cap);
  if (!ensure_dynamic_lds<nms_rank_kernel<Cand, Row>>(lds1)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL((nms_rank_kernel<Cand, Row>), dim3((unsigned)batch), dim3(kDecThreads), lds1, st, boxes_in, scores_in,
                     labels_in, count_in, ws, (unsigned)num, cap, cand, row);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  const unsigned waves = kPairThreads / kWave, tasks = ws.stride * ws.words;
  const unsigned blocks = min((tasks + waves - 1) / waves, (unsigned)kMaskBlocks);
  hipLaunchKernelGGL(nms_mask_kernel<Pair>, dim3(blocks, (unsigned)batch), dim3(kPairThreads), 0, st, ws, pair);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  const size_t lds3 = (size_t)stage_rows * ws.words * 8 + (size_t)post * 4 + 16;   // <= 64 KiB + 64 KiB + 16
  if (MAXROWS <= 64 * kWave || ws.words <= (unsigned)kWave) {
    if (!ensure_dynamic_lds<nms_scan_kernel<1, W, Fix>>(lds3)) return BEVOPS_FAILURE;
    hipLaunchKernelGGL((nms_scan_kernel<1, W, Fix>), dim3((unsigned)batch), dim3(kScanThreads), lds3, st, boxes_in,
                       scores_in, labels_in, ws, boxes, scores, labels, count, index, (unsigned)num, stage_rows,
                       (unsigned)post, fix);
  } else if constexpr (MAXROWS > 64 * kWave) {
    if (!ensure_dynamic_lds<nms_scan_kernel<4, W, Fix>>(lds3)) return BEVOPS_FAILURE;
    hipLaunchKernelGGL((nms_scan_kernel<4, W, Fix>), dim3((unsigned)batch), dim3(kScanThreads), lds3, st, boxes_in,
                       scores_in, labels_in, ws, boxes, scores, labels, count, index, (unsigned)num, stage_rows,
                       (unsigned)post, fix);
  }
  return launch_status();
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_bev_nms_workspace_size(int batch, int num) {
  if (batch < 1 || num < 1 || num > kNmsMaxRows) return 0;
  return nms_ws_bytes((size_t)batch, (size_t)num, kBevRowFloats);
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
  if (!workspace_ok(workspace, workspace_bytes, bevops_bev_nms_workspace_size(batch, num))) return BEVOPS_BAD_PARAM;
  const unsigned kmax = nms_kmax(num, pre_max_size);
  const NmsWs ws = nms_ws_carve(workspace, (size_t)batch, kmax, kBevRowFloats);   // (kmax <= num: inside the checked size)
  const unsigned stage_rows = scan_stage_rows(ws, kBevStageBytes, ws.stride);
  const TopCandidates cand{kmax, index_bytes((unsigned)num)};
  const PairRow row{fac};
  const SizeRestore fix{fac, bottom_center};
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == 0)
    return launch_nms<kNmsMaxRows, 9>(boxes_in, scores_in, labels_in, count_in, boxes, scores, labels, count, index, ws,
                                      batch, num, pow2_at_least(kmax), stage_rows, post_max_size, cand, row,
                                      RotatedIou{threshold}, fix, st);
  return launch_nms<kNmsMaxRows, 9>(boxes_in, scores_in, labels_in, count_in, boxes, scores, labels, count, index, ws,
                                    batch, num, pow2_at_least(kmax), stage_rows, post_max_size, cand, row,
                                    CircleDistance{threshold}, fix, st);
}

extern "C" size_t bevops_box_nms_workspace_size(int batch, int num) {
  if (batch < 1 || batch > 65535 || num < 1 || num > kBoxMaxRows) return 0;
  return nms_ws_bytes((size_t)batch, (size_t)num, kBoxRowFloats);
}

extern "C" int bevops_box_nms(const float *boxes_in, const float *scores_in, const int32_t *labels_in,
                              const int32_t *count_in, float *boxes, float *scores, int32_t *labels, int32_t *count,
                              int32_t *index, int batch, int num, float score_threshold, float iou_threshold,
                              int class_aware, int max_out, void *workspace, size_t workspace_bytes, void *stream) {
  if (!boxes_in || !scores_in || !labels_in || !boxes || !scores || !labels || !count || !workspace)
    return BEVOPS_BAD_PARAM;
  if (batch < 1 || num < 1 || (class_aware != 0 && class_aware != 1)) return BEVOPS_BAD_PARAM;
  if (score_threshold != score_threshold || !finite_f(iou_threshold)) return BEVOPS_BAD_PARAM;
  if (num > kBoxMaxRows || batch > 65535) return BEVOPS_NOT_SUPPORTED;
  if (max_out < 1 || max_out > num) return BEVOPS_BAD_PARAM;
  if (!workspace_ok(workspace, workspace_bytes, bevops_box_nms_workspace_size(batch, num))) return BEVOPS_BAD_PARAM;
  const NmsWs ws = nms_ws_carve(workspace, (size_t)batch, (size_t)num, kBoxRowFloats);
  const unsigned stage_rows = scan_stage_rows(ws, kBoxStageBytes, kBoxStageRows);
  return launch_nms<kBoxMaxRows, 4>(boxes_in, scores_in, labels_in, count_in, boxes, scores, labels, count, index, ws,
                                    batch, num, pow2_at_least((unsigned)num), stage_rows, max_out,
                                    ThresholdCandidates{score_threshold}, CornerRow{}, AlignedIou{iou_threshold, class_aware},
                                    NoFix{}, static_cast<hipStream_t>(stream));
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
