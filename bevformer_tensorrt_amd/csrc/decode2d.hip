// 2-D detection decode on the device: CenterNetHead.get_bboxes / decode_heatmap, YOLOXHead.get_bboxes up to the NMS
// (_bbox_decode, score and label) and the axis-aligned batched NMS behind it.  The statement is the published algorithm
// of mmdet 2.x and mmcv.ops.batched_nms, read against how the reference calls them
// (det2trt/models/detector/{centernet,yolox}.py: post_process, rescale=True); parity with the libraries themselves is
// unpinned (design/postprocess.md).  Fixed-capacity outputs, no host round trip, no launch sized by a device value:
// every entry can be captured.
//
// bevops_centernet_decode, two launches:
//   1. partial: block (x, b) takes kCnChunk cells of item b's C x H x W map, applies the local-maximum test while it
//      reads (each cell and its window once; the thinned values of the chunk live in LDS as 32-bit ranking keys, so
//      the radix passes of topk.h re-read LDS, not the window), and writes the top k of its chunk to the workspace.
//   2. decode: one block per item selects the top k among the partial winners, sorts, gathers wh / offset at the
//      winning cells and writes the boxes.
//   A constant map ties every key; the flat index in the key's low half then decides, chunk by chunk and again in
//   launch 2, so the first k flat indices come out.
// bevops_yolox_decode, one launch: one thread per (item, prior), level found by comparing the prior number with the
//   level offsets (unrolled over the 8 possible levels: no runtime-indexed argument array).
// bevops_box_nms, three launches like csrc/nms.hip:
//   1. rank: one block per item collects the candidate rows (count_in, score >= threshold) as 64-bit keys in LDS,
//      sorts as many as there are (the sort's size follows the candidate count, a power of two), writes per ranked row
//      (x1, y1, x2, y2, area, label).
//   2. mask: a fixed grid of waves strides over the (row i, 64-column word) pairs on or above the diagonal among the
//      M ranked rows: lane = column, the word is the ballot of the pair test.  Nothing is written for rows >= M or for
//      words below the diagonal; launch 3 never reads them.
//   3. scan: wave 0 of one block per item holds the suppressed set (16 384 rows = 256 words: lane w owns words
//      w, w + 64, w + 128, w + 192), the block stages 32 or 64 mask rows per round in LDS; then the block gathers.
// No atomics apart from LDS integer counters whose order is erased by a sort (the histogram of topk.h, the candidate
// collection of launch 1 of the NMS).
#include "topk.h"

namespace bevops {
namespace {

constexpr int kCnChunk = 8192;             // cells per block of the CenterNet partial selection (32 KiB of LDS keys)
constexpr int kCnMaxK = 4096;              // k of bevops_centernet_decode
constexpr long long kCnMaxCells = 1ll << 24;
constexpr int kCnMaxKernel = 7;            // local-maximum windows 1, 3, 5, 7
constexpr int kD2MaxBatch = 64;            // per-image borders / scale factors travel as a kernel argument
constexpr int kYxMaxLevels = 8;
constexpr int kYxThreads = 256;
constexpr long long kYxMaxPriors = 1ll << 24;
constexpr int kBoxMaxRows = 16384;         // num of bevops_box_nms: 256 words of 64 columns
constexpr int kBoxRowFloats = 6;           // x1, y1, x2, y2, area, label (as bits)
constexpr int kBoxMaskThreads = 256;
constexpr int kBoxMaskBlocks = 2048;       // 8 192 waves stride over the (row, word) pairs
constexpr int kBoxScanThreads = 1024;
constexpr int kBoxStageBytes = 64 * 1024;  // mask rows staged in LDS per round of the scan

template <typename T>
__device__ __forceinline__ float ld(const T *p, size_t i);
template <>
__device__ __forceinline__ float ld<float>(const float *p, size_t i) { return p[i]; }
template <>
__device__ __forceinline__ float ld<__half>(const __half *p, size_t i) { return __half2float(p[i]); }

__host__ __device__ inline size_t dec_lds_bytes(unsigned cap) {   // lds_bytes of topk.h, callable from a kernel
  return (size_t)cap * 8 + (256 + kDecWaves + 4) * sizeof(unsigned);
}
__device__ __forceinline__ bool finite_dev(float v) { return fabsf(v) <= 3.4028234e38f; }   // (false for NaN)

// Position of this thread's row among the kept rows of the block's current 1024 ranks (+ running), and the new running
// total.  Every thread of the block calls it.
__device__ __forceinline__ unsigned compact_slot(bool keep, unsigned &running, unsigned *part) {
  const unsigned t = threadIdx.x;
  const unsigned long long m = __ballot(keep);
  const unsigned before = (unsigned)__popcll(m & ((1ull << (t & 63)) - 1ull));
  if ((t & 63) == 0) part[t >> 6] = (unsigned)__popcll(m);
  __syncthreads();
  unsigned off = running, total = running;
  for (unsigned w = 0; w < (unsigned)kDecWaves; ++w) {
    const unsigned v = part[w];
    if (w < (t >> 6)) off += v;
    total += v;
  }
  __syncthreads();   // part is rewritten by the next round
  running = total;
  return off + before;
}

extern __shared__ __attribute__((aligned(16))) char d2_smem[];

// ---------------------------------------------------------------------------------------------------- CenterNet
struct ChunkKeySrc {   // keys of a chunk whose 32-bit rank halves sit in LDS
  const unsigned *v;
  unsigned base;
  __device__ __forceinline__ u64 operator()(unsigned i) const { return ((u64)v[i] << 32) | (base + i); }
};
struct KeySrc {
  const u64 *p;
  __device__ __forceinline__ u64 operator()(unsigned i) const { return p[i]; }
};

// Launch 1: block (x, b) thins its chunk and selects the top Kslot of it into ws[(b * gridDim.x + x) * Kslot ..]; a
// chunk with fewer cells fills up with sentinels.  radius = (kernel - 1) / 2.
template <typename T>
__global__ __launch_bounds__(kDecThreads) void centernet_partial_kernel(const T *__restrict__ heat, u64 *__restrict__ ws,
                                                                         unsigned total, unsigned C, unsigned H, unsigned W,
                                                                         size_t cs, size_t ps, int radius, unsigned Kslot,
                                                                         unsigned cap, int idx_bytes) {
  const unsigned b = blockIdx.y, t = threadIdx.x;
  const unsigned hw = H * W;
  const unsigned base = blockIdx.x * (unsigned)kCnChunk;
  const unsigned n = min((unsigned)kCnChunk, total - base);
  const DecLds l = carve(d2_smem, cap);
  unsigned *vals = reinterpret_cast<unsigned *>(d2_smem + dec_lds_bytes(cap));
  const T *item = heat + (size_t)b * C * hw;
  for (unsigned i = t; i < n; i += kDecThreads) {
    const unsigned f = base + i;
    const unsigned c = f / hw, cell = f % hw;
    const int y = (int)(cell / W), x = (int)(cell % W);
    const T *plane = item + (size_t)c * cs;
    const float v = ld(plane, (size_t)cell * ps);
    const int y0 = max(y - radius, 0), y1 = min(y + radius, (int)H - 1);
    const int x0 = max(x - radius, 0), x1 = min(x + radius, (int)W - 1);
    bool keep = true;   // no cell of the window compares greater (a NaN never does)
    for (int yy = y0; yy <= y1; ++yy)
      for (int xx = x0; xx <= x1; ++xx) keep = keep && !(ld(plane, ((size_t)yy * W + (unsigned)xx) * ps) > v);
    vals[i] = rank_bits(keep ? v : 0.f);
  }
  __syncthreads();
  const ChunkKeySrc src{vals, base};
  const unsigned K = min(Kslot, n);
  block_topk(src, n, K, cap, idx_bytes, false, l);
  u64 *out = ws + ((size_t)b * gridDim.x + blockIdx.x) * Kslot;
  for (unsigned i = t; i < Kslot; i += kDecThreads) out[i] = i < K ? l.list[i] : kSentinel;
}

struct CnMaps {
  const void *wh, *off;
  int cs[2], ps[2];   // channel / pixel strides in elements of wh, offset
};
struct CnMeta {   // per-image host values of the call
  float rx, ry;
  int has_border, has_scale;
  float border[kD2MaxBatch][2];   // (x, y) = mmdet's border[2], border[0]
  float scale[kD2MaxBatch][4];
};

// Launch 2: one block per item; the candidates are the partial winners in ws (nkeys per item).
template <typename T>
__global__ __launch_bounds__(kDecThreads) void centernet_decode_kernel(CnMaps m, const u64 *__restrict__ ws, unsigned nkeys,
                                                                        float *__restrict__ boxes, float *__restrict__ scores,
                                                                        int32_t *__restrict__ labels,
                                                                        int32_t *__restrict__ count, unsigned C, unsigned H,
                                                                        unsigned W, unsigned K, unsigned cap, int idx_bytes,
                                                                        CnMeta g, float score_threshold) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  const unsigned hw = H * W;
  const DecLds l = carve(d2_smem, cap);
  const KeySrc src{ws + (size_t)b * nkeys};
  block_topk(src, nkeys, K, cap, idx_bytes, true, l);
  const T *wh = static_cast<const T *>(m.wh) + (size_t)b * 2 * hw;
  const T *off = static_cast<const T *>(m.off) + (size_t)b * 2 * hw;
  const size_t row0 = (size_t)b * K;
  unsigned running = 0;
  for (unsigned r0 = 0; r0 < K; r0 += kDecThreads) {
    const unsigned r = r0 + t;
    bool keep = false;
    float box[4] = {0.f, 0.f, 0.f, 0.f}, s = 0.f;
    int label = 0;
    const u64 key = r < K ? l.list[r] : kSentinel;
    const unsigned idx = (unsigned)key;
    if (idx < C * hw) {   // (always, for r < K: k <= C H W; a sentinel must never become an address)
      s = rank_logit((unsigned)(key >> 32));
      label = (int)(idx / hw);
      const unsigned cell = idx % hw;
      const float col = (float)(cell % W), row = (float)(cell / W);
      const float w0 = ld(wh, (size_t)cell * m.ps[0]), w1 = ld(wh, (size_t)m.cs[0] + (size_t)cell * m.ps[0]);
      const float o0 = ld(off, (size_t)cell * m.ps[1]), o1 = ld(off, (size_t)m.cs[1] + (size_t)cell * m.ps[1]);
      // every step rounded on its own, as mmdet's tensor ops round it
      const float xs = add_rn(col, o0), ys = add_rn(row, o1);
      const float hx = mul_rn(w0, 0.5f), hy = mul_rn(w1, 0.5f);   // (wh / 2, exact either way)
      box[0] = mul_rn(sub_rn(xs, hx), g.rx);
      box[1] = mul_rn(sub_rn(ys, hy), g.ry);
      box[2] = mul_rn(add_rn(xs, hx), g.rx);
      box[3] = mul_rn(add_rn(ys, hy), g.ry);
      if (g.has_border) {
#pragma unroll
        for (int c = 0; c < 4; ++c) box[c] = sub_rn(box[c], g.border[b][c & 1]);
      }
      if (g.has_scale) {
#pragma unroll
        for (int c = 0; c < 4; ++c) box[c] = box[c] / g.scale[b][c];
      }
      keep = score_threshold < 0.f || s > score_threshold;
    }
    const unsigned slot = compact_slot(keep, running, l.part);
    if (keep) {
#pragma unroll
      for (int c = 0; c < 4; ++c) boxes[(row0 + slot) * 4 + c] = box[c];
      scores[row0 + slot] = s;
      labels[row0 + slot] = label;
    }
  }
  for (unsigned r = running + t; r < K; r += kDecThreads) {
#pragma unroll
    for (int c = 0; c < 4; ++c) boxes[(row0 + r) * 4 + c] = 0.f;
    scores[row0 + r] = 0.f;
    labels[row0 + r] = 0;
  }
  if (t == 0) count[b] = (int32_t)running;
}

inline unsigned cn_blocks(long long total) { return (unsigned)((total + kCnChunk - 1) / kCnChunk); }
inline bool finite_f(float v) { return v == v && v <= 3.4028234e38f && v >= -3.4028234e38f; }

template <typename T>
int launch_centernet(const void *heat, const CnMaps &m, size_t hcs, size_t hps, float *boxes, float *scores,
                     int32_t *labels, int32_t *count, int batch, int C, int H, int W, int K, int kernel, const CnMeta &g,
                     float thr, void *workspace, hipStream_t st) {
  const unsigned total = (unsigned)(C * H * W);
  const int ib = index_bytes(total);
  const unsigned cap = pow2_at_least((unsigned)K);
  const size_t lds1 = dec_lds_bytes(cap) + (size_t)kCnChunk * sizeof(unsigned), lds2 = dec_lds_bytes(cap);
  const unsigned nblk = cn_blocks(total);
  u64 *ws = static_cast<u64 *>(workspace);
  if (!ensure_dynamic_lds<centernet_partial_kernel<T>>(lds1)) return BEVOPS_FAILURE;
  if (!ensure_dynamic_lds<centernet_decode_kernel<T>>(lds2)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(centernet_partial_kernel<T>, dim3(nblk, (unsigned)batch), dim3(kDecThreads), lds1, st,
                     static_cast<const T *>(heat), ws, total, (unsigned)C, (unsigned)H, (unsigned)W, hcs, hps,
                     (kernel - 1) / 2, (unsigned)K, cap, ib);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(centernet_decode_kernel<T>, dim3((unsigned)batch), dim3(kDecThreads), lds2, st, m, ws,
                     nblk * (unsigned)K, boxes, scores, labels, count, (unsigned)C, (unsigned)H, (unsigned)W, (unsigned)K,
                     cap, ib, g, thr);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------- YOLOX
struct YxLevels {
  const void *cls[kYxMaxLevels], *bbox[kYxMaxLevels], *obj[kYxMaxLevels];
  unsigned start[kYxMaxLevels];   // first prior of the level
  int H[kYxMaxLevels], W[kYxMaxLevels], stride[kYxMaxLevels];
  int cs[kYxMaxLevels][3], ps[kYxMaxLevels][3];   // cls, bbox, obj
  int n;
};
struct YxScale {
  int on;
  float v[kD2MaxBatch][4];
};

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename T>
__global__ __launch_bounds__(kYxThreads) void yolox_decode_kernel(YxLevels lv, YxScale sc, float *__restrict__ boxes,
                                                                   float *__restrict__ scores,
                                                                   int32_t *__restrict__ labels, unsigned P, unsigned C) {
  const unsigned p = blockIdx.x * (unsigned)kYxThreads + threadIdx.x, b = blockIdx.y;
  if (p >= P) return;
  // the level of prior p (levels ascend, so the last start at or below p wins); constant indices only
  const T *cls = nullptr, *bbox = nullptr, *obj = nullptr;
  unsigned start = 0;
  int H = 1, W = 1, stride = 1, ccs = 1, cps = 1, bcs = 1, bps = 1, ops = 1;
#pragma unroll
  for (int k = 0; k < kYxMaxLevels; ++k) {
    if (k < lv.n && p >= lv.start[k]) {
      cls = static_cast<const T *>(lv.cls[k]), bbox = static_cast<const T *>(lv.bbox[k]);
      obj = static_cast<const T *>(lv.obj[k]);
      start = lv.start[k], H = lv.H[k], W = lv.W[k], stride = lv.stride[k];
      ccs = lv.cs[k][0], cps = lv.ps[k][0], bcs = lv.cs[k][1], bps = lv.ps[k][1], ops = lv.ps[k][2];
    }
  }
  const unsigned cell = p - start, hw = (unsigned)(H * W);
  const unsigned row = cell / (unsigned)W, col = cell % (unsigned)W;
  const T *pc = cls + (size_t)b * C * hw + (size_t)cell * cps;
  const T *pb = bbox + (size_t)b * 4 * hw + (size_t)cell * bps;
  float best = ld(pc, 0);
  int label = 0;
  for (unsigned c = 1; c < C; ++c) {   // first maximum: ties go to the lower class
    const float v = ld(pc, (size_t)c * ccs);
    if (v > best) best = v, label = (int)c;
  }
  const float fs = (float)stride;
  const float p0 = ld(pb, 0), p1 = ld(pb, (size_t)bcs), p2 = ld(pb, 2 * (size_t)bcs), p3 = ld(pb, 3 * (size_t)bcs);
  const float cx = add_rn(mul_rn(p0, fs), (float)(col * (unsigned)stride));
  const float cy = add_rn(mul_rn(p1, fs), (float)(row * (unsigned)stride));
  const float hx = mul_rn(mul_rn(expf(p2), fs), 0.5f), hy = mul_rn(mul_rn(expf(p3), fs), 0.5f);
  float box[4] = {sub_rn(cx, hx), sub_rn(cy, hy), add_rn(cx, hx), add_rn(cy, hy)};
  if (sc.on) {
#pragma unroll
    for (int c = 0; c < 4; ++c) box[c] = box[c] / sc.v[b][c];
  }
  const float s = mul_rn(sigmoid_f32(ld(obj, (size_t)b * hw + (size_t)cell * ops)), sigmoid_f32(best));
  const size_t o = (size_t)b * P + p;
#pragma unroll
  for (int c = 0; c < 4; ++c) boxes[o * 4 + c] = box[c];
  scores[o] = s;
  labels[o] = label;
}

// ---------------------------------------------------------------------------------------------------- box NMS
struct BoxWs {   // carve of the caller's workspace
  int32_t *ranked;   // [batch] rows that entered the scan
  int32_t *index;    // [batch, num] input row of each ranked row
  float *rows;       // [batch, num, kBoxRowFloats]
  u64 *mask;         // [batch, num, words]
};
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t box_ws_bytes(size_t batch, size_t num) {
  const size_t words = (num + 63) / 64;
  return round_up(batch * 4, 16) + round_up(batch * num * 4, 16) + round_up(batch * num * kBoxRowFloats * 4, 16) +
         batch * num * words * 8;
}
inline BoxWs box_ws_carve(void *ws, size_t batch, size_t num) {
  char *p = static_cast<char *>(ws);
  BoxWs w;
  w.ranked = reinterpret_cast<int32_t *>(p);
  p += round_up(batch * 4, 16);
  w.index = reinterpret_cast<int32_t *>(p);
  p += round_up(batch * num * 4, 16);
  w.rows = reinterpret_cast<float *>(p);
  p += round_up(batch * num * kBoxRowFloats * 4, 16);
  w.mask = reinterpret_cast<u64 *>(p);
  return w;
}

// Launch 1.  Dynamic LDS: cap_max keys, then the carve's histogram words (unused) whose sel[2] counts candidates.
__global__ __launch_bounds__(kDecThreads) void box_rank_kernel(const float *__restrict__ boxes_in,
                                                               const float *__restrict__ scores_in,
                                                               const int32_t *__restrict__ labels_in,
                                                               const int32_t *__restrict__ count_in, BoxWs ws, unsigned num,
                                                               unsigned cap_max, float score_threshold) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  int cnt = count_in ? count_in[b] : (int)num;
  cnt = cnt < 0 ? 0 : cnt;
  const unsigned n = min((unsigned)cnt, num);
  const DecLds l = carve(d2_smem, cap_max);
  if (t == 0) l.sel[2] = 0;
  __syncthreads();
  const float *sc = scores_in + (size_t)b * num;
  for (unsigned i = t; i < n; i += kDecThreads) {
    const float s = sc[i];
    if (s >= score_threshold) {   // (false for NaN)
      const unsigned slot = atomicAdd(&l.sel[2], 1u);   // the order is erased by the sort
      l.list[slot] = ((u64)rank_bits(s) << 32) | i;
    }
  }
  __syncthreads();
  const unsigned M = l.sel[2];
  if (t == 0) ws.ranked[b] = (int32_t)M;
  if (M == 0) return;   // (uniform)
  unsigned cap = 1;
  while (cap < M) cap <<= 1;   // <= cap_max: M <= num
  for (unsigned i = M + t; i < cap; i += kDecThreads) l.list[i] = kSentinel;
  __syncthreads();
  block_sort(cap, l);
  for (unsigned r = t; r < M; r += kDecThreads) {
    const unsigned idx = (unsigned)l.list[r];
    if (idx >= n) continue;   // (never: a sentinel must not become an address)
    const float *p = boxes_in + ((size_t)b * num + idx) * 4;
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    float area = mul_rn(sub_rn(x2, x1), sub_rn(y2, y1));
    if (!(finite_dev(x1) && finite_dev(y1) && finite_dev(x2) && finite_dev(y2))) area = __uint_as_float(0x7fc00000u);
    float *row = ws.rows + ((size_t)b * num + r) * kBoxRowFloats;
    row[0] = x1, row[1] = y1, row[2] = x2, row[3] = y2, row[4] = area;
    row[5] = __int_as_float(labels_in[(size_t)b * num + idx]);
    ws.index[(size_t)b * num + r] = (int32_t)idx;
  }
}

// Launch 2: grid (kBoxMaskBlocks, batch); wave v takes the pairs v, v + waves, ... of (row i, word) with i < M and
// word < ceil(M / 64), and evaluates those on or above the diagonal.
__global__ __launch_bounds__(kBoxMaskThreads) void box_mask_kernel(BoxWs ws, unsigned num, unsigned words, float thr,
                                                                   int class_aware) {
  const unsigned b = blockIdx.y, lane = threadIdx.x & 63u;
  const unsigned M = min((unsigned)max(ws.ranked[b], 0), num);
  const unsigned Mw = (M + 63u) / 64u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBoxMaskThreads / kWave) + (threadIdx.x >> 6));
  const unsigned nwaves = gridDim.x * (kBoxMaskThreads / kWave);
  const float *rows = ws.rows + (size_t)b * num * kBoxRowFloats;
  u64 *mask = ws.mask + (size_t)b * num * words;
  for (unsigned task = wave; task < M * Mw; task += nwaves) {   // (M Mw <= 2^22)
    const unsigned i = task / Mw, word = task % Mw;
    if (word < i / 64u) continue;   // below the diagonal; the diagonal word is always written (launch 3 reads it)
    const unsigned j = word * 64u + lane;
    bool sup = false;
    if (j > i && j < M) {
      const float *ri = rows + (size_t)i * kBoxRowFloats, *rj = rows + (size_t)j * kBoxRowFloats;
      const float iw = fmaxf(sub_rn(fminf(ri[2], rj[2]), fmaxf(ri[0], rj[0])), 0.f);
      const float ih = fmaxf(sub_rn(fminf(ri[3], rj[3]), fmaxf(ri[1], rj[1])), 0.f);
      const float inter = mul_rn(iw, ih);
      const float iou = inter / sub_rn(add_rn(ri[4], rj[4]), inter);   // NaN area: NaN, compares false
      sup = iou > thr && (!class_aware || __float_as_int(ri[5]) == __float_as_int(rj[5]));
    }
    const u64 m = __ballot(sup);
    if (lane == 0) mask[(size_t)i * words + word] = m;
  }
}

__device__ __forceinline__ u64 readlane64(u64 v, unsigned lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)lane);
  return ((u64)hi << 32) | lo;
}

// Launch 3: one block per item.  Dynamic LDS: stage_rows * words mask words, then max_out kept ranks, then the count.
// stage_rows is 32 or 64: one round covers (part of) one 64-row word.
__global__ __launch_bounds__(kBoxScanThreads) void box_scan_kernel(
    const float *__restrict__ boxes_in, const float *__restrict__ scores_in, const int32_t *__restrict__ labels_in, BoxWs ws,
    float *__restrict__ boxes, float *__restrict__ scores, int32_t *__restrict__ labels, int32_t *__restrict__ count,
    int32_t *__restrict__ index, unsigned num, unsigned words, unsigned stage_rows, unsigned post) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  u64 *stage = reinterpret_cast<u64 *>(d2_smem);
  unsigned *kept = reinterpret_cast<unsigned *>(d2_smem + (size_t)stage_rows * words * 8);
  unsigned *total = kept + post;
  const unsigned M = min((unsigned)max(ws.ranked[b], 0), num);
  const unsigned Mw = (M + 63u) / 64u;
  const u64 *mask = ws.mask + (size_t)b * num * words;
  u64 removed[4] = {0, 0, 0, 0};   // wave 0, lane w: words w, w + 64, w + 128, w + 192 of the suppressed set
  unsigned nkept = 0;
  for (unsigned row0 = 0; row0 < M; row0 += stage_rows) {   // (M, nkept, post uniform: every thread takes the same trips)
    const unsigned rows = min(stage_rows, M - row0);
    const unsigned w = __builtin_amdgcn_readfirstlane(row0 / 64u);   // the word these rows are bits of
    for (unsigned e = t; e < rows * Mw; e += kBoxScanThreads) {
      const unsigned r = e / Mw, c = e % Mw;
      if (c >= w) stage[e] = mask[(size_t)(row0 + r) * words + c];   // words below the diagonal were never written
    }
    __syncthreads();
    if (t < (unsigned)kWave) {
      const unsigned first = row0 % 64u;
      const u64 range = (rows >= 64u ? ~0ull : ((1ull << rows) - 1ull)) << first;   // (rows < 64 when first != 0)
      u64 mine = 0;
#pragma unroll
      for (unsigned s = 0; s < 4; ++s)
        if ((w >> 6) == s) mine = readlane64(removed[s], w & 63u);
      u64 cand = ~mine & range;
      while (cand != 0 && nkept < post) {
        const unsigned bit = (unsigned)__ffsll((long long)cand) - 1u;
        const unsigned i = w * 64u + bit;
        if (t == 0) kept[nkept] = i;
        ++nkept;
        u64 own = 0;
#pragma unroll
        for (unsigned s = 0; s < 4; ++s) {
          const unsigned c = s * 64u + t;
          const u64 row = (c >= w && c < Mw) ? stage[(size_t)(i - row0) * Mw + c] : 0ull;
          removed[s] |= row;
          if ((w >> 6) == s) own = readlane64(row, w & 63u);
        }
        cand &= ~own;
        cand &= ~((2ull << bit) - 1ull);   // rows at and before i are decided
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
  for (unsigned r = t; r < post; r += kBoxScanThreads) {
    float box[4] = {0.f, 0.f, 0.f, 0.f}, s = 0.f;
    int label = 0, idx = 0;
    if (r < nkept) {
      idx = ws.index[(size_t)b * num + kept[r]];
      const size_t at = (size_t)b * num + (unsigned)idx;
#pragma unroll
      for (int c = 0; c < 4; ++c) box[c] = boxes_in[at * 4 + c];
      s = scores_in[at];
      label = labels_in[at];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) boxes[(out0 + r) * 4 + c] = box[c];
    scores[out0 + r] = s;
    labels[out0 + r] = label;
    if (index) index[out0 + r] = idx;
  }
  if (t == 0) count[b] = (int32_t)nkept;
}

inline unsigned box_stage_rows(unsigned words) { return words * 64u * 8u <= (unsigned)kBoxStageBytes ? 64u : 32u; }

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_centernet_decode_workspace_size(int batch, int num_classes, int height, int width, int k) {
  if (batch < 1 || batch > kD2MaxBatch || num_classes < 1 || height < 1 || width < 1 || k < 1) return 0;
  const long long total = (long long)num_classes * height * width;
  if ((long long)num_classes * height > kCnMaxCells || total > kCnMaxCells || k > kCnMaxK || k > total) return 0;
  return (size_t)batch * cn_blocks(total) * (size_t)k * sizeof(u64);
}

extern "C" int bevops_centernet_decode(int dtype, const void *heatmap, const void *wh, const void *offset,
                                       const int32_t *strides_host, float *boxes, float *scores, int32_t *labels,
                                       int32_t *count, int batch, int num_classes, int map_h, int map_w, int k, int kernel,
                                       int inp_h, int inp_w, const float *border_host, const float *scale_factor_host,
                                       float score_threshold, void *workspace, size_t workspace_bytes, void *stream) {
  if (!heatmap || !wh || !offset || !strides_host || !boxes || !scores || !labels || !count) return BEVOPS_BAD_PARAM;
  if (batch < 1 || num_classes < 1 || map_h < 1 || map_w < 1 || inp_h < 1 || inp_w < 1 || kernel < 1)
    return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F32 && dtype != BEVOPS_F16) return dtype == BEVOPS_I8 ? BEVOPS_NOT_SUPPORTED : BEVOPS_BAD_PARAM;
  if (score_threshold != score_threshold) return BEVOPS_BAD_PARAM;
  for (int i = 0; i < 6; ++i)
    if (strides_host[i] < 1) return BEVOPS_BAD_PARAM;
  const long long total = (long long)num_classes * map_h * map_w;
  if ((long long)num_classes * map_h > kCnMaxCells || total > kCnMaxCells || k < 1 || k > kCnMaxK || k > total ||
      batch > kD2MaxBatch || kernel > kCnMaxKernel || (kernel & 1) == 0)
    return BEVOPS_NOT_SUPPORTED;
  CnMeta g;
  g.rx = (float)((double)inp_w / map_w), g.ry = (float)((double)inp_h / map_h);
  g.has_border = border_host != nullptr, g.has_scale = scale_factor_host != nullptr;
  for (int b = 0; b < kD2MaxBatch; ++b) {
    for (int c = 0; c < 2; ++c) g.border[b][c] = 0.f;
    for (int c = 0; c < 4; ++c) g.scale[b][c] = 1.f;
  }
  for (int b = 0; b < batch; ++b) {
    for (int c = 0; c < 2 && border_host; ++c) {
      if (!finite_f(border_host[b * 2 + c])) return BEVOPS_BAD_PARAM;
      g.border[b][c] = border_host[b * 2 + c];
    }
    for (int c = 0; c < 4 && scale_factor_host; ++c) {
      const float f = scale_factor_host[b * 4 + c];
      if (!finite_f(f) || f == 0.f) return BEVOPS_BAD_PARAM;
      g.scale[b][c] = f;
    }
  }
  const size_t need = bevops_centernet_decode_workspace_size(batch, num_classes, map_h, map_w, k);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return BEVOPS_BAD_PARAM;
  CnMaps m;
  m.wh = wh, m.off = offset;
  m.cs[0] = strides_host[2], m.ps[0] = strides_host[3], m.cs[1] = strides_host[4], m.ps[1] = strides_host[5];
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == BEVOPS_F32)
    return launch_centernet<float>(heatmap, m, (size_t)strides_host[0], (size_t)strides_host[1], boxes, scores, labels,
                                   count, batch, num_classes, map_h, map_w, k, kernel, g, score_threshold, workspace, st);
  return launch_centernet<__half>(heatmap, m, (size_t)strides_host[0], (size_t)strides_host[1], boxes, scores, labels,
                                  count, batch, num_classes, map_h, map_w, k, kernel, g, score_threshold, workspace, st);
}

extern "C" int bevops_yolox_decode(int dtype, const void *const *cls_host, const void *const *bbox_host,
                                   const void *const *obj_host, const int32_t *level_shapes_host,
                                   const int32_t *strides_host, float *boxes, float *scores, int32_t *labels, int batch,
                                   int num_levels, int num_classes, const float *scale_factor_host, void *stream) {
  if (!cls_host || !bbox_host || !obj_host || !level_shapes_host || !strides_host || !boxes || !scores || !labels)
    return BEVOPS_BAD_PARAM;
  if (batch < 1 || num_levels < 1 || num_classes < 1) return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F32 && dtype != BEVOPS_F16) return dtype == BEVOPS_I8 ? BEVOPS_NOT_SUPPORTED : BEVOPS_BAD_PARAM;
  if (num_levels > kYxMaxLevels || batch > kD2MaxBatch) return BEVOPS_NOT_SUPPORTED;
  YxLevels lv;
  lv.n = num_levels;
  long long priors = 0;
  for (int k = 0; k < kYxMaxLevels; ++k) {
    lv.cls[k] = lv.bbox[k] = lv.obj[k] = nullptr;
    lv.start[k] = 0, lv.H[k] = lv.W[k] = lv.stride[k] = 1;
    for (int c = 0; c < 3; ++c) lv.cs[k][c] = lv.ps[k][c] = 1;
  }
  for (int k = 0; k < num_levels; ++k) {
    const int H = level_shapes_host[3 * k], W = level_shapes_host[3 * k + 1], s = level_shapes_host[3 * k + 2];
    if (!cls_host[k] || !bbox_host[k] || !obj_host[k] || H < 1 || W < 1 || s < 1) return BEVOPS_BAD_PARAM;
    for (int c = 0; c < 6; ++c)
      if (strides_host[6 * k + c] < 1) return BEVOPS_BAD_PARAM;
    if ((long long)H * W > kYxMaxPriors || (long long)(H > W ? H : W) * s > kYxMaxPriors) return BEVOPS_NOT_SUPPORTED;
    lv.cls[k] = cls_host[k], lv.bbox[k] = bbox_host[k], lv.obj[k] = obj_host[k];
    lv.start[k] = (unsigned)priors, lv.H[k] = H, lv.W[k] = W, lv.stride[k] = s;
    for (int c = 0; c < 3; ++c) lv.cs[k][c] = strides_host[6 * k + 2 * c], lv.ps[k][c] = strides_host[6 * k + 2 * c + 1];
    priors += (long long)H * W;
    if (priors > kYxMaxPriors) return BEVOPS_NOT_SUPPORTED;
  }
  YxScale sc;
  sc.on = scale_factor_host != nullptr;
  for (int b = 0; b < kD2MaxBatch; ++b)
    for (int c = 0; c < 4; ++c) sc.v[b][c] = 1.f;
  for (int b = 0; b < batch && scale_factor_host; ++b)
    for (int c = 0; c < 4; ++c) {
      const float f = scale_factor_host[b * 4 + c];
      if (!finite_f(f) || f == 0.f) return BEVOPS_BAD_PARAM;
      sc.v[b][c] = f;
    }
  const unsigned P = (unsigned)priors;
  const dim3 grid((P + kYxThreads - 1) / kYxThreads, (unsigned)batch);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == BEVOPS_F32)
    hipLaunchKernelGGL(yolox_decode_kernel<float>, grid, dim3(kYxThreads), 0, st, lv, sc, boxes, scores, labels, P,
                       (unsigned)num_classes);
  else
    hipLaunchKernelGGL(yolox_decode_kernel<__half>, grid, dim3(kYxThreads), 0, st, lv, sc, boxes, scores, labels, P,
                       (unsigned)num_classes);
  return launch_status();
}

extern "C" size_t bevops_box_nms_workspace_size(int batch, int num) {
  if (batch < 1 || batch > 65535 || num < 1 || num > kBoxMaxRows) return 0;
  return box_ws_bytes((size_t)batch, (size_t)num);
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
  if (workspace_bytes < bevops_box_nms_workspace_size(batch, num) || (reinterpret_cast<uintptr_t>(workspace) & 7u))
    return BEVOPS_BAD_PARAM;
  const unsigned words = ((unsigned)num + 63u) / 64u;
  const BoxWs ws = box_ws_carve(workspace, (size_t)batch, (size_t)num);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned cap = pow2_at_least((unsigned)num);
  const size_t lds1 = lds_bytes(cap);
  if (!ensure_dynamic_lds<box_rank_kernel>(lds1)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(box_rank_kernel, dim3((unsigned)batch), dim3(kDecThreads), lds1, st, boxes_in, scores_in, labels_in,
                     count_in, ws, (unsigned)num, cap, score_threshold);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(box_mask_kernel, dim3(kBoxMaskBlocks, (unsigned)batch), dim3(kBoxMaskThreads), 0, st, ws,
                     (unsigned)num, words, iou_threshold, class_aware);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  const unsigned stage_rows = box_stage_rows(words);
  const size_t lds3 = (size_t)stage_rows * words * 8 + (size_t)max_out * 4 + 16;   // <= 64 KiB + 64 KiB + 16
  if (!ensure_dynamic_lds<box_scan_kernel>(lds3)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(box_scan_kernel, dim3((unsigned)batch), dim3(kBoxScanThreads), lds3, st, boxes_in, scores_in,
                     labels_in, ws, boxes, scores, labels, count, index, (unsigned)num, words, stage_rows,
                     (unsigned)max_out);
  return launch_status();
}
