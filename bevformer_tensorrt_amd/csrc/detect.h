// What the detection post-processing shares on top of the block selection of topk.h (decode.hip, decode2d.hip, nms.hip):
// typed loads, the emit routine "ranked keys -> compacted fixed-capacity rows", the partial-selection kernel of the
// two-launch decoders, and the argument checks the host entries have in common.  design/postprocess.md has the layout.
#pragma once
#include "topk.h"

namespace bevops {
namespace {

constexpr int kD2MaxBatch = 64;   // per-image host values (borders, scale factors) travel as a kernel argument

template <typename T>
__device__ __forceinline__ float ld(const T *p, size_t i);
template <>
__device__ __forceinline__ float ld<float>(const float *p, size_t i) { return p[i]; }
template <>
__device__ __forceinline__ float ld<__half>(const __half *p, size_t i) { return __half2float(p[i]); }

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ u64 readlane64(u64 v, unsigned lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)lane);
  return ((u64)hi << 32) | lo;
}

struct KeySrc {   // key source of block_topk: keys that are already in memory
  const u64 *p;
  __device__ __forceinline__ u64 operator()(unsigned i) const { return p[i]; }
};

extern __shared__ __attribute__((aligned(16))) char det_smem[];

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

// One output row of W box columns, and rows [from, to) behind the kept ones zeroed by a block of kDecThreads.
template <int W>
__device__ __forceinline__ void write_row(float *boxes, float *scores, int32_t *labels, size_t row, const float *b,
                                          float s, int label) {
#pragma unroll
  for (int c = 0; c < W; ++c) boxes[row * W + c] = b[c];
  scores[row] = s;
  labels[row] = label;
}
template <int W>
__device__ __forceinline__ void zero_tail(float *boxes, float *scores, int32_t *labels, int32_t *index, size_t row0,
                                          unsigned from, unsigned to) {
  for (unsigned r = from + threadIdx.x; r < to; r += kDecThreads) {
#pragma unroll
    for (int c = 0; c < W; ++c) boxes[(row0 + r) * W + c] = 0.f;
    scores[row0 + r] = 0.f;
    labels[row0 + r] = 0;
    if (index) index[row0 + r] = 0;
  }
}

// The epilogue of every decoder: l.list[0..K) holds item b's ranked keys; decode(key, idx, box, s, label) turns one into
// a row and says whether it is kept (it must answer false for a sentinel, whose index is no address).  Kept rows go to
// the front of the item's K output rows in rank order, the rows behind them are zeroed, count[b] is their number.
// Every thread of the block calls it.
template <int W, class Decode>
__device__ __forceinline__ void emit_ranked(const DecLds &l, unsigned K, unsigned b, float *boxes, float *scores,
                                            int32_t *labels, int32_t *count, const Decode &decode) {
  const unsigned t = threadIdx.x;
  const size_t row0 = (size_t)b * K;
  unsigned running = 0;
  for (unsigned r0 = 0; r0 < K; r0 += kDecThreads) {
    const unsigned r = r0 + t;
    float box[W], s = 0.f;
    int label = 0;
    const u64 key = r < K ? l.list[r] : kSentinel;
    const bool keep = decode(key, (unsigned)key, box, s, label);
    const unsigned slot = compact_slot(keep, running, l.part);
    if (keep) write_row<W>(boxes, scores, labels, row0 + slot, box, s, label);
  }
  zero_tail<W>(boxes, scores, labels, nullptr, row0, running, K);
  if (t == 0) count[b] = (int32_t)running;
}

// First launch of a two-launch decoder: block (x, b) selects the top Kslot of its chunk of item b's candidates into
// ws[(b * gridDim.x + x) * Kslot ..]; a chunk with fewer candidates fills up with sentinels.  Chunk: kChunk candidates
// per block, and prepare(lds behind the selection's carve, b, base, n) -> the chunk's key source (it may first put the
// chunk into that LDS; it ends in a barrier if it does).
template <class Chunk>
__global__ __launch_bounds__(kDecThreads) void partial_topk_kernel(Chunk chunk, u64 *__restrict__ ws, unsigned total,
                                                                   unsigned Kslot, unsigned cap, int idx_bytes) {
  const unsigned b = blockIdx.y, t = threadIdx.x;
  const unsigned base = blockIdx.x * (unsigned)Chunk::kChunk;
  const unsigned n = min((unsigned)Chunk::kChunk, total - base);
  const DecLds l = carve(det_smem, cap);
  const auto src = chunk.prepare(det_smem + lds_bytes(cap), b, base, n);
  const unsigned K = min(Kslot, n);
  block_topk(src, n, K, cap, idx_bytes, false, l);
  u64 *out = ws + ((size_t)b * gridDim.x + blockIdx.x) * Kslot;
  for (unsigned i = t; i < Kslot; i += kDecThreads) out[i] = i < K ? l.list[i] : kSentinel;
}

// ---- host side: the checks the entries share (each entry keeps its own order of them)
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline bool finite_f(float v) { return v == v && v <= 3.4028234e38f && v >= -3.4028234e38f; }
inline int dtype_status(int dtype) {   // BEVOPS_SUCCESS for the two float types the decoders read
  if (dtype == BEVOPS_F32 || dtype == BEVOPS_F16) return BEVOPS_SUCCESS;
  return dtype == BEVOPS_I8 ? BEVOPS_NOT_SUPPORTED : BEVOPS_BAD_PARAM;
}
inline bool workspace_ok(const void *workspace, size_t bytes, size_t need) {
  return workspace && bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0;
}

struct ScaleTable {   // per-image divisors of the four box columns
  float v[kD2MaxBatch][4];
};
// 1 everywhere, then the batch rows of host (when given); false for a factor that is zero or not finite
inline bool fill_scale(ScaleTable &s, const float *host, int batch) {
  for (int b = 0; b < kD2MaxBatch; ++b)
    for (int c = 0; c < 4; ++c) s.v[b][c] = 1.f;
  for (int i = 0; host && i < batch * 4; ++i) {
    if (!finite_f(host[i]) || host[i] == 0.f) return false;
    s.v[i / 4][i % 4] = host[i];
  }
  return true;
}

}  // namespace
}  // namespace bevops
