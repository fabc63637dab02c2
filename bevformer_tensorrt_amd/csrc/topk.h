// Block-wide selection shared by the detection decoders (decode.hip, decode2d.hip) and the NMS (nms.hip), which reach
// it through detect.h: the 64-bit ranking key, an 8-bit radix select over such keys and a bitonic sort of the winners in LDS.
//
// Ranking rule (include/bevops.h, design/postprocess.md): candidates rank by an fp32 value, larger first; equal values
// (-0 counts as +0) rank by lower flat index first.  Both go into one 64-bit key,
//   key = (~monotone(value) << 32) | flat_index,
// so "rank order" is ascending key order and all keys of one batch item are distinct.  The LDS histogram uses integer
// atomics; counts do not depend on their order, and the order in which winners are collected is erased by the sort,
// so results are bit-reproducible.
#pragma once
#include "common.h"

namespace bevops {
namespace {

constexpr int kDecThreads = 1024;
constexpr int kDecWaves = kDecThreads / kWave;
constexpr unsigned long long kSentinel = ~0ull;   // ranks behind every candidate (flat index 0xffffffff is never real)

typedef unsigned long long u64;

// smaller = ranks earlier: ~(the usual order-preserving map of a float onto unsigned)
__device__ __forceinline__ unsigned rank_bits(float f) {
  f = (f == 0.f) ? 0.f : f;   // -0 ranks as +0
  const unsigned u = __float_as_uint(f);
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~o;
}
__device__ __forceinline__ float rank_logit(unsigned k) {
  const unsigned o = ~k;
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct DecLds {   // carve of the dynamic LDS region (every offset a multiple of 16)
  u64 *list;        // [cap] winners
  unsigned *hist;   // [256]
  unsigned *part;   // [kDecWaves] wave totals
  unsigned *sel;    // [4] digit, remaining rank, collect counter
};
__device__ __forceinline__ DecLds carve(char *smem, unsigned cap) {
  DecLds l;
  l.list = reinterpret_cast<u64 *>(smem);
  l.hist = reinterpret_cast<unsigned *>(smem + (size_t)cap * 8);
  l.part = l.hist + 256;
  l.sel = l.part + kDecWaves;
  return l;
}
__host__ __device__ inline size_t lds_bytes(unsigned cap) { return (size_t)cap * 8 + (256 + kDecWaves + 4) * sizeof(unsigned); }
inline unsigned pow2_at_least(unsigned v) {
  unsigned p = 1;
  while (p < v) p <<= 1;
  return p;
}

// Ascending bitonic sort of l.list[0..cap), cap a power of two.  Every thread of the block calls it.
__device__ __forceinline__ void block_sort(unsigned cap, const DecLds &l) {
  const unsigned t = threadIdx.x;
  for (unsigned k2 = 2; k2 <= cap; k2 <<= 1) {
    for (unsigned j = k2 >> 1; j > 0; j >>= 1) {
      for (unsigned i = t; i < cap; i += kDecThreads) {
        const unsigned p = i ^ j;
        if (p > i) {
          const u64 a = l.list[i], b = l.list[p];
          if ((a > b) == ((i & k2) == 0)) {
            l.list[i] = b;
            l.list[p] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

// The K smallest of the n distinct keys src(0..n), ascending, into l.list[0..K); l.list[K..cap) = sentinel.
// Needs 1 <= K <= n, K <= cap, cap a power of two.  idx_bytes: how many low bytes of the flat index can be non-zero.
// sorted = false skips the sort (the winners are then in no particular order).
template <typename Src>
__device__ void block_topk(const Src &src, unsigned n, unsigned K, unsigned cap, int idx_bytes, bool sorted,
                           const DecLds &l) {
  const unsigned t = threadIdx.x;
  u64 prefix = 0, mask = 0;
  unsigned k = K;
  for (int pass = 0; pass < 4 + idx_bytes; ++pass) {
    const int shift = pass < 4 ? 56 - 8 * pass : 8 * (idx_bytes - 1 - (pass - 4));
    if (t < 256) l.hist[t] = 0;
    __syncthreads();
    for (unsigned i = t; i < n; i += kDecThreads) {
      const u64 key = src(i);
      if ((key & mask) == prefix) atomicAdd(&l.hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    // inclusive scan of the 256 bins by the first four waves
    unsigned c = 0, incl = 0;
    if (t < 256) {
      c = incl = l.hist[t];
      for (int d = 1; d < kWave; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, kWave);
        if ((int)(t & 63) >= d) incl += up;
      }
      if ((t & 63) == 63) l.part[t >> 6] = incl;
    }
    __syncthreads();
    if (t < 256) {
      for (unsigned w = 0; w < (t >> 6); ++w) incl += l.part[w];
      const unsigned excl = incl - c;
      if (excl < k && k <= incl) {   // exactly one bin
        l.sel[0] = t;
        l.sel[1] = k - excl;
      }
    }
    __syncthreads();
    prefix |= (u64)l.sel[0] << shift;
    mask |= (u64)255 << shift;
    k = l.sel[1];
    __syncthreads();   // sel is rewritten by the next pass
  }
  // prefix is now the K-th smallest key
  if (t == 0) l.sel[2] = 0;
  __syncthreads();
  for (unsigned i = t; i < n; i += kDecThreads) {
    const u64 key = src(i);
    if (key <= prefix) {
      const unsigned slot = atomicAdd(&l.sel[2], 1u);
      if (slot < cap) l.list[slot] = key;
    }
  }
  for (unsigned i = K + t; i < cap; i += kDecThreads) l.list[i] = kSentinel;
  __syncthreads();
  if (sorted) block_sort(cap, l);
}

inline int index_bytes(unsigned n) {   // low bytes of a flat index below n that can be non-zero
  int b = 1;
  while (b < 4 && ((n - 1) >> (8 * b)) != 0) ++b;
  return b;
}

}  // namespace
}  // namespace bevops
