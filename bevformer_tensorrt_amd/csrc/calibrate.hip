// PTQ calibration on the device (design/calibration.md): a running 2048-bin histogram of |x| per site whose range
// doubles when a batch exceeds it (bevformer_tensorrt_amd/quantization.py: _Histogram's rule), and the two threshold
// searches over it -- TensorRT's "entropy calibration 2" (argmin KL(P || Q) over the clip bin) and the percentile rule.
// The reference leaves calibration to TensorRT (det2trt/quantization/calibrator_trt.py:6-92); nothing here restates
// its code.  Only integer atomics touch the state, so every result is independent of the order of arrival.
#include <math.h>

#include "common.h"

namespace bevops {
namespace {

constexpr int kBins = 2048;
constexpr int kLevels = 128;
constexpr int kCand = kBins - kLevels + 1;   // clip candidates i = 128 .. 2048 (bins kept)
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;             // grid-stride passes: four blocks for each of the 256 CUs

struct CalibState {
  float range;                // 0: no data yet
  float amax;                 // running maximum of |x|
  float batch_amax;           // this batch's maximum; 0 between calls
  uint32_t batches;
  unsigned long long count;   // finite elements binned
  unsigned long long nonfinite;
  uint32_t batch_finite;      // set by the maximum pass when the batch has a finite element; 0 between calls
  uint32_t zero[7];
  unsigned long long hist[kBins];
};
static_assert(sizeof(CalibState) == 64 + kBins * 8, "state layout");

__device__ __forceinline__ bool finite_bits(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }

template <typename T>
struct Elem;
template <>
struct Elem<float> {
  static constexpr int kVec = 4;
  static __device__ __forceinline__ float one(const float *p, size_t i) { return p[i]; }
  static __device__ __forceinline__ void vec(const u32x4 &v, float *f) {
    for (int j = 0; j < 4; ++j) f[j] = __uint_as_float(v[j]);
  }
};
template <>
struct Elem<__half> {
  static constexpr int kVec = 8;
  static __device__ __forceinline__ float one(const __half *p, size_t i) { return __half2float(p[i]); }
  static __device__ __forceinline__ void vec(const u32x4 &v, float *f) {
    for (int j = 0; j < 4; ++j) {
      f[2 * j] = h2f_lo(v[j]);
      f[2 * j + 1] = h2f_hi(v[j]);
    }
  }
};

// elements in front of the first 16-byte boundary (x is element-aligned)
template <typename T>
__host__ __device__ inline size_t head_count(const T *x, size_t count) {
  const size_t mis = reinterpret_cast<uintptr_t>(x) & 15u;
  const size_t head = mis ? (16 - mis) / sizeof(T) : 0;
  return head < count ? head : count;
}

// ---- pass 1: maximum of |x| over the finite elements (integer max of the bit pattern: the values are non-negative)
template <typename T>
__global__ __launch_bounds__(kThreads) void calib_max_kernel(const T *__restrict__ x, size_t count, CalibState *st) {
  constexpr int V = Elem<T>::kVec;
  __shared__ unsigned s_max, s_nonfinite, s_finite;
  if (threadIdx.x == 0) s_max = s_nonfinite = s_finite = 0;
  __syncthreads();
  unsigned vmax = 0, nonfinite = 0, finite = 0;
  auto see = [&](float f) {
    const unsigned u = __float_as_uint(f) & 0x7fffffffu;
    if (finite_bits(u)) {
      vmax = u > vmax ? u : vmax;
      finite = 1;
    } else {
      ++nonfinite;
    }
  };
  const size_t head = head_count(x, count);
  const size_t nvec = (count - head) / V;
  const size_t tail = head + nvec * V;
  if (blockIdx.x == 0) {
    if (threadIdx.x < head) see(Elem<T>::one(x, threadIdx.x));
    if (tail + threadIdx.x < count) see(Elem<T>::one(x, tail + threadIdx.x));
  }
  const u32x4 *xv = reinterpret_cast<const u32x4 *>(x + head);
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += (size_t)gridDim.x * kThreads) {
    float f[V];
    Elem<T>::vec(xv[i], f);
    for (int j = 0; j < V; ++j) see(f[j]);
  }
  if (finite) {
    atomicMax(&s_max, vmax);
    atomicOr(&s_finite, 1u);
  }
  if (nonfinite) atomicAdd(&s_nonfinite, nonfinite);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_finite) {
      atomicMax(reinterpret_cast<unsigned *>(&st->batch_amax), s_max);
      atomicOr(&st->batch_finite, 1u);
    }
    if (s_nonfinite) atomicAdd(&st->nonfinite, (unsigned long long)s_nonfinite);
  }
}

// ---- pass 2: one block; the range doubles until it holds the batch, bins merge 2^d to one
__global__ __launch_bounds__(kThreads) void calib_rescale_kernel(CalibState *st) {
  __shared__ unsigned long long old[kBins];
  const float batch_amax = st->batch_amax;
  const bool any = st->batch_finite != 0;
  float range = st->range;
  const float amax = st->amax;
  int d = 0;
  if (any) {
    if (range == 0.0f) range = fmaxf(batch_amax, 1e-12f);
    while (batch_amax > range) {
      range *= 2.0f;     // exact
      ++d;
    }
  }
  if (d > 0) {
    for (int k = threadIdx.x; k < kBins; k += kThreads) old[k] = st->hist[k];
    __syncthreads();     // every thread has also read the header by now
    const int sh = d < 11 ? d : 11;
    const int live = kBins >> sh;
    for (int j = threadIdx.x; j < kBins; j += kThreads) {
      unsigned long long s = 0;
      if (j < live)
        for (int k = j << sh; k < (j + 1) << sh; ++k) s += old[k];
      st->hist[j] = s;
    }
  } else {
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (any) {
      st->range = range;
      st->amax = fmaxf(amax, batch_amax);
    }
    st->batch_amax = 0.0f;
    st->batch_finite = 0;
    st->batches += 1;
  }
}

// ---- pass 3: per-block histogram in LDS, flushed with 64-bit integer atomics
template <typename T>
__global__ __launch_bounds__(kThreads) void calib_hist_kernel(const T *__restrict__ x, size_t count, CalibState *st) {
  constexpr int V = Elem<T>::kVec;
  __shared__ unsigned bins[kBins];
  __shared__ unsigned s_count;
  const float range = st->range;
  if (range == 0.0f) return;     // no finite element yet: nothing to bin (uniform over the grid)
  for (int k = threadIdx.x; k < kBins; k += kThreads) bins[k] = 0;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  const float inv = __fdiv_rn(2048.0f, range);
  // bin of a finite value, -1 otherwise; fminf keeps the conversion in range whatever the input
  auto bin_of = [&](float f) {
    if (!finite_bits(__float_as_uint(f))) return -1;
    const int b = (int)fminf(__fmul_rn(fabsf(f), inv), 2047.0f);
    return b < 2047 ? b : 2047;
  };
  const size_t head = head_count(x, count);
  const size_t nvec = (count - head) / V;
  const size_t tail = head + nvec * V;
  if (blockIdx.x == 0) {
    if (threadIdx.x < head) {
      const int b = bin_of(Elem<T>::one(x, threadIdx.x));
      if (b >= 0) atomicAdd(&bins[b], 1u);
    }
    if (tail + threadIdx.x < count) {
      const int b = bin_of(Elem<T>::one(x, tail + threadIdx.x));
      if (b >= 0) atomicAdd(&bins[b], 1u);
    }
  }
  // The zero bin (half of a ReLU output) is counted per wave with a ballot instead of 64 atomics on one LDS address.
  // The loop bound is the same for every lane of a wave, so the ballot sees the whole wave in every trip.
  const u32x4 *xv = reinterpret_cast<const u32x4 *>(x + head);
  unsigned zeros = 0;
  for (size_t base = (size_t)blockIdx.x * kThreads + (threadIdx.x & ~(kWave - 1)); base < nvec;
       base += (size_t)gridDim.x * kThreads) {
    const size_t i = base + (threadIdx.x & (kWave - 1));
    const bool live = i < nvec;
    float f[V];
    if (live) Elem<T>::vec(xv[i], f);
    for (int j = 0; j < V; ++j) {
      const int b = live ? bin_of(f[j]) : -1;
      zeros += __popcll(__ballot(b == 0));
      if (b > 0) atomicAdd(&bins[b], 1u);
    }
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && zeros) atomicAdd(&bins[0], zeros);
  __syncthreads();
  unsigned mine = 0;
  for (int k = threadIdx.x; k < kBins; k += kThreads) {
    const unsigned v = bins[k];
    if (v) {
      atomicAdd(&st->hist[k], (unsigned long long)v);
      mine += v;
    }
  }
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_count) atomicAdd(&st->count, (unsigned long long)s_count);
}

template <typename T>
int collect(const void *x, size_t count, CalibState *st, hipStream_t stream) {
  const T *p = static_cast<const T *>(x);
  const size_t nvec = (count - head_count(p, count)) / Elem<T>::kVec;
  size_t blocks = (nvec + kThreads - 1) / kThreads;
  blocks = blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks);
  calib_max_kernel<T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(p, count, st);
  calib_rescale_kernel<<<dim3(1), dim3(kThreads), 0, stream>>>(st);
  calib_hist_kernel<T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(p, count, st);
  return launch_status();
}

// ---- threshold search
// sum of v over the block in a fixed order (a binary tree over the thread index); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double *red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// first bin of level l when i bins are kept: the smallest k with (2k + 1) 64 > l i, i.e. with
// ceil((k + 0.5) 128 / i) - 1 >= l
__device__ __forceinline__ int level_begin(int l, int i) { return (l * i / 64 + 1) / 2; }

// One block per (candidate, state): KL(P || Q) of entropy_threshold_bin for i = 128 + candidate kept bins.
__global__ __launch_bounds__(kThreads) void calib_kl_kernel(const unsigned char *states, size_t stride, double *kl_all) {
  __shared__ double h[kBins];
  __shared__ double red[kThreads];
  __shared__ double qv[kLevels], lsum[kLevels], lcnt[kLevels];
  const int s = blockIdx.x / kCand, c = blockIdx.x % kCand;
  const int i = kLevels + c;
  const CalibState *st = reinterpret_cast<const CalibState *>(states + (size_t)s * stride);
  if (st->count == 0) return;    // the argmin pass answers -1 without reading the curve
  for (int k = threadIdx.x; k < kBins; k += kThreads) h[k] = (double)st->hist[k == 0 ? 1 : k];   // h[0] = h[1]
  __syncthreads();
  // level sums and non-empty counts; thread l owns level l's contiguous bins (all integers: exact in any order)
  double total_part = 0.0;
  for (int k = threadIdx.x; k < kBins; k += kThreads) total_part += h[k];
  if (threadIdx.x < kLevels) {
    const int l = threadIdx.x;
    double sum = 0.0, cnt = 0.0;
    for (int k = level_begin(l, i); k < level_begin(l + 1, i); ++k) {
      sum += h[k];
      cnt += h[k] > 0.0 ? 1.0 : 0.0;
    }
    lsum[l] = sum;
    lcnt[l] = cnt;
    qv[l] = sum / fmax(cnt, 1.0);
  }
  const double psum = block_sum(total_part, red);                                           // P keeps the whole mass
  const double kept = block_sum(threadIdx.x < kLevels ? lsum[threadIdx.x] : 0.0, red);
  const double qsum = block_sum(threadIdx.x < kLevels ? qv[threadIdx.x] * lcnt[threadIdx.x] : 0.0, red);
  double klv = INFINITY;
  if (psum > 0.0 && qsum > 0.0) {     // uniform over the block
    const double tail = psum - kept;
    double part = 0.0;
    for (int k = threadIdx.x; k < i; k += kThreads) {
      const double p = h[k] + (k == i - 1 ? tail : 0.0);
      if (p > 0.0) {
        const int lv = ((2 * k + 1) * 64 + i - 1) / i - 1;
        const double q = h[k] > 0.0 ? qv[lv < 0 ? 0 : (lv > kLevels - 1 ? kLevels - 1 : lv)] : 0.0;
        const double pn = p / psum;
        part += pn * log(pn / fmax(q / qsum, 1e-12));
      }
    }
    klv = block_sum(part, red);
  }
  if (threadIdx.x == 0) kl_all[(size_t)s * kCand + c] = klv;
}

// One block per state: first minimum of the curve, minus 1 + 128; 2047 when every candidate is infinite.
__global__ __launch_bounds__(kThreads) void calib_argmin_kernel(const unsigned char *states, size_t stride,
                                                                const double *kl_all, int32_t *bins, double *kl) {
  __shared__ double bv[kThreads];
  __shared__ int bi[kThreads];
  const int s = blockIdx.x;
  const CalibState *st = reinterpret_cast<const CalibState *>(states + (size_t)s * stride);
  if (st->count == 0) {
    if (threadIdx.x == 0) {
      bins[s] = -1;
      if (kl) kl[s] = INFINITY;
    }
    return;
  }
  double best = INFINITY;
  int at = kCand;
  for (int c = threadIdx.x; c < kCand; c += kThreads) {
    const double v = kl_all[(size_t)s * kCand + c];
    if (v < best) {
      best = v;
      at = c;
    }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = at;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const double v = bv[threadIdx.x + w];
      const int a = bi[threadIdx.x + w];
      if (v < bv[threadIdx.x] || (v == bv[threadIdx.x] && a < bi[threadIdx.x])) {
        bv[threadIdx.x] = v;
        bi[threadIdx.x] = a;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool found = bi[0] < kCand && bv[0] < INFINITY;
    bins[s] = found ? kLevels + bi[0] - 1 : kBins - 1;
    if (kl) kl[s] = found ? bv[0] : INFINITY;
  }
}

// One block per state: first k with cdf[k] >= cdf[2047] * percentile / 100.0, capped at 2047.
__global__ __launch_bounds__(kThreads) void calib_percentile_kernel(const unsigned char *states, size_t stride,
                                                                    double percentile, int32_t *bins, double *kl) {
  constexpr int kPer = kBins / kThreads;
  __shared__ unsigned long long part[kThreads];
  __shared__ int first;
  const int s = blockIdx.x;
  const CalibState *st = reinterpret_cast<const CalibState *>(states + (size_t)s * stride);
  if (threadIdx.x == 0 && kl) kl[s] = 0.0;
  if (st->count == 0) {
    if (threadIdx.x == 0) bins[s] = -1;
    return;
  }
  unsigned long long v[kPer], sum = 0;
  for (int j = 0; j < kPer; ++j) {
    v[j] = st->hist[threadIdx.x * kPer + j];
    sum += v[j];
  }
  part[threadIdx.x] = sum;
  if (threadIdx.x == 0) first = kBins - 1;
  __syncthreads();
  unsigned long long before = 0, total = 0;
  for (int t = 0; t < kThreads; ++t) {
    if (t == (int)threadIdx.x) before = total;
    total += part[t];
  }
  const double want = (double)total * percentile / 100.0;
  unsigned long long cdf = before;
  for (int j = 0; j < kPer; ++j) {
    cdf += v[j];
    if ((double)cdf >= want) {
      atomicMin(&first, (int)threadIdx.x * kPer + j);
      break;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) bins[s] = first;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_calib_state_size(void) { return sizeof(CalibState); }

extern "C" int bevops_calib_collect(int dtype, const void *x, size_t count, void *state, void *stream) {
  if (dtype != BEVOPS_F32 && dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  if (count == 0) return BEVOPS_SUCCESS;
  const size_t esize = dtype == BEVOPS_F32 ? 4 : 2;
  if (!x || !state || (reinterpret_cast<uintptr_t>(x) & (esize - 1)) || (reinterpret_cast<uintptr_t>(state) & 63u))
    return BEVOPS_BAD_PARAM;
  if (count > ((size_t)1 << 40)) return BEVOPS_NOT_SUPPORTED;   // a block's 32-bit bins hold its share up to here
  CalibState *st = static_cast<CalibState *>(state);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == BEVOPS_F32 ? collect<float>(x, count, st, s) : collect<__half>(x, count, st, s);
}

extern "C" size_t bevops_calib_threshold_workspace_size(int num_states) {
  return num_states > 0 ? (size_t)num_states * kCand * sizeof(double) : 0;
}

extern "C" int bevops_calib_threshold(int method, double percentile, const void *states, int num_states,
                                      size_t state_stride, int32_t *bins, double *kl, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  if (method != 0 && method != 1) return BEVOPS_NOT_SUPPORTED;
  if (!states || !bins || num_states <= 0 || state_stride < sizeof(CalibState) || (state_stride & 63u) ||
      (reinterpret_cast<uintptr_t>(states) & 63u) || (reinterpret_cast<uintptr_t>(bins) & 3u) ||
      (reinterpret_cast<uintptr_t>(kl) & 7u) || !(percentile >= 0.0))
    return BEVOPS_BAD_PARAM;
  if (!workspace || workspace_bytes < bevops_calib_threshold_workspace_size(num_states) ||
      (reinterpret_cast<uintptr_t>(workspace) & 7u))
    return BEVOPS_BAD_PARAM;
  if (num_states > (1 << 20)) return BEVOPS_NOT_SUPPORTED;      // candidates x states is the grid
  const unsigned char *p = static_cast<const unsigned char *>(states);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (method == 0) {
    double *curve = static_cast<double *>(workspace);
    calib_kl_kernel<<<dim3((unsigned)num_states * kCand), dim3(kThreads), 0, s>>>(p, state_stride, curve);
    calib_argmin_kernel<<<dim3(num_states), dim3(kThreads), 0, s>>>(p, state_stride, curve, bins, kl);
  } else {
    calib_percentile_kernel<<<dim3(num_states), dim3(kThreads), 0, s>>>(p, state_stride, percentile, bins, kl);
  }
  return launch_status();
}
